"""Host-only checks of the preset-dictionary calls: tools/dict_host_check.cpp
(the dictionary tail / history layout and the FDICT header arithmetic of
zlib.ts_amd/csrc/dict_host.h) built with ASan + UBSan as a stand-alone
program and run on the CPU, and the ABI of include/zt_dict.h."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ missing")
def test_dict_host_check_sanitized(tmp_path):
    exe = str(tmp_path / "dict_host_check")
    b = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tools", "dict_host_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("dict_host_check ok")


def test_header_declares_what_the_binding_binds():
    """every function include/zt_dict.h declares is in the Python binding's
    list, and the other way round (the library itself is checked on the GPU
    box: tests/test_gpu_dict.py calls each of them)"""
    src = open(os.path.join(ROOT, "include", "zt_dict.h")).read()
    declared = set(re.findall(r"^int (zt_\w+)\(", src, flags=re.M))
    py = open(os.path.join(ROOT, "zlib.ts_amd", "py", "ztamd.py")).read()
    m = re.search(r"DICT_SYMBOLS = \[(.*?)\]", py, flags=re.S)
    bound = set(re.findall(r'"(zt_\w+)"', m.group(1)))
    assert declared == bound and len(declared) == 7
    assert "#define ZT_E_ZLIB_DICTID -44" in src
