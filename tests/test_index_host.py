"""Host-only checks of the indexed range inflate: tools/index_host_check.cpp
(the index blob's validation and the range planner of
zlib.ts_amd/csrc/index_host.h) built with ASan + UBSan as a stand-alone
program and run on the CPU, and the ABI of include/zt_index.h."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ missing")
def test_index_host_check_sanitized(tmp_path):
    exe = str(tmp_path / "index_host_check")
    b = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tools", "index_host_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("index_host_check ok")


def test_header_declares_what_the_binding_binds():
    """every function include/zt_index.h declares is in the Python binding's
    list, and the other way round (the library itself is checked on the GPU
    box: tests/test_gpu_index.py calls each of them)"""
    src = open(os.path.join(ROOT, "include", "zt_index.h")).read()
    declared = set(re.findall(r"^int (zt_\w+)\(", src, flags=re.M))
    py = open(os.path.join(ROOT, "zlib.ts_amd", "py", "ztamd.py")).read()
    m = re.search(r"INDEX_SYMBOLS = \[(.*?)\]", py, flags=re.S)
    bound = set(re.findall(r'"(zt_\w+)"', m.group(1)))
    assert declared == bound and len(declared) == 4
    assert "#define ZT_E_NO_INDEX -60" in src
    assert "#define ZT_E_INDEX -61" in src
    assert "#define ZT_E_INDEX_MISMATCH -62" in src


def test_blob_layout_constants_agree():
    """the layout the header documents is the one the host code and the
    Python parser use"""
    hdr = open(os.path.join(ROOT, "include", "zt_index.h")).read()
    py = open(os.path.join(ROOT, "zlib.ts_amd", "py", "ztamd.py")).read()
    assert "#define ZT_INDEX_HEADER_BYTES 64" in hdr and "INDEX_HEADER_BYTES = 64" in py
    assert "#define ZT_INDEX_ENTRY_BYTES 24" in hdr and "INDEX_ENTRY_BYTES = 24" in py
