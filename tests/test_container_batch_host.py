"""Host-only checks of the container batch calls: tools/gunzip_chain_check.cpp
(the gzip header / trailer checks, the candidate bounds and the chain walk of
zlib.ts_amd/csrc/gunzip_chain.h over hand-made candidate and decode tables)
built with ASan + UBSan as a stand-alone program and run on the CPU, the same
for tools/inflate_chain_check.cpp (the segment and batch chains of
zlib.ts_amd/csrc/inflate_chain.h) and for tools/batch_plan_check.cpp (the host
batch layer's arithmetic and fan-out, zlib.ts_amd/csrc/batch_plan.h), and the
ABI of include/zt_container_batch.h."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ missing")
def test_gunzip_chain_check_sanitized(tmp_path):
    exe = str(tmp_path / "gunzip_chain_check")
    b = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tools", "gunzip_chain_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("gunzip_chain_check ok")


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ missing")
def test_inflate_chain_check_sanitized(tmp_path):
    """tools/inflate_chain_check.cpp: the host chain logic of the two-phase
    inflate (zlib.ts_amd/csrc/inflate_chain.h) over hand-made unit tables"""
    exe = str(tmp_path / "inflate_chain_check")
    b = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tools", "inflate_chain_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("inflate_chain_check ok")


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ missing")
def test_batch_plan_check_sanitized(tmp_path):
    """tools/batch_plan_check.cpp: the host batch layer's arithmetic
    (zlib.ts_amd/csrc/batch_plan.h: device splits, staging layout, upload
    chunks, pipeline groups, output bounds, the option resolver) against slow
    re-statements, and the fan-out's collection of each share's code and
    message for 1 and 3 stub shares"""
    exe = str(tmp_path / "batch_plan_check")
    b = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tools", "batch_plan_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("batch_plan_check ok")


def test_header_declares_what_the_binding_binds():
    """every function include/zt_container_batch.h declares is in the Python
    binding's list, and the other way round, and libzt.so exports each (the
    calls themselves are checked on the GPU: tests/test_gpu_container_batch.py)"""
    import ztamd

    src = open(os.path.join(ROOT, "include", "zt_container_batch.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(zt_[a-z0-9_]+)\s*\(", src))
    assert declared == set(ztamd.CONTAINER_BATCH_SYMBOLS)
    assert {"zt_gunzip_batch", "zt_zlib_decompress_batch", "zt_zlib_decompress_batch_dict",
            "zt_gunzip_batch_last_stats"} <= declared
    lib = ctypes.CDLL(ztamd.LIBPATH)
    assert not [n for n in declared if not hasattr(lib, n)]
    assert '#include "zt_dict.h"' in src
