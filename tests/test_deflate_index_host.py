"""Host-only checks of the deflate-time index: tools/deflate_index_host_check.cpp
(the entry count, the entry layout of a pieced stream and the header fill of
zlib.ts_amd/csrc/deflate_index_host.h, against a serial restatement and
index_validate) built with ASan + UBSan as a stand-alone program and run on
the CPU, and the ABI of the write side of include/zt_index.h."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRITERS = ["zt_deflate_raw_indexed", "zt_gzip_compress_indexed", "zt_zlib_compress_indexed"]
ZT_E_NO_DEVICE, ZT_E_NO_INDEX = -100, -60


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ missing")
def test_deflate_index_host_check_sanitized(tmp_path):
    exe = str(tmp_path / "deflate_index_host_check")
    b = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tools", "deflate_index_host_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("deflate_index_host_check ok")


def test_header_declares_the_writers_the_binding_binds():
    src = open(os.path.join(ROOT, "include", "zt_index.h")).read()
    declared = re.findall(r"^ZT_INDEX_WRITER int (zt_\w+)\(", src, flags=re.M)
    py = open(os.path.join(ROOT, "zlib.ts_amd", "py", "ztamd.py")).read()
    m = re.search(r"DEFLATE_INDEX_SYMBOLS = \[(.*?)\]", py, flags=re.S)
    bound = re.findall(r'"(zt_\w+)"', m.group(1))
    assert sorted(declared) == sorted(bound) == sorted(WRITERS)
    # the blob format is the read side's, unchanged
    assert "#define ZT_INDEX_VERSION 1" in src


def test_writers_exist_and_need_a_device():
    """the three symbols are in libzt.so; without a GPU each returns
    ZT_E_NO_DEVICE (never a CPU fallback), and a stored-only request is
    refused before the device is looked for"""
    import ztamd

    lib = ztamd.lib
    for name in WRITERS:
        assert getattr(lib, name, None) is not None, name
    opts = ztamd.DeflateOpts(0, 0, -1)  # compression_type NONE
    d, n = ztamd._cbuf(b"abc" * 100)
    out, idx = ctypes.POINTER(ctypes.c_uint8)(), ctypes.POINTER(ctypes.c_uint8)()
    olen, ilen = ctypes.c_size_t(), ctypes.c_size_t()
    rc = lib.zt_deflate_raw_indexed(d, n, ctypes.byref(opts), 0, ctypes.byref(out), ctypes.byref(olen),
                                    ctypes.byref(idx), ctypes.byref(ilen))
    assert rc == ZT_E_NO_INDEX and not out and not idx
    rc = lib.zt_zlib_compress_indexed(d, n, ctypes.byref(opts), ctypes.byref(out), ctypes.byref(olen), None,
                                      ctypes.byref(idx), ctypes.byref(ilen))
    assert rc == ZT_E_NO_INDEX and not out and not idx
    if ztamd.device_count() > 0:
        return
    rc = lib.zt_deflate_raw_indexed(d, n, None, 0, ctypes.byref(out), ctypes.byref(olen), ctypes.byref(idx),
                                    ctypes.byref(ilen))
    assert rc == ZT_E_NO_DEVICE and not out and not idx
    rc = lib.zt_gzip_compress_indexed(d, n, None, ctypes.byref(out), ctypes.byref(olen), None, ctypes.byref(idx),
                                      ctypes.byref(ilen))
    assert rc == ZT_E_NO_DEVICE and not out and not idx
    rc = lib.zt_zlib_compress_indexed(d, n, None, ctypes.byref(out), ctypes.byref(olen), None, ctypes.byref(idx),
                                      ctypes.byref(ilen))
    assert rc == ZT_E_NO_DEVICE and not out and not idx
