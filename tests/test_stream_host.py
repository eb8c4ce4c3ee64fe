"""Host-only checks of the inflate sessions (include/zt_stream.h):
tools/stream_host_check.cpp (the pending-tail bookkeeping for every end_bits
around a feed boundary, the decode limit, the pack offsets, the output slots
and the relaunch plan after an output-full stop, the trailing-byte count, the
checksum combination and the duplicate-session check of
zlib.ts_amd/csrc/stream_host.h, against slow restatements) built with ASan +
UBSan as a stand-alone program and run on the CPU; the ABI of the header; and
the calls' answer without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ZT_E_NO_DEVICE = -100


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ missing")
def test_stream_host_check_sanitized(tmp_path):
    exe = str(tmp_path / "stream_host_check")
    b = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-pthread", "-o", exe, os.path.join(ROOT, "tools", "stream_host_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("stream_host_check ok")


def test_header_declares_what_the_binding_binds():
    """every function include/zt_stream.h declares is in the Python binding's
    list and exported by libzt.so, and the other way round; none of them is in
    zt.h's list"""
    import ztamd

    src = open(os.path.join(ROOT, "include", "zt_stream.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*) ?(zt_\w+)\(", src, flags=re.M))
    assert declared == set(ztamd.STREAM_SYMBOLS) and len(declared) == 6
    lib = ctypes.CDLL(ztamd.LIBPATH)
    assert not [n for n in declared if not hasattr(lib, n)]
    assert not set(ztamd.STREAM_SYMBOLS) & set(ztamd.SYMBOLS)
    # the info record of the binding is the header's
    fields = re.search(r"typedef struct \{(.*?)\} zt_inflate_session_info;", src, flags=re.S).group(1)
    names = [n for decl in re.findall(r"^\s*u?int\d+_t\s+([^;]+);", fields, flags=re.M)
             for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [k for k, _ in ztamd.InflateSessionInfo._fields_]
    assert ctypes.sizeof(ztamd.InflateSessionInfo) == 56


def test_calls_without_a_device():
    """without a GPU create and feed return ZT_E_NO_DEVICE (count 0: ZT_OK, no device asked for)"""
    import ztamd

    assert ztamd.lib.zt_inflate_sessions_feed(None, None, None, None, 0, None, None, None) == 0
    import torch

    if torch.cuda.is_available():
        return  # tests/test_gpu_stream_session.py runs the calls
    assert ztamd.device_count() == 0
    with pytest.raises(ztamd.ZtError) as e:
        ztamd.InflateSession()
    assert e.value.code == ZT_E_NO_DEVICE
    h = ctypes.c_void_p()
    assert ztamd.lib.zt_inflate_session_create(b"abc", 3, ctypes.byref(h)) == ZT_E_NO_DEVICE and not h
    out, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
    assert ztamd.lib.zt_inflate_session_feed(None, b"\x03\x00", 2, 1, ctypes.byref(out),
                                             ctypes.byref(n)) == ZT_E_NO_DEVICE
    one = (ctypes.c_void_p * 1)(None)
    assert ztamd.lib.zt_inflate_sessions_feed(one, one, (ctypes.c_size_t * 1)(0), None, 1, ctypes.byref(out),
                                              ctypes.byref(n), (ctypes.c_int * 1)()) == ZT_E_NO_DEVICE
