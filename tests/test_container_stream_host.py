"""Host-only checks of the container sessions
(include/zt_stream_container.h): tools/container_stream_check.cpp (the
incremental gzip header test at every split of headers with every flag
combination against gzip_parse_header on the whole header, the AUTO decision,
ISIZE modulo 2^32, and the framing state machine of
zlib.ts_amd/csrc/container_stream_host.h driven over files cut at every
position) built with ASan + UBSan as a stand-alone program and run on the
CPU; the ABI of the header; and the calls' answer without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ZT_E_NO_DEVICE = -100


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ missing")
def test_container_stream_check_sanitized(tmp_path):
    exe = str(tmp_path / "container_stream_check")
    b = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-pthread", "-o", exe, os.path.join(ROOT, "tools", "container_stream_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("container_stream_check ok")


def _struct_fields(src, name):
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} %s;" % name, src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in re.findall(r"^\s*(?:const\s+)?(?:u?int\d+_t|size_t)\s+([^;]+);", body, flags=re.M):
        names += [n.strip().lstrip("*") for n in decl.split(",")]
    return names


def test_header_declares_what_the_binding_binds():
    """every function include/zt_stream_container.h declares is in the Python
    binding's list and exported by libzt.so, and the other way round; the list
    shares nothing with zt.h's or zt_stream.h's"""
    import ztamd

    src = open(os.path.join(ROOT, "include", "zt_stream_container.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^(?:int|void|const char \*) ?(zt_\w+)\(", code, flags=re.M))
    assert declared == set(ztamd.CONTAINER_STREAM_SYMBOLS) and len(declared) == 7
    lib = ctypes.CDLL(ztamd.LIBPATH)
    assert not [n for n in declared if not hasattr(lib, n)]
    assert not set(ztamd.CONTAINER_STREAM_SYMBOLS) & (set(ztamd.SYMBOLS) | set(ztamd.STREAM_SYMBOLS))
    # zt_stream.h keeps its six
    stream = open(os.path.join(ROOT, "include", "zt_stream.h")).read()
    assert not re.findall(r"zt_container_\w+", stream)
    # the records of the binding are the header's
    assert _struct_fields(src, "zt_container_session_info") == [k for k, _ in ztamd.ContainerSessionInfo._fields_]
    assert ctypes.sizeof(ztamd.ContainerSessionInfo) == 80
    assert _struct_fields(src, "zt_container_member") == [k for k, _ in ztamd.ContainerMember._fields_]
    assert ctypes.sizeof(ztamd.ContainerMember) == 96
    formats = dict(re.findall(r"#define (ZT_SESSION_\w+) (\d+)", src))
    assert formats == {"ZT_SESSION_GZIP": str(ztamd.SESSION_GZIP), "ZT_SESSION_ZLIB": str(ztamd.SESSION_ZLIB),
                       "ZT_SESSION_AUTO": str(ztamd.SESSION_AUTO)}


def test_makefile_lists_the_header():
    mk = open(os.path.join(ROOT, "zlib.ts_amd", "Makefile")).read()
    assert mk.count("../include/zt_stream_container.h") == mk.count("../include/zt_stream.h ") == 2


def test_calls_without_a_device():
    """without a GPU create and feed return ZT_E_NO_DEVICE (count 0: ZT_OK, no device asked for)"""
    import ztamd

    assert ztamd.lib.zt_container_sessions_feed(None, None, None, None, 0, None, None, None) == 0
    import torch

    if torch.cuda.is_available():
        return  # tests/test_gpu_container_session.py runs the calls
    assert ztamd.device_count() == 0
    for cls in (ztamd.GunzipSession, ztamd.ZlibInflateSession):
        with pytest.raises(ztamd.ZtError) as e:
            cls()
        assert e.value.code == ZT_E_NO_DEVICE
    h = ctypes.c_void_p()
    assert ztamd.lib.zt_container_session_create(ztamd.SESSION_ZLIB, b"abc", 3, 1,
                                                 ctypes.byref(h)) == ZT_E_NO_DEVICE and not h
    out, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
    assert ztamd.lib.zt_container_session_feed(None, b"\x1f\x8b", 2, 1, ctypes.byref(out),
                                               ctypes.byref(n)) == ZT_E_NO_DEVICE
    one = (ctypes.c_void_p * 1)(None)
    assert ztamd.lib.zt_container_sessions_feed(one, one, (ctypes.c_size_t * 1)(0), None, 1, ctypes.byref(out),
                                                ctypes.byref(n), (ctypes.c_int * 1)()) == ZT_E_NO_DEVICE
