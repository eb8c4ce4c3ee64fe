"""Host-only checks of the checkpoint index: tools/ckpt_host_check.cpp (the
blob's validation and the range planner of zlib.ts_amd/csrc/ckpt_host.h)
built with ASan + UBSan as a stand-alone program and run on the CPU, and the
ABI of include/zt_checkpoint.h."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ missing")
def test_ckpt_host_check_sanitized(tmp_path):
    exe = str(tmp_path / "ckpt_host_check")
    b = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tools", "ckpt_host_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("ckpt_host_check ok")


def test_header_declares_what_the_binding_binds():
    """every function include/zt_checkpoint.h declares is in the Python
    binding's list, and the other way round (the library itself is checked on
    the GPU box: tests/test_gpu_ckpt.py calls each of them); the sync-point
    index's header and list keep their four"""
    src = open(os.path.join(ROOT, "include", "zt_checkpoint.h")).read()
    declared = set(re.findall(r"^int (zt_\w+)\(", src, flags=re.M))
    py = open(os.path.join(ROOT, "zlib.ts_amd", "py", "ztamd.py")).read()
    m = re.search(r"CKPT_SYMBOLS = \[(.*?)\]", py, flags=re.S)
    bound = set(re.findall(r'"(zt_\w+)"', m.group(1)))
    assert declared == bound and len(declared) == 4
    assert declared == {"zt_inflate_ckpt_build", "zt_inflate_ckpt_range", "zt_inflate_ckpt_ranges",
                        "zt_ckpt_stats_read"}
    # no new error codes: the header reuses zt_index.h's
    assert not re.findall(r"#define ZT_E_", src)
    assert '#include "zt_index.h"' in src


def test_library_exports_the_checkpoint_calls():
    import ctypes

    import ztamd

    lib = ctypes.CDLL(ztamd.LIBPATH)
    assert not [n for n in ztamd.CKPT_SYMBOLS if not hasattr(lib, n)]


def test_blob_layout_constants_agree():
    """the layout the header documents is the one the host code and the
    Python parser use"""
    hdr = open(os.path.join(ROOT, "include", "zt_checkpoint.h")).read()
    py = open(os.path.join(ROOT, "zlib.ts_amd", "py", "ztamd.py")).read()
    host = open(os.path.join(ROOT, "zlib.ts_amd", "csrc", "ckpt_host.h")).read()
    assert "#define ZT_CKPT_HEADER_BYTES 64" in hdr and "CKPT_HEADER_BYTES = 64" in py
    assert "#define ZT_CKPT_ENTRY_BYTES 48" in hdr and "CKPT_ENTRY_BYTES = 48" in py
    assert "#define ZT_CKPT_WINDOW_BYTES 32768" in hdr and "CKPT_WINDOW_BYTES = 32768" in py
    assert "#define ZT_CKPT_WINDOW_RECORD_BYTES 32784" in hdr and "CKPT_WINDOW_RECORD_BYTES = 32784" in py
    assert "#define ZT_CKPT_FIXED_HDR 0x4000000000000000ull" in hdr and "CKPT_FIXED_HDR = 1 << 62" in py
    assert '"ZTCK"' in hdr and '"ZTCK"' in host and 'b"ZTCK"' in py
    assert "#define ZT_CKPT_SPAN_MIN 65536" in hdr and "#define ZT_CKPT_SPAN_DEFAULT 1048576" in hdr


def test_python_parser_reads_the_documented_layout():
    """ckpt_entries on a hand-packed blob: one unit, the sentinel, no window"""
    import struct

    import ztamd

    head = b"ZTCK" + struct.pack("<III", 1, 1, 0) + struct.pack("<QQQQ", 10, 30, 77, 1 << 20) + bytes(16)
    e0 = struct.pack("<QQQIIIIII", 80, 0, 0, 0, 0, 0, 40, 0, 0)
    e1 = struct.pack("<QQQIIIIII", 237, 0, 77, 4, 0, 0, 0, 0, 0)
    h, ent, wins = ztamd.ckpt_entries(head + e0 + e1)
    assert h == {"version": 1, "nunits": 1, "nwin": 0, "stream_start": 10, "end_ip": 30, "total_out": 77,
                 "span": 1 << 20}
    assert len(ent) == 2 and int(ent["pos"][1]) == 237 and int(ent["kind"][1]) == ztamd.CKPT_KINDS["final"]
    assert int(ent["ntok"][0]) == 40 and wins == []
    with pytest.raises(ValueError):
        ztamd.ckpt_entries(b"ZTIX" + head[4:] + e0 + e1)
    with pytest.raises(ValueError):
        ztamd.ckpt_entries(head + e0)
