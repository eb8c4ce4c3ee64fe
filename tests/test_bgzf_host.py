"""Host-only checks of BGZF (include/zt_bgzf.h): tools/bgzf_host_check.cpp (the
header parse, the chain walk, the marker, the expansion bound, the .gzi blob,
virtual offsets, the range-to-blocks lookup and the dedup of
zlib.ts_amd/csrc/bgzf_host.h against slow restatements) built with ASan + UBSan
as a stand-alone program and run on the CPU; zt_bgzf_index -- a host walk that
touches no device -- on files from the plain-Python writer tests/bgzf_py.py;
and the ABI of the header."""
import ctypes
import os
import re
import shutil
import struct
import subprocess
import zlib

import pytest

import bgzf_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ZT_E_BGZF_FORMAT = -70


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ missing")
def test_bgzf_host_check_sanitized(tmp_path):
    exe = str(tmp_path / "bgzf_host_check")
    b = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tools", "bgzf_host_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("bgzf_host_check ok")


def _data(n, seed=1):
    # compressible, not periodic: words picked by an LCG
    words = [b"block", b"gzip", b"virtual", b"offset", b"index", b"chain", b"marker", b"range"]
    out, x = bytearray(), seed
    while len(out) < n:
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out += words[(x >> 16) & 7] + b" "
    return bytes(out[:n])


def test_helper_files_are_gzip():
    """the helper's files are what Python's gzip reads, marker included"""
    import gzip

    d = _data(150000)
    for f in (bgzf_py.write(d), bgzf_py.write(d, block_size=4096, level=1), bgzf_py.write(d, eof=False),
              bgzf_py.write(b"")):
        assert gzip.decompress(f) == (d if len(f) > 28 else b"")
    assert bgzf_py.write(b"") == bgzf_py.EOF and len(bgzf_py.EOF) == 28
    assert [b.isize for b in bgzf_py.walk(bgzf_py.write(d))] == [65280, 65280, 150000 - 2 * 65280, 0]


def test_index_pairs_and_info():
    """zt_bgzf_index without a GPU: pairs equal the helper's, info fields right"""
    import ztamd

    d = _data(200000, 3)
    cases = {
        "default": bgzf_py.write(d),
        "small blocks": bgzf_py.write(d[:30000], block_size=4096),
        "no marker": bgzf_py.write(d, eof=False),
        "two files": bgzf_py.write(d[:70000]) + bgzf_py.write(d[70000:]),
        "empty block inside": bgzf_py.block(d[:100]) + bgzf_py.block(b"") + bgzf_py.block(d[100:300]) + bgzf_py.EOF,
        "foreign subfield": bgzf_py.write(d[:9000], block_size=4096, extra_subfields=b"ZT\x02\x00\x07\x07"),
        "stored": bgzf_py.write(d[:70000], level=0),
        "marker alone": bgzf_py.EOF,
        "empty file": b"",
    }
    for name, f in cases.items():
        gzi, info = ztamd.bgzf_index(f, return_info=True)
        blocks = bgzf_py.walk(f)
        assert gzi == bgzf_py.gzi(f), name
        assert info["blocks"] == len(blocks), name
        assert info["data_blocks"] == sum(1 for b in blocks if b.isize), name
        assert info["total_out"] == sum(b.isize for b in blocks), name
        assert info["has_eof"] == int(f.endswith(bgzf_py.EOF)), name
    n, = struct.unpack_from("<Q", ztamd.bgzf_index(cases["default"]))
    assert n == 3  # four data blocks: a pair for every one after the first
    assert ztamd.bgzf_voffset(5, 7) == bgzf_py.voffset(5, 7) == (5 << 16) + 7


def _format_error(f):
    import ztamd

    with pytest.raises(ztamd.ZtError) as e:
        ztamd.bgzf_index(f)
    assert e.value.code == ZT_E_BGZF_FORMAT
    return e.value


def test_index_rejects_malformed_files():
    """each malformed file gives ZT_E_BGZF_FORMAT with the offending block's offset"""
    d = _data(20000, 5)
    f = bgzf_py.write(d, block_size=8192)
    second = bgzf_py.walk(f)[1].offset

    def at(off, patch):
        b = bytearray(f)
        b[off:off + len(patch)] = patch
        return bytes(b)

    import gzip

    cases = [
        ("truncated inside the second block", f[:second + 40]),
        ("truncated inside its header", f[:second + 7]),
        ("wrong magic", at(second, b"\x1f\x8c")),
        ("method", at(second + 2, b"\x09")),
        ("FLG 0x0C", at(second + 3, b"\x0c")),
        ("XLEN 4", at(second + 10, b"\x04\x00")),
        ("no BC subfield", at(second + 12, b"XC")),
        ("BSIZE smaller than the header", at(second + 16, struct.pack("<H", 20))),
        ("BSIZE past the file", at(second + 16, struct.pack("<H", 65535))),
        ("a plain gzip member", f[:second] + gzip.compress(d[:100])),
    ]
    b1 = bgzf_py.walk(f)[1]
    cases.append(("ISIZE 65537", at(second + b1.size - 4, struct.pack("<I", 65537))))
    tiny = bgzf_py.block(b"")  # 2 bytes of CDATA: at most 2064 bytes
    cases.append(("ISIZE above 1032 x CDATA", f[:second] + tiny[:-4] + struct.pack("<I", 2065)))
    for name, bad in cases:
        e = _format_error(bad)
        assert e.info["error_offset"] == second, name
        assert f"not a BGZF block at offset {second}: " in e.msg, (name, e.msg)
    # ISIZE exactly at both bounds passes the walk (the payload is not looked at here)
    import ztamd

    ok = f[:second] + tiny[:-4] + struct.pack("<I", 2064)
    assert ztamd.bgzf_index(ok, return_info=True)[1]["total_out"] == 8192 + 2064


def test_header_declares_what_the_binding_binds():
    """every function include/zt_bgzf.h declares is in the Python binding's
    list and exported by libzt.so, and the other way round"""
    import ztamd

    src = open(os.path.join(ROOT, "include", "zt_bgzf.h")).read()
    declared = set(re.findall(r"^int (zt_\w+)\(", src, flags=re.M))
    assert declared == set(ztamd.BGZF_SYMBOLS) and len(declared) == 6
    lib = ctypes.CDLL(ztamd.LIBPATH)
    assert not [n for n in declared if not hasattr(lib, n)]
    assert "#define ZT_E_BGZF_FORMAT -70" in src and "#define ZT_E_BGZF_INDEX  -71" in src
    assert "#define ZT_BGZF_BLOCK_MAX 65280" in src and ztamd.BGZF_BLOCK_MAX == 65280
    assert not set(ztamd.BGZF_SYMBOLS) & set(ztamd.SYMBOLS)
    # the structures' sizes are the header's (LP64)
    assert ctypes.sizeof(ztamd.BgzfOpts) == 16 and ctypes.sizeof(ztamd.BgzfInfo) == 40
    assert ctypes.sizeof(ztamd.BgzfStats) == 48
    assert zlib.crc32(b"") == 0
