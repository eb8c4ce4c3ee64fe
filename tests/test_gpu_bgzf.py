"""BGZF on the GPU (include/zt_bgzf.h): the writer against the plain-Python
parser tests/bgzf_py.py, Python's gzip and zt_deflate_raw_batch; the exact
reader on its own and on foreign (zlib-written) files; every error with its
block's offset and, for payload failures, zt_gunzip's code and message for
that block alone; byte ranges and virtual-offset chunks with the work counters
held against the blocks the ranges touch; bad .gzi blobs."""
import gzip
import hashlib
import json
import os
import struct
import subprocess
import sys
import zlib

import pytest

import bgzf_py

pytestmark = pytest.mark.gpu

ZT_E_ARG, ZT_E_BGZF_FORMAT, ZT_E_BGZF_INDEX = -103, -70, -71
SIZES = [0, 1, 4095, 4096, 65279, 65280, 65281, 130560, 130561, (200 << 10) + 37]


@pytest.fixture(scope="module")
def zt():
    import ztamd

    return ztamd


@pytest.fixture(scope="module")
def corpus(oracle):
    n = 4 * 65280 + 1000  # (the five-block range file; >= max(SIZES))
    return {"wordsalad": oracle.gen("wordsalad", 11, n), "xorshift32": oracle.gen("xorshift32", 12, n),
            "structured": oracle.gen("structured", 13, n), "zeros": bytes(n)}


def _slices(data, bs):
    return [data[p:p + bs] for p in range(0, len(data), bs)]


def _check_file(zt, f, data, bs, gzi=None, **opts):
    """the writer's contract for one file"""
    blocks = bgzf_py.walk(f)  # (raises where the BSIZE chain breaks)
    assert f.endswith(bgzf_py.EOF) and blocks[-1].size == 28 and blocks[-1].offset == len(f) - 28
    sl = _slices(data, bs)
    assert len(blocks) == len(sl) + 1
    raw = zt.deflate_raw_batch(sl, **opts) if sl else []
    for k, b in enumerate(blocks[:-1]):
        assert f[b.offset:b.offset + 16] == bgzf_py.HEADER
        assert b.size <= 65536 and b.isize == len(sl[k]) and b.crc == zlib.crc32(sl[k]), k
        assert b.cdata == raw[k], k
    assert gzip.decompress(f) == data
    if gzi is not None:
        assert gzi == zt.bgzf_index(f) == bgzf_py.gzi(f)
        assert gzi == bgzf_py.gzi_blob([(b.offset, k * bs) for k, b in enumerate(blocks[:-1]) if k])


@pytest.mark.parametrize("kind", ["wordsalad", "xorshift32", "structured", "zeros"])
def test_write_and_read_back(zt, corpus, kind):
    for n in SIZES:
        data = corpus[kind][:n]
        f, gzi = zt.bgzf_compress(data, want_index=True)
        assert f == zt.bgzf_compress(data)
        _check_file(zt, f, data, 65280, gzi)
        out, info = zt.bgzf_decompress(f, return_info=True)
        nb = (n + 65279) // 65280
        assert out == data, n
        assert info == {"blocks": nb + 1, "data_blocks": nb, "total_out": n, "error_offset": 0, "has_eof": 1}, n


def test_empty_input_is_the_marker(zt):
    f, gzi = zt.bgzf_compress(b"", want_index=True)
    assert f == bgzf_py.EOF and gzi == struct.pack("<Q", 0)
    assert zt.bgzf_decompress(b"", return_info=True) == (
        b"", {"blocks": 0, "data_blocks": 0, "total_out": 0, "error_offset": 0, "has_eof": 0})


def test_block_size_option(zt, corpus):
    data = corpus["wordsalad"][:20481]
    f, gzi = zt.bgzf_compress(data, block_size=4096, want_index=True)
    assert len(bgzf_py.walk(f)) == 6 + 1
    _check_file(zt, f, data, 4096, gzi)
    assert zt.bgzf_decompress(f) == data
    # a block size that is no multiple of 16: the reader packs the blocks on the device
    f = zt.bgzf_compress(data, block_size=5001)
    _check_file(zt, f, data, 5001)
    assert zt.bgzf_decompress(f) == data
    for bad in (4095, 65281):
        with pytest.raises(zt.ZtError) as e:
            zt.bgzf_compress(data, block_size=bad)
        assert e.value.code == ZT_E_ARG


@pytest.mark.parametrize("opts", [{"compression_type": 0}, {"compression_type": 1}, {"level": 1}, {"level": 9}])
def test_compression_options(zt, corpus, opts):
    data = corpus["wordsalad"][:150001]
    f, gzi = zt.bgzf_compress(data, want_index=True, **opts)
    _check_file(zt, f, data, 65280, gzi, **opts)
    assert zt.bgzf_decompress(f) == data


def test_grouping_does_not_change_a_byte(zt, corpus):
    """ZT_BGZF_GROUP_BLOCKS=3 on 13-block inputs (5 groups through the stage
    pipeline): the files are the one-group files.  The hook is read once per
    process: tests/bgzf_group_child.py runs with it set."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, ZT_BGZF_GROUP_BLOCKS="3")
    p = subprocess.run([sys.executable, os.path.join(here, "bgzf_group_child.py")], env=env, capture_output=True,
                       text=True, timeout=100)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    import bgzf_group_child

    want = {}
    for name, (data, bs) in bgzf_group_child.inputs().items():
        f, gzi = zt.bgzf_compress(data, block_size=bs, want_index=True)
        assert len(bgzf_py.walk(f)) == 13 + 1
        want[name] = [hashlib.sha256(f).hexdigest(), hashlib.sha256(gzi).hexdigest()]
    assert res == want


# ---- foreign files -------------------------------------------------------------------
def _foreign(corpus):
    d = corpus["wordsalad"][:150000]
    big = corpus["wordsalad"][:65536]
    return {
        "level 1": (bgzf_py.write(d, level=1), d),
        "level 6": (bgzf_py.write(d, level=6), d),
        "level 9": (bgzf_py.write(d, level=9), d),
        "stored": (bgzf_py.write(d, level=0, block_size=65000), d),
        "fixed codes": (bgzf_py.write(d, strategy=zlib.Z_FIXED, block_size=30000), d),
        "ISIZE 65536": (bgzf_py.block(big) + bgzf_py.block(d[:777]) + bgzf_py.EOF, big + d[:777]),
        "empty block inside": (bgzf_py.block(d[:5000]) + bgzf_py.block(b"") + bgzf_py.block(d[5000:9000]) + bgzf_py.EOF,
                               d[:9000]),
        "two files": (bgzf_py.write(d[:70000]) + bgzf_py.write(d[70000:]), d),
        "no marker": (bgzf_py.write(d, eof=False), d),
        "foreign subfield": (bgzf_py.write(d[:20000], block_size=4099, extra_subfields=b"ZT\x02\x00\x07\x07"),
                             d[:20000]),
        "random bytes": (bgzf_py.write(corpus["xorshift32"][:70001]), corpus["xorshift32"][:70001]),
    }


def test_reads_foreign_files(zt, corpus):
    for name, (f, data) in _foreign(corpus).items():
        out, info = zt.bgzf_decompress(f, return_info=True)
        blocks = bgzf_py.walk(f)
        assert out == data, name
        assert info["blocks"] == len(blocks) and info["total_out"] == len(data), name
        assert info["data_blocks"] == sum(1 for b in blocks if b.isize), name
        assert info["has_eof"] == int(name != "no marker"), name
        # and by ranges, with the helper's index and without one
        total = len(data)
        rs = [(0, total), (total - 1, 1), (total // 3, total // 2)]
        for gzi in (bgzf_py.gzi(f), None):
            for (off, ln), (st, got) in zip(rs, zt.bgzf_read_ranges(f, rs, gzi=gzi)):
                assert st == 0 and got == data[off:off + ln], (name, off, ln)


# ---- errors -----------------------------------------------------------------------------
def _patched(f, off, patch):
    b = bytearray(f)
    b[off:off + len(patch)] = patch
    return bytes(b)


def _gunzip_error(zt, block_bytes):
    with pytest.raises(zt.ZtError) as e:
        zt.gunzip(block_bytes)
    return e.value.code, e.value.msg


@pytest.fixture(scope="module")
def err_file(zt, corpus):
    data = corpus["wordsalad"][:40000]
    f = zt.bgzf_compress(data, block_size=8192)
    return f, data, bgzf_py.walk(f)


def test_format_errors(zt, err_file):
    f, data, blocks = err_file
    b1 = blocks[1]
    tiny = bgzf_py.block(b"")
    cases = {
        "truncated inside the second block": f[:b1.offset + b1.size - 5],
        "wrong magic": _patched(f, b1.offset, b"\x1f\x8c"),
        "BSIZE smaller than the header": _patched(f, b1.offset + 16, struct.pack("<H", 20)),
        "no BC subfield": f[:b1.offset] + zt.gzip_compress(data[:500])[0],
        "FLG 0x0C": _patched(f, b1.offset + 3, b"\x0c"),
        "ISIZE 65537": _patched(f, b1.offset + b1.size - 4, struct.pack("<I", 65537)),
        "ISIZE above 1032 x CDATA": f[:b1.offset] + tiny[:-4] + struct.pack("<I", 2065),
    }
    before = zt.bgzf_stats()
    for name, bad in cases.items():
        with pytest.raises(zt.ZtError) as e:
            zt.bgzf_decompress(bad)
        assert e.value.code == ZT_E_BGZF_FORMAT, name
        assert e.value.info["error_offset"] == b1.offset, name
        assert e.value.msg.startswith(f"not a BGZF block at offset {b1.offset}: "), (name, e.value.msg)
        with pytest.raises(zt.ZtError) as e:  # the range call walks the same chain
            zt.bgzf_read_ranges(bad, [(0, 10)])
        assert e.value.code == ZT_E_BGZF_FORMAT, name
    assert zt.bgzf_stats() == before


def test_payload_errors(zt, err_file):
    f, data, blocks = err_file
    b1, b3 = blocks[1], blocks[3]
    cd = b1.offset + 18
    cases = {
        "a CDATA byte flipped": (_patched(f, cd + 40, bytes([f[cd + 40] ^ 0x10])), b1),
        "the first CDATA byte flipped": (_patched(f, cd, bytes([f[cd] ^ 0x06])), b1),
        "the CRC field flipped": (_patched(f, b1.offset + b1.size - 8, bytes([f[b1.offset + b1.size - 8] ^ 1])), b1),
        "ISIZE off by one": (_patched(f, b1.offset + b1.size - 4, struct.pack("<I", b1.isize + 1)), b1),
        "ISIZE one short": (_patched(f, b1.offset + b1.size - 4, struct.pack("<I", b1.isize - 1)), b1),
        "two bad blocks": (_patched(_patched(f, b3.offset + 18 + 9, bytes([f[b3.offset + 18 + 9] ^ 0xFF])),
                                    b1.offset + b1.size - 8, bytes([f[b1.offset + b1.size - 8] ^ 1])), b1),
    }
    for name, (bad, blk) in cases.items():
        want = _gunzip_error(zt, bad[blk.offset:blk.offset + blk.size])
        with pytest.raises(zt.ZtError) as e:
            zt.bgzf_decompress(bad)
        assert (e.value.code, e.value.msg) == want, name
        assert e.value.info["error_offset"] == blk.offset, name
    assert _gunzip_error(zt, cases["the CRC field flipped"][0][b1.offset:b1.offset + b1.size])[0] == -33
    assert _gunzip_error(zt, cases["ISIZE off by one"][0][b1.offset:b1.offset + b1.size])[0] == -34


# ---- ranges ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def range_files(zt, corpus):
    a = corpus["structured"][:12 * 4096 - 123]
    b = corpus["wordsalad"][:4 * 65280 + 1000]
    fa, ga = zt.bgzf_compress(a, block_size=4096, want_index=True)
    fb, gb = zt.bgzf_compress(b, want_index=True)
    assert len(bgzf_py.walk(fa)) == 13 and len(bgzf_py.walk(fb)) == 6
    return {"12 x 4096": (fa, ga, a, 4096), "5 x 65280": (fb, gb, b, 65280)}


def _range_cases(total, bs):
    return {
        "first byte": [(0, 1)],
        "across a block boundary": [(bs - 3, 7)],
        "whole file": [(0, total)],
        "last byte": [(total - 1, 1)],
        "off == total": [(total, 5)],
        "off > total": [(total + 1, 5)],
        "clamped": [(total - 10, 1000), (0, 1 << 62)],
        "unsorted, overlapping, repeated": [(3 * bs + 5, 100), (10, bs), (bs - 1, 2), (10, bs), (2 * bs, bs + 1),
                                            (total, 0), (0, 0), (total + 9, 1)],
    }


@pytest.mark.parametrize("which", ["12 x 4096", "5 x 65280"])
@pytest.mark.parametrize("indexed", [True, False])
def test_ranges(zt, range_files, which, indexed):
    f, gzi, data, bs = range_files[which]
    total = len(data)
    for name, rs in _range_cases(total, bs).items():
        before = zt.bgzf_stats()
        rc, res = zt.bgzf_read_ranges(f, rs, gzi=gzi if indexed else None, return_code=True)
        after = zt.bgzf_stats()
        returned = 0
        for (off, ln), (st, got) in zip(rs, res):
            if off > total:
                assert st == ZT_E_ARG and got is None, name
            else:
                assert st == 0 and got == data[off:off + ln], (name, off, ln)
                returned += len(got)
        assert rc == (ZT_E_ARG if any(off > total for off, _ in rs) else 0), name
        nblocks, nbytes = bgzf_py.touched(f, rs)
        assert after["blocks_decoded"] - before["blocks_decoded"] == nblocks, name
        assert after["in_bytes_uploaded"] - before["in_bytes_uploaded"] == nbytes, name
        assert after["ranges"] - before["ranges"] == len(rs), name
        assert after["range_calls"] - before["range_calls"] == (1 if nblocks else 0), name
        assert after["out_bytes_returned"] - before["out_bytes_returned"] == returned, name
    # (the whole file is 13 / 6 blocks: a reader that decodes all of it fails the counts above)
    assert bgzf_py.touched(f, [(0, 1)])[0] == 1 and bgzf_py.touched(f, [(bs - 3, 7)])[0] == 2


def test_virtual_offsets(zt, range_files):
    f, gzi, data, bs = range_files["12 x 4096"]
    blocks = bgzf_py.walk(f)
    v = bgzf_py.voffset
    assert zt.bgzf_voffset(blocks[2].offset, 9) == v(blocks[2].offset, 9)
    chunks = [
        (v(blocks[2].offset, 10), v(blocks[2].offset, 1000)),      # inside one block
        (v(blocks[4].offset, 4000), v(blocks[6].offset, 17)),      # across three blocks
        (v(blocks[7].offset, 33), v(blocks[7].offset, 33)),        # beg == end
        (v(blocks[0].offset, 0), v(blocks[12].offset, 0)),         # everything, up to the marker
        (v(blocks[11].offset, 5), v(len(f), 0)),                   # up to the end of the file
        (v(blocks[3].offset + 7, 0), v(blocks[5].offset, 1)),      # a coffset in the middle of a block
        (v(blocks[3].offset, 0), v(blocks[5].offset - 1, 1)),
        (v(blocks[3].offset, 4097), v(blocks[5].offset, 1)),       # uoffset above ISIZE
        (v(blocks[3].offset, 5), v(blocks[3].offset, 4)),          # end < beg
        (v(blocks[4].offset, 4000), v(blocks[6].offset, 17)),      # repeated
    ]
    want = [data[2 * bs + 10:2 * bs + 1000], data[4 * bs + 4000:6 * bs + 17], b"", data, data[11 * bs + 5:],
            ZT_E_BGZF_FORMAT, ZT_E_BGZF_FORMAT, ZT_E_ARG, ZT_E_ARG, data[4 * bs + 4000:6 * bs + 17]]
    before = zt.bgzf_stats()
    rc, res = zt.bgzf_read_virtual(f, chunks, return_code=True)
    after = zt.bgzf_stats()
    for w, (st, got) in zip(want, res):
        if isinstance(w, int):
            assert st == w and got is None
        else:
            assert st == 0 and got == w
    assert rc == ZT_E_BGZF_FORMAT
    assert res[5][0].message.startswith("not a BGZF block at offset")
    assert after["blocks_decoded"] - before["blocks_decoded"] == 12  # every data block, once
    # empty chunks alone never reach the device
    before = zt.bgzf_stats()
    assert zt.bgzf_read_virtual(f, [chunks[2], (v(len(f), 0), v(len(f), 0))]) == [(0, b""), (0, b"")]
    after = zt.bgzf_stats()
    assert after["range_calls"] == before["range_calls"] and after["blocks_decoded"] == before["blocks_decoded"]
    # three blocks of the default size
    f, gzi, data, bs = range_files["5 x 65280"]
    blocks = bgzf_py.walk(f)
    (st, got), = zt.bgzf_read_virtual(f, [(v(blocks[1].offset, 65000), v(blocks[3].offset, 123))])
    assert st == 0 and got == data[bs + 65000:3 * bs + 123]


def test_bad_gzi_is_rejected_on_the_host(zt, range_files):
    f, gzi, data, bs = range_files["12 x 4096"]
    pairs = bgzf_py.gzi_pairs(f)
    swapped = list(pairs)
    swapped[3], swapped[4] = swapped[4], swapped[3]
    past = pairs[:-1] + [(len(f) - 10, pairs[-1][1])]
    off_by_one = pairs[:5] + [(pairs[5][0], pairs[5][1] + 1)] + pairs[6:]
    not_a_block = pairs[:5] + [(pairs[5][0] + 1, pairs[5][1])] + pairs[6:]
    cases = {"wrong length": gzi[:-1], "count disagrees": struct.pack("<Q", 3) + gzi[8:],
             "swapped pairs": bgzf_py.gzi_blob(swapped), "offset past the file": bgzf_py.gzi_blob(past),
             "uncompressed offset off by one": bgzf_py.gzi_blob(off_by_one),
             "pair off a block start": bgzf_py.gzi_blob(not_a_block)}
    before = zt.bgzf_stats()
    for name, bad in cases.items():
        with pytest.raises(zt.ZtError) as e:
            zt.bgzf_read_ranges(f, [(0, len(data)), (5 * bs + 7, 100)], gzi=bad)
        assert e.value.code == ZT_E_BGZF_INDEX, name
    assert zt.bgzf_stats() == before
    # a sparse index, and one with a pair on the marker, are fine
    sparse = bgzf_py.gzi_blob(pairs[4:5] + [(len(f) - 28, len(data))])
    assert zt.bgzf_read_ranges(f, [(6 * bs - 2, 9)], gzi=sparse) == [(0, data[6 * bs - 2:6 * bs + 7])]


def test_bad_block_fails_only_the_ranges_that_touch_it(zt, range_files):
    f, gzi, data, bs = range_files["12 x 4096"]
    b5 = bgzf_py.walk(f)[5]
    bad = _patched(f, b5.offset + b5.size - 8, bytes([f[b5.offset + b5.size - 8] ^ 0x80]))
    code, msg = _gunzip_error(zt, bad[b5.offset:b5.offset + b5.size])
    assert code == -33
    rs = [(0, 5 * bs), (5 * bs, 1), (6 * bs, 100), (4 * bs + 1, 3 * bs), (11 * bs, 50)]
    for g in (gzi, None):
        rc, res = zt.bgzf_read_ranges(bad, rs, gzi=g, return_code=True)
        assert rc == code
        for (off, ln), (st, got) in zip(rs, res):
            if off < 6 * bs and off + ln > 5 * bs:
                assert st == code and got is None
            else:
                assert st == 0 and got == data[off:off + ln]
        assert res[1][0].message == msg
    with pytest.raises(zt.ZtError) as e:
        zt.bgzf_decompress(bad)
    assert (e.value.code, e.value.msg) == (code, msg) and e.value.info["error_offset"] == b5.offset
