"""The deflate-time index (include/zt_index.h, the write side):
zt_deflate_raw_indexed, zt_gzip_compress_indexed and zt_zlib_compress_indexed
return the index of the stream they write.  The definition of correct: the
stream is the plain writer's, and the blob is byte for byte what
zt_inflate_index_build returns for that stream, wherever that build
succeeds."""
import gzip
import zlib

import numpy as np
import pytest

import index_corpus
from index_corpus import MIB, TOTAL

pytestmark = pytest.mark.gpu

E_ARG, E_NO_INDEX = -103, -60
NO_INDEX_TEXT = "stream has no usable sync points"
VARIANTS = {"level6": dict(level=6), "level1": dict(level=1), "fixed": dict(compression_type=1)}


@pytest.fixture(scope="module")
def zt():
    import ztamd

    assert ztamd.device_count() > 0, "no GPU visible"
    return ztamd


@pytest.fixture(scope="module")
def data(oracle):
    return index_corpus.corpus(oracle)


def range_cases():
    """the range cases of tests/test_gpu_index.py"""
    cases = [(0, 1), (0, TOTAL), (TOTAL - 1, 1), (TOTAL, 0), (TOTAL, 5), (TOTAL - 3, 100)]
    for b in (32768, MIB, 2 * MIB):
        cases += [(b - 1, 2), (b, 1), (b - 1, 1)]
    cases.append((MIB - 70000, 140000))
    return cases


def describe(zt, blob):
    hdr, ent = zt.index_entries(blob)
    return hdr, [tuple(int(x) for x in e) for e in ent[:6]], len(ent)


def same_blob(zt, got, want):
    assert got == want, (describe(zt, got), describe(zt, want))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_identity_on_the_index_corpus(zt, data, variant):
    opts = VARIANTS[variant]
    s, blob = zt.deflate_raw_indexed(data, **opts)
    assert s == zt.deflate_raw(data, **opts)
    same_blob(zt, blob, zt.inflate_index_build(s))
    hdr, ent = zt.index_entries(blob)
    assert hdr["total_out"] == TOTAL and hdr["end_ip"] == len(s) and hdr["stream_start"] == 0
    # the double marker behind a stored block that ends a segment: two flagged
    # entries in a row at one output offset
    flags, out_off = ent["flags"][:-1] & 1, ent["out_off"][:-1]
    pairs = [k for k in range(len(flags) - 1) if flags[k] and flags[k + 1] and out_off[k] == out_off[k + 1]]
    assert pairs, "no pair of consecutive flagged entries at one output offset"
    for off, length in range_cases():
        assert zt.inflate_range(s, blob, off, length) == data[off:off + length], (off, length)


SMALL = [1, 5, 1023, 1024, 32767, 32768, 32769, 65536, MIB, MIB + 1]


def build_or_none(zt, stream, index=0):
    """the build's blob, or None where it finds no sync point to build from"""
    try:
        return zt.inflate_index_build(stream, index=index)
    except zt.ZtError as e:
        assert e.code == E_NO_INDEX and e.msg == NO_INDEX_TEXT, e
        return None


@pytest.mark.parametrize("kind", ["wordsalad", "xorshift32"])
def test_smallest_shapes(zt, oracle, kind):
    """The blob equals the build's in every case the build succeeds.  A raw
    stream of a single block (inputs up to 32 KiB) holds no sync point before
    its end, so the build answers ZT_E_NO_INDEX for it; the writer still knows
    the one unit, and there the check is the blob's content and the ranges
    read through it."""
    whole = oracle.gen(kind, 41, MIB + 1)
    for n in SMALL:
        d = whole[:n]
        s, blob = zt.deflate_raw_indexed(d)
        assert s == zt.deflate_raw(d), n
        hdr, ent = zt.index_entries(blob)
        assert hdr["total_out"] == n and hdr["end_ip"] == len(s)
        want = build_or_none(zt, s)
        assert (want is None) == (n <= 32768), n
        if want is not None:
            same_blob(zt, blob, want)
        else:
            assert hdr["nunits"] == 1 and hdr["nseg"] == 1
            assert [tuple(int(x) for x in e) for e in ent][1] == (len(s), n, 0, 0)
            if kind == "xorshift32":  # a stored block: run tokens from kStoredRunMin = 1024 bytes on
                assert int(ent["ntok"][0]) == (3 if n >= 1024 else n)
            # the same stream in a container has a sync point before the trailer: there the build agrees
            z, zblob = zt.zlib_compress_indexed(d)
            assert z[2:-4] == s
            same_blob(zt, zblob, zt.inflate_index_build(z, index=2))
            assert zt.index_entries(zblob)[1]["ntok"].tolist() == ent["ntok"].tolist()
        for off, length in [(0, n), (n - 1, 1), (n // 2, 7), (n, 3)]:
            assert zt.inflate_range(s, blob, off, length) == d[off:off + length], (n, off, length)
        if n == MIB:  # ends on a segment boundary: the final call writes no marker behind its last block
            assert hdr["nseg"] == 1 and hdr["nunits"] == 32
        if n == MIB + 1:
            assert hdr["nseg"] >= 2 and hdr["nunits"] == 35


def test_empty_input(zt):
    """the 5-byte stream of the empty input: what the build does, the writers do"""
    s = zt.deflate_raw(b"")
    assert len(s) == 5
    want = build_or_none(zt, s)
    if want is None:
        for call in (zt.deflate_raw_indexed, zt.gzip_compress_indexed, zt.zlib_compress_indexed):
            with pytest.raises(zt.ZtError) as ei:
                call(b"")
            assert ei.value.code == E_NO_INDEX and ei.value.msg == NO_INDEX_TEXT
        assert zt.deflate_raw(b"") == s
        return
    s2, blob = zt.deflate_raw_indexed(b"")
    assert s2 == s
    same_blob(zt, blob, want)


def test_stream_start(zt, data):
    d = data[:3 * MIB // 2 + 77]
    s, blob = zt.deflate_raw_indexed(d, stream_start=37)
    assert s == zt.deflate_raw(d)
    placed = b"\xAA" * 37 + s
    same_blob(zt, blob, zt.inflate_index_build(placed, index=37))
    hdr, ent = zt.index_entries(blob)
    assert hdr["stream_start"] == 37 and hdr["end_ip"] == len(placed) and int(ent["in_off"][0]) == 37
    assert zt.inflate_range(placed, blob, MIB - 5, 10) == d[MIB - 5:MIB + 5]


def test_gzip_and_zlib(zt, data):
    f, blob = zt.gzip_compress_indexed(data, name=b"corpus.bin", mtime=1700000000)
    plain, _ = zt.gzip_compress(data, name=b"corpus.bin", mtime=1700000000)
    assert f == plain
    assert gzip.decompress(f) == data
    hdr, _ = zt.index_entries(blob)
    assert hdr["stream_start"] == 10 + len(b"corpus.bin") + 1
    same_blob(zt, blob, zt.inflate_index_build(f, index=hdr["stream_start"]))
    for off, length in range_cases():
        assert zt.inflate_range(f, blob, off, length) == data[off:off + length], (off, length)

    z, zblob = zt.zlib_compress_indexed(data)
    zplain, _ = zt.zlib_compress(data)
    assert z == zplain
    assert zlib.decompress(z) == data
    zhdr, _ = zt.index_entries(zblob)
    assert zhdr["stream_start"] == 2
    same_blob(zt, zblob, zt.inflate_index_build(z, index=2))
    for off, length in range_cases():
        assert zt.inflate_range(z, zblob, off, length) == data[off:off + length], (off, length)


@pytest.mark.parametrize("n,kind,opts", [
    ((64 << 20) + 1, "mixed", dict(level=6)),            # three pieces, the last a single byte
    ((96 << 20) + 777, "mixed", dict(compression_type=1)),
])
def test_pipelined(zt, n, kind, opts):
    import torch

    d_in = torch.empty(n, dtype=torch.uint8, device="cuda")
    zt.synth_dev(kind, 7, d_in.data_ptr(), n)
    host = d_in.cpu().numpy()
    del d_in
    s, blob = zt.deflate_raw_indexed(memoryview(host), **opts)
    assert s == zt.deflate_raw(memoryview(host), **opts)
    same_blob(zt, blob, zt.inflate_index_build(s))
    hdr, ent = zt.index_entries(blob)
    assert hdr["total_out"] == n and hdr["end_ip"] == len(s)
    # the piece boundaries (deflate_api.cpp: n / 8 clamped to 32..128 MiB, whole segments)
    piece = -(-min(max(n // 8, 32 << 20), 128 << 20) // MIB) * MIB
    bounds = list(range(piece, n, piece))
    assert len(bounds) >= 2
    ranges = []
    for b in bounds:
        ranges += [(b - 1, 2), (b - 40000, 80000), (b, 1)]
    ranges.append((n - 1, 1))
    for (off, length), (st, got) in zip(ranges, zt.inflate_ranges(s, blob, ranges)):
        assert st == 0 and got == host[off:off + length].tobytes(), (off, length)
    # every piece but the last ends with the marker: the next piece's first unit is a segment start
    out_off, flags = ent["out_off"].astype(np.int64), ent["flags"]
    for b in bounds:
        k = int(np.searchsorted(out_off, b, side="right") - 1)  # the last entry at b: the block itself
        assert int(out_off[k]) == b and flags[k] & 1


def test_stored_payload_holding_the_sync_bytes(zt, oracle):
    """64 KiB of random bytes (stored blocks) with 00 00 FF FF planted inside a
    block, between two blocks of text: the build's scan finds a sync point that
    is none, the compressor knows its own unit boundaries"""
    text = oracle.gen("wordsalad", 5, 65536)
    rnd = bytearray(oracle.gen("xorshift32", 6, 65536))
    rnd[40000:40004] = bytes([0, 0, 0xFF, 0xFF])
    d = text[:32768] + bytes(rnd) + text[32768:]
    s, blob = zt.deflate_raw_indexed(d)
    assert s == zt.deflate_raw(d)
    assert zlib.decompress(s, -15) == d
    p = s.find(bytes(rnd[39990:40010]))
    assert p > 0, "the planted block is not stored"
    try:
        want = zt.inflate_index_build(s)
    except zt.ZtError as e:
        assert e.code == E_NO_INDEX, e
        want = None
    if want is not None:
        same_blob(zt, blob, want)
    cases = [(0, len(d)), (32768 + 39990, 30), (32768 + 40004, 1), (32768, 65536), (len(d) - 1, 1), (70000, 5)]
    for off, length in cases:
        assert zt.inflate_range(s, blob, off, length) == d[off:off + length], (off, length)
    for (off, length), (st, got) in zip(cases, zt.inflate_ranges(s, blob, cases)):
        assert st == 0 and got == d[off:off + length], (off, length)


def test_refusals(zt, oracle):
    d = oracle.gen("wordsalad", 9, 100000)
    for call, opts in [(zt.deflate_raw_indexed, dict(compression_type=0)), (zt.deflate_raw_indexed, dict(level=0)),
                       (zt.gzip_compress_indexed, dict(compression_type=0)), (zt.gzip_compress_indexed, dict(level=0)),
                       (zt.zlib_compress_indexed, dict(compression_type=0)), (zt.zlib_compress_indexed, dict(level=0))]:
        with pytest.raises(zt.ZtError) as ei:
            call(d, **opts)
        assert ei.value.code == E_NO_INDEX and ei.value.msg == NO_INDEX_TEXT
    with pytest.raises(zt.ZtError) as ei:
        zt.zlib_compress_indexed(d, dictionary=b"the quick brown fox")
    assert ei.value.code == E_ARG
    s = zt.deflate_raw(d)
    assert zlib.decompress(s, -15) == d
    s2, blob = zt.deflate_raw_indexed(d)
    assert s2 == s and zt.inflate_range(s, blob, 50000, 100) == d[50000:50100]
