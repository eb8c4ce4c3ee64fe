"""Indexed random access (include/zt_index.h): zt_inflate_index_build and
zt_inflate_range / zt_inflate_ranges on the GPU, against slices of the
original input."""
import random
import zlib

import numpy as np
import pytest

import index_corpus
from index_corpus import MIB, TOTAL

pytestmark = pytest.mark.gpu

MARKER = bytes([0, 0, 0, 0xFF, 0xFF, 0, 0, 0, 0xFF, 0xFF])
SYNC = bytes([0, 0, 0xFF, 0xFF])
E_ARG, E_NO_INDEX, E_INDEX, E_MISMATCH, E_NLEN = -103, -60, -61, -62, -14


@pytest.fixture(scope="module")
def zt():
    import ztamd

    assert ztamd.device_count() > 0, "no GPU visible"
    return ztamd


@pytest.fixture(scope="module")
def data(oracle):
    return index_corpus.corpus(oracle)


VARIANTS = {"level6": dict(level=6), "level1": dict(level=1), "fixed": dict(compression_type=1)}


@pytest.fixture(scope="module")
def built(zt, data):
    """per variant: (stream, index blob, header, entries), made once"""
    cache = {}

    def get(name):
        if name not in cache:
            s = zt.deflate_raw(data, **VARIANTS[name])
            blob = zt.inflate_index_build(s)
            hdr, ent = zt.index_entries(blob)
            cache[name] = (s, blob, hdr, ent)
        return cache[name]

    return get


def span_units(ent, off, length):
    """(first, last) units a range needs: the last flagged entry with out_off <=
    off, the entry holding its last byte"""
    out_off = ent["out_off"].astype(np.int64)
    flagged = np.nonzero(ent["flags"][:-1] & 1)[0]
    first = int(flagged[np.searchsorted(out_off[flagged], off, side="right") - 1])
    last = int(np.searchsorted(out_off, off + length - 1, side="right") - 1)
    return first, last


def test_build(zt, data, built):
    s, blob, hdr, ent = built("level6")
    assert zlib.decompress(s, -15) == data  # the truth, cross-checked once
    ref_out, ref_ip = zt.inflate_raw(s)
    assert hdr["total_out"] == len(data) == TOTAL
    assert hdr["end_ip"] == ref_ip and hdr["stream_start"] == 0
    blob2, out, ip = zt.inflate_index_build(s, want_output=True)
    assert out == ref_out == data and ip == ref_ip
    assert blob2 == blob, "the index does not depend on want_output"
    out_off, in_off, flags = ent["out_off"], ent["in_off"], ent["flags"]
    assert np.all(np.diff(out_off.astype(np.int64)) >= 0) and int(out_off[-1]) == hdr["total_out"]
    assert np.all(np.diff(in_off.astype(np.int64)) >= 0) and int(in_off[-1]) == hdr["end_ip"]
    assert int(ent["ntok"][-1]) == 0 and int(flags[-1]) == 0 and int(flags[0]) == 1
    for k in range(1, hdr["nunits"]):
        p = int(in_off[k])
        assert s[p - 4:p] == SYNC, k
        if flags[k] & 1:
            assert s[p - 10:p] == MARKER, k
    spacing = index_corpus.restart_spacing()
    flagged = [int(out_off[k]) for k in range(hdr["nunits"]) if flags[k] & 1]
    # (where a stored block ends a segment, its own empty stored block and the
    # marker's two make two marker patterns in a row: two flagged units at one
    # output offset, the first of them empty)
    assert sorted(set(flagged)) == [0, spacing, 2 * spacing]
    assert hdr["nseg"] == len(flagged)
    for a, b in zip(flagged, flagged[1:]):
        assert b >= a


def range_cases():
    cases = [(0, 1), (0, TOTAL), (TOTAL - 1, 1), (TOTAL, 0), (TOTAL, 5), (TOTAL - 3, 100)]
    for b in (32768, MIB, 2 * MIB):
        cases += [(b - 1, 2), (b, 1), (b - 1, 1)]
    cases.append((MIB - 70000, 140000))
    return cases


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ranges(zt, data, built, variant):
    s, blob, hdr, ent = built(variant)
    assert hdr["total_out"] == TOTAL
    for off, length in range_cases():
        got = zt.inflate_range(s, blob, off, length)
        assert got == data[off:off + length], (off, length)
    assert zt.inflate_range(s, blob, TOTAL - 3, 100) == data[-3:]
    assert zt.inflate_range(s, blob, TOTAL, 5) == b""
    with pytest.raises(zt.ZtError) as ei:
        zt.inflate_range(s, blob, TOTAL + 1, 1)
    assert ei.value.code == E_ARG
    # the same cases in one call
    res = zt.inflate_ranges(s, blob, range_cases())
    for (off, length), (st, got) in zip(range_cases(), res):
        assert st == 0 and got == data[off:off + length], (off, length)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_batch(zt, data, built, variant):
    s, blob, hdr, ent = built(variant)
    rnd = random.Random(20260117)
    ranges = []
    for _ in range(60):
        off = rnd.randrange(TOTAL)
        ranges.append((off, rnd.choice([1, 17, 300, 4096, 65536, 200000])))
    ranges.insert(7, ranges[3])     # two duplicates
    ranges.insert(40, ranges[21])
    ranges.insert(13, (12345, 0))   # two empty ones
    ranges.insert(50, (TOTAL, 9))
    assert len(ranges) == 64
    zt.index_stats(reset=True)
    rc, res = zt.inflate_ranges(s, blob, ranges, return_code=True)
    st = zt.index_stats()
    assert rc == 0
    need = set()
    clamped = 0
    for (off, length), (code, got) in zip(ranges, res):
        assert code == 0 and got == data[off:off + length], (off, length)
        n = min(length, TOTAL - off)
        clamped += n
        if n:
            first, last = span_units(ent, off, n)
            need.update(range(first, last + 1))
    assert 1 <= st["units_tokenized"] <= len(need)
    assert st["out_bytes_returned"] == clamped
    assert st["ranges"] == 64 and st["range_calls"] == 1


def test_bounded_work(zt, data, built):
    s, blob, hdr, ent = built("level6")
    off = 3 * MIB // 2
    first, last = span_units(ent, off, 1)
    assert int(ent["out_off"][first]) == MIB
    paths = zt.timing_read()["inflate_paths"]
    zt.index_stats(reset=True)
    assert zt.inflate_range(s, blob, off, 1) == data[off:off + 1]
    st = zt.index_stats()
    assert 1 <= st["units_tokenized"] <= last - first + 1
    assert st["in_bytes_uploaded"] <= int(ent["in_off"][last + 1]) - int(ent["in_off"][first]) + 4096
    assert st["out_bytes_decoded"] <= int(ent["out_off"][last + 1]) - int(ent["out_off"][first])
    assert zt.timing_read()["inflate_paths"] == paths


@pytest.mark.parametrize("mode", ["sync", "full"])
def test_foreign_streams(zt, oracle, mode):
    step = 10007
    d = oracle.gen("wordsalad", step, 600000) + oracle.gen("structured", step, 300000) + b"ab" * 50000
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    flush = zlib.Z_SYNC_FLUSH if mode == "sync" else zlib.Z_FULL_FLUSH
    parts = [c.compress(d[o:o + step]) + c.flush(flush) for o in range(0, len(d), step)]
    parts.append(c.flush())
    s = b"".join(parts)
    blob, out, ip = zt.inflate_index_build(s, want_output=True)
    assert out == d and ip == len(s)
    hdr, ent = zt.index_entries(blob)
    assert hdr["total_out"] == len(d)
    assert int(np.sum(ent["flags"] & 1)) == 1 and hdr["nseg"] == 1  # no double marker in these streams
    total = len(d)
    for off, length in [(0, 1), (500000, 30000), (total - 1, 1)]:
        assert zt.inflate_range(s, blob, off, length) == d[off:off + length], (off, length)
    zt.index_stats(reset=True)
    assert zt.inflate_range(s, blob, 500000, 1) == d[500000:500001]
    holding = int(np.searchsorted(ent["out_off"].astype(np.int64), 500000, side="right") - 1)
    assert zt.index_stats()["units_tokenized"] == holding + 1


def test_not_indexable(zt, oracle):
    d = oracle.gen("wordsalad", 5, 256 << 10)
    s = zlib.compress(d, 6)[2:-4]
    with pytest.raises(zt.ZtError) as ei:
        zt.inflate_index_build(s)
    assert ei.value.code == E_NO_INDEX and ei.value.msg == "stream has no usable sync points"
    out, ip = zt.inflate_raw(s)
    assert out == d and ip == len(s)


def test_corrupt_stream_keeps_its_status(zt, data, built):
    """a corrupt stream's build fails with what zt_inflate_raw reports for it"""
    s = bytearray(built("level6")[0][:200000])  # cut: the stream ends without BFINAL
    with pytest.raises(zt.ZtError) as want:
        zt.inflate_raw(bytes(s))
    with pytest.raises(zt.ZtError) as ei:
        zt.inflate_index_build(bytes(s))
    assert ei.value.code == want.value.code and ei.value.code != E_NO_INDEX


def test_verified_not_trusted(zt, data, built):
    s, blob, hdr, ent = built("level6")
    off, length = 3 * MIB // 2, 1000
    first, last = span_units(ent, off, length)
    good = data[off:off + length]

    def ok():  # a correct call still returns correct bytes: no state was poisoned
        assert zt.inflate_range(s, blob, off, length) == good

    def fails(stream, idx, codes, o=off, n=length):
        with pytest.raises(zt.ZtError) as ei:
            zt.inflate_range(stream, idx, o, n)
        assert ei.value.code in codes, ei.value
        ok()

    # the NLEN of the empty stored block that ends unit k - 1, inside the span
    k = first + 3
    assert first < k <= last
    p = int(ent["in_off"][k])
    assert s[p - 4:p] == SYNC
    bad = bytearray(s)
    bad[p - 1] = 0xFE
    bad = bytes(bad)
    fails(bad, blob, (E_NLEN, E_MISMATCH))
    fails(bad, blob, (E_NLEN, E_MISMATCH), MIB + 5, 200000)
    rc, res = zt.inflate_ranges(bad, blob, [(off, length), (MIB, 1), (off + 5, 0)], return_code=True)
    assert rc in (E_NLEN, E_MISMATCH) and res[0][0] != 0 and res[1][0] != 0 and res[2] == (0, b"")
    assert zt.inflate_range(bad, blob, 100, 50) == data[100:150]  # another segment
    assert zt.inflate_range(bad, blob, 2 * MIB + 7, 50) == data[2 * MIB + 7:2 * MIB + 57]
    ok()
    # one flipped out_off
    ent2 = ent.copy()
    ent2["out_off"][k] += 1
    blob2 = blob[:64] + ent2.tobytes()
    fails(s, blob2, (E_INDEX, E_MISMATCH))
    # one wrong token count
    ent3 = ent.copy()
    ent3["ntok"][k] -= 1
    fails(s, blob[:64] + ent3.tobytes(), (E_INDEX, E_MISMATCH))
    # a unit boundary moved into the middle of a block
    ent4 = ent.copy()
    ent4["in_off"][k] += 1
    fails(s, blob[:64] + ent4.tobytes(), (E_INDEX, E_MISMATCH))
    # an unflagged unit passed off as a segment start: the range's span then
    # starts inside a segment
    ent5 = ent.copy()
    ent5["flags"][k] = 1
    hdr5 = bytearray(blob[:64])
    hdr5[12:16] = (hdr["nseg"] + 1).to_bytes(4, "little")
    with pytest.raises(zt.ZtError) as ei:
        zt.inflate_range(s, bytes(hdr5) + ent5.tobytes(), off, length)
    assert ei.value.code != 0
    ok()
    # a truncated blob, and the input cut below end_ip
    fails(s, blob[:-7], (E_INDEX,))
    fails(s, blob[:70], (E_INDEX,))
    fails(s[:hdr["end_ip"] - 1], blob, (E_INDEX,))
    fails(s, b"ZTIY" + blob[4:], (E_INDEX,))
