"""Checkpoint index (include/zt_checkpoint.h): zt_inflate_ckpt_build and
zt_inflate_ckpt_range / zt_inflate_ckpt_ranges on the GPU, on streams without
sync points made on the CPU (zlib at several levels and strategies, stored
blocks, the reference's one-block stream, a gzip file) and on one of the
engine's own, against slices of the original input."""
import gzip
import random
import zlib

import numpy as np
import pytest

import index_corpus
from index_corpus import MIB, TOTAL

pytestmark = pytest.mark.gpu

SPAN = 256 << 10
WIN = 32768
BLOCK, HUFF, STORED, SHDR, FINAL = 0, 1, 2, 3, 4
E_ARG, E_NO_INDEX, E_INDEX, E_MISMATCH = -103, -60, -61, -62
INFLATE_ERRORS = set(range(-17, -9))

VARIANTS = ["zlib6", "zlib1", "zlib9", "fixed", "huffonly", "stored", "reference", "own", "gzip"]


@pytest.fixture(scope="module")
def zt():
    import ztamd

    assert ztamd.device_count() > 0, "no GPU visible"
    return ztamd


@pytest.fixture(scope="module")
def data(oracle):
    return index_corpus.corpus(oracle)


def _zlib_raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return co.compress(data) + co.flush()


def make_stream(name, data, oracle, zt):
    """(buffer, index): the raw stream starts at buffer[index]"""
    if name == "zlib6":
        return _zlib_raw(data, 6), 0
    if name == "zlib1":
        return _zlib_raw(data, 1), 0
    if name == "zlib9":
        return _zlib_raw(data, 9), 0
    if name == "fixed":
        return _zlib_raw(data, 6, zlib.Z_FIXED), 0
    if name == "huffonly":
        return _zlib_raw(data, 6, zlib.Z_HUFFMAN_ONLY), 0
    if name == "stored":
        return _zlib_raw(data, 0), 0
    if name == "reference":
        return oracle.raw_deflate(data)[0], 0
    if name == "own":
        return zt.deflate_raw(data, level=6), 0
    if name == "gzip":
        return gzip.compress(data, mtime=0), 10
    raise KeyError(name)


@pytest.fixture(scope="module")
def built(zt, data, oracle):
    """per variant: (buffer, index, blob, header, entries, windows), made once"""
    cache = {}

    def get(name):
        if name not in cache:
            s, index = make_stream(name, data, oracle, zt)
            blob = zt.inflate_ckpt_build(s, index=index, span=SPAN)
            hdr, ent, wins = zt.ckpt_entries(blob)
            cache[name] = (s, index, blob, hdr, ent, wins)
        return cache[name]

    return get


def window_entries(ent):
    return [k for k in range(len(ent) - 1) if int(ent["flags"][k]) & 1]


def span_units(ent, off, length):
    """(first, last) units a range needs: the last of entry 0 and the window
    entries with out_off <= off, the entry holding its last byte"""
    out_off = ent["out_off"].astype(np.int64)
    starts = np.array([0] + window_entries(ent))
    first = int(starts[np.searchsorted(out_off[starts], off, side="right") - 1])
    last = int(np.searchsorted(out_off[:-1], off + length - 1, side="right") - 1)
    return first, last


@pytest.mark.parametrize("name", VARIANTS)
def test_build(zt, data, built, name):
    s, index, blob, hdr, ent, wins = built(name)
    if name == "gzip":
        assert zlib.decompress(s[index:], -15) == data
    else:
        assert zlib.decompress(s, -15) == data  # the truth, cross-checked once
    ref_out, ref_ip = zt.inflate_raw(s, index=index)
    assert ref_out == data
    assert hdr["total_out"] == len(data) == TOTAL
    assert hdr["end_ip"] == ref_ip and hdr["stream_start"] == index and hdr["span"] == SPAN
    if name == "gzip":
        assert hdr["end_ip"] + 8 == len(s)
    blob2, out, ip = zt.inflate_ckpt_build(s, index=index, span=SPAN, want_output=True)
    assert out == data and ip == ref_ip
    assert blob2 == blob, "the blob does not depend on want_output"
    pos, out_off, kind, flags = (ent[f].astype(np.int64) for f in ("pos", "out_off", "kind", "flags"))
    n = hdr["nunits"]
    assert n >= 20, "the stream is cut into many units"
    assert np.all(np.diff(pos) >= 0) and np.all(np.diff(out_off) >= 0)
    # entry 0: the stream start, a block start, no window
    assert pos[0] == 8 * index and kind[0] == BLOCK and out_off[0] == 0 and flags[0] == 0
    assert int(ent["hdr"][0]) == 0 and int(ent["rem"][0]) == 0 and int(ent["win"][0]) == 0
    # the sentinel
    assert kind[n] == FINAL and out_off[n] == TOTAL and (pos[n] + 7) // 8 == hdr["end_ip"]
    assert all(int(ent[f][n]) == 0 for f in ("hdr", "rem", "flags", "ntok", "win"))
    assert np.all(kind[:n] <= SHDR)
    # window entries: exactly the first entry at or after each multiple of span
    want = []
    for m in range(SPAN, TOTAL, SPAN):
        ks = np.nonzero(out_off[1:n] >= m)[0]
        if len(ks) and (not want or want[-1] != int(ks[0]) + 1):
            want.append(int(ks[0]) + 1)
    have = window_entries(ent)
    assert have == want and len(have) == hdr["nwin"] == len(wins) and len(have) >= 8
    for w, k in enumerate(have):
        assert int(ent["win"][k]) == w
        o = int(out_off[k])
        assert wins[w][0] == data[o - WIN:o], (name, w)
        assert wins[w][1] == zlib.crc32(data[o - WIN:o]), (name, w)
    assert len(blob) == 64 + 48 * (n + 1) + 32784 * len(wins)
    huff = kind[:n] == HUFF
    if name == "reference":
        assert huff.sum() >= n - 2 and np.all(ent["hdr"][:n][huff] == 0), "one block: every entry names bit 0"
    if name == "fixed":
        assert np.all(ent["hdr"][:n][huff] == zt.CKPT_FIXED_HDR)
    if name == "stored":
        st = kind[:n] == STORED
        assert st.sum() >= 10, "checkpoints inside stored payloads"
        assert np.all(ent["rem"][:n][st] >= 1) and np.all(pos[:n][st] % 8 == 0)


def range_cases(ent):
    cases = [(0, 1), (0, TOTAL), (TOTAL - 1, 1), (TOTAL, 0), (TOTAL, 5), (TOTAL - 3, 100)]
    marks = [WIN] + [int(ent["out_off"][k]) for k in window_entries(ent)] + [MIB, 2 * MIB]
    for b in marks:
        cases += [(b - 1, 2), (b, 1), (b - 1, 1)]
    cases.append((MIB - 70000, 140000))
    return cases


@pytest.mark.parametrize("name", VARIANTS)
def test_ranges(zt, data, built, name):
    s, index, blob, hdr, ent, wins = built(name)
    cases = range_cases(ent)
    for off, ln in cases:
        assert zt.inflate_ckpt_range(s, blob, off, ln) == data[off:off + ln], (name, off, ln)
    with pytest.raises(zt.ZtError) as ei:
        zt.inflate_ckpt_range(s, blob, TOTAL + 1, 1)
    assert ei.value.code == E_ARG
    # the same cases in one call, and one range past the end among them
    rc, res = zt.inflate_ckpt_ranges(s, blob, cases + [(TOTAL + 1, 1)], return_code=True)
    assert rc == E_ARG
    for (off, ln), (st, got) in zip(cases, res):
        assert st == 0 and got == data[off:off + ln], (name, off, ln)
    assert res[-1] == (E_ARG, None)


@pytest.mark.parametrize("name", ["zlib6", "reference", "stored"])
def test_batch_no_unit_twice(zt, data, built, name):
    s, index, blob, hdr, ent, wins = built(name)
    rng = random.Random(20250 + len(name))
    ranges = []
    for i in range(64):
        if i % 8 == 7:
            ranges.append(ranges[rng.randrange(len(ranges))])  # a repeat
        else:
            ln = rng.randint(1, 200000)
            ranges.append((rng.randrange(0, TOTAL - ln), ln))
    zt.ckpt_stats(reset=True)
    res = zt.inflate_ckpt_ranges(s, blob, ranges)
    stats = zt.ckpt_stats()
    for (off, ln), (st, got) in zip(ranges, res):
        assert st == 0 and got == data[off:off + ln], (name, off, ln)
    units = set()
    for off, ln in ranges:
        a, b = span_units(ent, off, ln)
        units.update(range(a, b + 1))
    assert stats["range_calls"] == 1 and stats["ranges"] == 64
    assert stats["units_tokenized"] <= len(units), "no unit is decoded twice"
    assert stats["out_bytes_returned"] == sum(ln for _, ln in ranges)


def test_bounded_work(zt, data, built):
    """a 1-byte range decodes from one window checkpoint and no further than the next"""
    s, index, blob, hdr, ent, wins = built("zlib6")
    off = TOTAL // 2
    we = window_entries(ent)
    out_off = ent["out_off"].astype(np.int64)
    prev = max(k for k in we if out_off[k] <= off)
    nxt = min(k for k in we if out_off[k] > off)
    zt.ckpt_stats(reset=True)
    assert zt.inflate_ckpt_range(s, blob, off, 1) == data[off:off + 1]
    st = zt.ckpt_stats()
    print("bounded work:", st)
    assert st["range_calls"] == 1 and st["window_bytes_uploaded"] == WIN
    between = (int(ent["pos"][nxt]) + 7) // 8 - int(ent["pos"][prev]) // 8
    # one relocated block header (at most 287 bytes, RFC 1951) and the 64-byte packing alignment
    assert st["in_bytes_uploaded"] <= between + 287 + 64
    assert st["out_bytes_decoded"] <= 2 * SPAN
    assert st["out_bytes_returned"] == 1
    # an empty range never reaches the device
    zt.ckpt_stats(reset=True)
    assert zt.inflate_ckpt_range(s, blob, TOTAL, 7) == b""
    assert zt.ckpt_stats()["range_calls"] == 0


def test_small_stream(zt, data):
    """below the general path's 16 KiB minimum: one exact unit, no window"""
    small = data[:40000]
    s = _zlib_raw(small, 6)
    assert len(s) < (1 << 14)
    blob, out, ip = zt.inflate_ckpt_build(s, span=SPAN, want_output=True)
    assert out == small and ip == len(s)
    assert zt.inflate_ckpt_build(s, span=SPAN) == blob
    hdr, ent, wins = zt.ckpt_entries(blob)
    assert hdr["nunits"] == 1 and hdr["nwin"] == 0 and wins == [] and hdr["total_out"] == 40000
    assert int(ent["kind"][0]) == BLOCK and int(ent["kind"][1]) == FINAL and int(ent["out_off"][1]) == 40000
    for off, ln in [(0, 1), (0, 40000), (39999, 1), (40000, 0), (40000, 5), (39990, 100), (WIN - 1, 2), (12345, 6789)]:
        assert zt.inflate_ckpt_range(s, blob, off, ln) == small[off:off + ln]
    res = zt.inflate_ckpt_ranges(s, blob, [(5, 10), (30000, 20000), (5, 10)])
    assert [r[1] for r in res] == [small[5:15], small[30000:], small[5:15]]
    # a few bytes: the empty stream and a one-literal stream
    for payload in (b"", b"a"):
        t = _zlib_raw(payload, 6)
        b2, o2, ip2 = zt.inflate_ckpt_build(t, want_output=True)
        assert o2 == payload and ip2 == len(t)
        assert zt.inflate_ckpt_range(t, b2, 0, 10) == payload


def test_build_arguments_and_refusals(zt, data, built):
    s = built("zlib6")[0]
    with pytest.raises(zt.ZtError) as ei:
        zt.inflate_ckpt_build(s, span=65535)
    assert ei.value.code == E_ARG
    # a corrupt stream reports its usual inflate status, as zt_inflate_raw does
    bad = bytearray(s)
    bad[len(bad) // 2] ^= 0x55
    try:
        zt.inflate_raw(bytes(bad))
        raw_code = 0
    except zt.ZtError as e:
        raw_code = e.code
    if raw_code:
        with pytest.raises(zt.ZtError) as ei:
            zt.inflate_ckpt_build(bytes(bad), span=SPAN)
        assert ei.value.code == raw_code
    # the sync-point index still has nothing to say about such a stream
    with pytest.raises(zt.ZtError) as ei:
        zt.inflate_index_build(s)
    assert ei.value.code == E_NO_INDEX


def _put(blob, at, val, width):
    b = bytearray(blob)
    b[at:at + width] = int(val).to_bytes(width, "little")
    return bytes(b)


def test_structural_errors_before_any_device_work(zt, data, built):
    s, index, blob, hdr, ent, wins = built("zlib6")
    n = hdr["nunits"]
    E, K = 64, 48
    k = n // 2
    w1 = window_entries(ent)[1]
    ix = zt.inflate_index_build(built("own")[0])
    assert ix[:4] == b"ZTIX"
    bad = {
        "truncated": blob[:-1],
        "truncated to the header": blob[:64],
        "magic": b"ZTCX" + blob[4:],
        "a sync-point index": ix,
        "pos beyond n": _put(blob, E + k * K, 8 * len(s) + 8, 8),
        "out_off decreases": _put(blob, E + k * K + 16, int(ent["out_off"][k - 1]) - 1, 8),
        "window index out of range": _put(blob, E + w1 * K + 40, hdr["nwin"], 4),
    }
    zt.ckpt_stats(reset=True)
    for what, b in bad.items():
        with pytest.raises(zt.ZtError) as ei:
            zt.inflate_ckpt_range(s, b, 100, 10)
        assert ei.value.code == E_INDEX, what
        with pytest.raises(zt.ZtError) as ei:
            zt.inflate_ckpt_ranges(s, b, [(100, 10), (TOTAL, 0)])
        assert ei.value.code == E_INDEX, what
    assert zt.ckpt_stats()["range_calls"] == 0, "stopped before any device work"
    # and the other way round: the sync-point reader refuses a checkpoint blob
    with pytest.raises(zt.ZtError) as ei:
        zt.inflate_range(s, blob, 100, 10)
    assert ei.value.code == E_INDEX


def test_device_checks(zt, data, built):
    s, index, blob, hdr, ent, wins = built("zlib6")
    n = hdr["nunits"]
    E, K = 64, 48
    we = window_entries(ent)
    # one flipped window byte: the CRC-32 check on the device
    w = 2
    o = int(ent["out_off"][we[w]])
    at = E + (n + 1) * K + w * 32784 + 12345
    flipped = bytearray(blob)
    flipped[at] ^= 1
    flipped = bytes(flipped)
    with pytest.raises(zt.ZtError) as ei:
        zt.inflate_ckpt_range(s, flipped, o + 10, 100)
    assert ei.value.code == E_INDEX
    rc, res = zt.inflate_ckpt_ranges(s, flipped, [(o + 10, 100), (5, 10), (TOTAL, 0)], return_code=True)
    assert rc == E_INDEX and res[0] == (E_INDEX, None) and res[1][0] != 0 and res[2] == (0, b"")
    # a range that does not start from that window is served
    assert zt.inflate_ckpt_range(s, flipped, 5, 10) == data[5:15]
    # an entry's pos moved by one bit: a Huffman entry (the others are byte aligned) that is no window entry
    k = next(k for k in range(n // 2, n) if int(ent["kind"][k]) == HUFF and k not in we)
    moved = _put(blob, E + k * K, int(ent["pos"][k]) + 1, 8)
    ko = int(ent["out_off"][k])
    rc, res = zt.inflate_ckpt_ranges(s, moved, [(ko - 5, 10), (7, 3), (TOTAL, 0), (TOTAL - 9, 9)], return_code=True)
    allowed = INFLATE_ERRORS | {E_MISMATCH}
    assert rc in allowed
    assert res[0][0] in allowed and res[1][0] in allowed and res[3][0] in allowed
    assert all(r[1] is None for r in (res[0], res[1], res[3])) and res[2] == (0, b"")
    # ranges whose spans do not hold the moved entry are served
    assert zt.inflate_ckpt_range(s, moved, 7, 3) == data[7:10]
    # one stream's blob with another stream of the same data: an error, or that stream's own bytes
    s9 = built("zlib9")[0]
    assert len(s9) < len(s)
    padded = s9 + bytes(len(s) - len(s9))
    for off, ln in [(0, 100), (MIB, 5000), (TOTAL - 50, 50)]:
        rc, res = zt.inflate_ckpt_ranges(padded, blob, [(off, ln)], return_code=True)
        st, got = res[0]
        assert (st in allowed | {E_INDEX} and got is None) or (st == 0 and got == data[off:off + ln]), (off, st)
