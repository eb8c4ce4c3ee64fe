"""The deflate match stage held to a brute-force LZ77 reference, position by
position.

ztamd.debug_match returns what match_kernel (csrc/deflate.hip) wrote -- one
word per position, byte << 24 | len << 15 | dist -- before price, DP, parse
and Huffman turn it into a stream, over a result buffer filled with
0xFFFFFFFF.  tests/lz77_ref.py states what should be there without the
kernel's hash tables: the window (DF_MAXDIST, not before the segment start),
the length cap (258, the block's end, the data's end) and, per position, L*:
the longest match among the candidates that share the position's first 8
bytes.  The inputs (tests/match_audit_inputs.py) plant copies where the kernel
can go wrong: quad lanes, 64-lane exchanges, 256-position super-steps,
sub-chunk ends and their heads, block ends, super-chunk starts, the 1 MiB
restart point, the data's ragged end and the window's edge.  Every constant
comes from the library's own record (info); the tests state none.

1. coverage and soundness, every shipped way of searching: every position is
   written, carries its byte, and a match is inside its window and its length
   cap, equals its source byte for byte, and from 8 bytes on is its
   candidate's full extension (but for two rules of the kernel, stated where
   they are checked: a carried 257 after a match cut at 258, and the 8-byte
   cap of the near probes and the 4-byte table).
2. exhaustive completeness: with 512 hops and at level 9 as shipped, every
   position holds at least min(L*, nice_len, skip_len - 1), and exactly L*
   wherever neither bound applies.  No tolerance: not one position may miss.
3. queued and at-once measurement, u16 and u32 heads: the same words.
4. what the shipped levels' streams do with the planted copies (the DP and the
   parse held to ground truth as well), a dictionary batch included.
"""
import contextlib
import os
import zlib
from collections import namedtuple

import numpy as np
import pytest

import deflate_audit
import lz77_ref as ref
import match_audit_inputs as inputs

pytestmark = pytest.mark.gpu

KIB = 1024
LEVELS = [1, 4, 6, 9]
HALO = 32 * KIB
UNWRITTEN = 0xFFFFFFFF
# check 2: "max_chain,nice,lazy,skip,klen,probe,good" (ZT_DF_PARAMS); None: level 9 as shipped
EXHAUSTIVE = {"nice258": "512,258,1,4096,8,16,258", "nice128": "512,128,1,128,8,16,16", "nice16": "512,16,1,16,8,16,4",
              "level9": None}

Input = namedtuple("Input", "data copies env ref halo_data halo_ref")


@pytest.fixture(scope="module")
def zt():
    import ztamd

    return ztamd


@contextlib.contextmanager
def env(**kw):
    """ZT_DF_* hooks for the calls inside (the library reads them per call)."""
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def info(zt):
    """the library's constants (a call on a few bytes: the parameters in it are level 6's)"""
    return zt.debug_match(b"match audit", level=6)[2]


def geom(info):
    return ref.Geom(info["block"], info["segment"], info["maxdist"])


def halo_for(data, g, seed):
    """HALO bytes of filler in front of `data`, with pieces of the data's
    first 3 KiB in it: sources in the halo, one at the window's edge and one
    just beyond it."""
    rng = np.random.RandomState(seed)
    h = (rng.randint(0, inputs.ALPHA_N, size=HALO) + inputs.ALPHA0).astype(np.uint8)
    d = np.frombuffer(data, dtype=np.uint8)
    for j, (dist, ln) in enumerate([(300, 9), (5000, 33), (g.maxdist, 258), (g.maxdist + 1, 128), (17000, 17),
                                    (3000, 64)]):
        y = 64 + 500 * j
        x = HALO + y - dist
        h[x:x + ln] = d[y:y + ln]
    return h.tobytes() + data


@pytest.fixture(scope="module")
def cases(info):
    """The inputs and their references, computed once."""
    g, sub = geom(info), info["sub"]
    made = {
        "matrix": inputs.matrix(g, sub) + ({},),
        "super4": inputs.small(g, sub, 160 * KIB + 511, 2, 21, True) + ({"ZT_DF_SUPER_MIN": 4},),
        "ragged1": inputs.small(g, sub, 8 * KIB + 1, 3, 22) + ({},),
        "ragged63": inputs.small(g, sub, 8 * KIB + 63, 5, 23) + ({},),
        "ragged513": inputs.small(g, sub, 8 * KIB + 513, 8, 24) + ({},),
        "vocab": (inputs.vocabulary_text(96 * KIB + 13), [], {}),
    }
    out = {}
    for k, (name, (data, copies, e)) in enumerate(sorted(made.items())):
        hd = halo_for(data, g, 100 + k)
        out[name] = Input(data, copies, e, ref.longest_keyed(data, g), hd, ref.longest_keyed(hd, g, HALO))
    assert out["vocab"].ref[2] <= 64 and out["vocab"].halo_ref[2] <= 64, "the text's key multiplicity"
    return out


NAMES = ["matrix", "super4", "ragged1", "ragged63", "ragged513", "vocab"]


def fields(res):
    return (res >> 15) & 511, res & 0x7FFF, res >> 24


def describe(i, res, best=None, dist=None):
    s = "position %d: res %#010x (len %d dist %d)" % (i, res[i], (res[i] >> 15) & 511, res[i] & 0x7FFF)
    if best is not None:
        s += ", L* %d at distance %d" % (best[i], dist[i])
    return s


def report(what, bad, res, best=None, dist=None):
    idx = np.nonzero(bad)[0]
    if idx.size == 0:
        return []
    return ["%s: %d positions\n    " % (what, idx.size) + "\n    ".join(describe(i, res, best, dist) for i in idx[:8])]


def soundness(res, store, data, halo, info):
    """check 1 on one result; returns (failure texts, positions checked, matches checked)"""
    g = geom(info)
    d = np.frombuffer(data, dtype=np.uint8)
    n = d.size - halo
    fails = []
    if store.any():
        fails.append("blocks flagged stored: %s" % np.nonzero(store)[0].tolist())
    fails += report("never written", res == UNWRITTEN, res)
    ln, dist, byte = fields(res)
    fails += report("not the position's byte", (byte != d[halo:]) & (res != UNWRITTEN), res)
    pos = np.arange(n, dtype=np.int64)
    ml = np.minimum(np.minimum(ref.MAX_MATCH, (pos // g.block + 1) * g.block - pos), n - pos)
    seg = pos // g.segment
    lo = np.maximum(halo + pos - g.maxdist, np.where(seg == 0, 0, halo + seg * g.segment))
    m = (ln != 0) & (res != UNWRITTEN)
    fails += report("a length below 3", m & (ln < 3), res)
    fails += report("longer than max_len", m & (ln > ml), res)
    fails += report("distance outside 1..DF_MAXDIST", m & ((dist < 1) | (dist > g.maxdist)), res)
    fails += report("source before the segment start or the buffer", m & (halo + pos - dist < lo), res)
    fails += report("a far 3-byte match", m & (ln == 3) & (dist > info["too_far"]), res)
    ok = m & (ln >= 3) & (ln <= ml) & (dist >= 1) & (halo + pos - dist >= 0)
    i = pos[ok]
    a, q, li = halo + i, halo + i - dist[ok].astype(np.int64), ln[ok].astype(np.int64)
    wrong = np.zeros(i.size, dtype=bool)
    for k in range(int(li.max()) if i.size else 0):
        live = np.nonzero(li > k)[0]
        wrong[live] |= d[a[live] + k] != d[q[live] + k]
    bad = np.zeros(n, dtype=bool)
    bad[i[wrong]] = True
    fails += report("source and position differ inside the match", bad, res)
    # from 8 bytes on a length is its candidate's full extension (shorter ones
    # come from the near probes and the 4-byte table, capped there by design).
    # A rule of the kernel: the second position of a pair starts from the
    # first one's match less its first byte; where that match was cut at 258
    # bytes, the carried 257 may stop one byte short of the candidate's
    # extension (a search that may take the carried match as it is -- skip_len
    # -- or ends before it reaches that candidate again leaves it so)
    prev = np.concatenate([[0], res[:-1]])
    carried = (fields(prev)[0] == ref.MAX_MATCH) & (ln == ref.MAX_MATCH - 1) & (fields(prev)[1] == dist) & (pos % 2 == 1)
    # A second rule: the near probes and the 4-byte table measure 8 bytes at
    # most, so a length of exactly 8 is a cap, not an extension, where the
    # chain walk ended before it reached the same source -- at a probed
    # distance, or at the nearest earlier position with the same 4 bytes (the
    # table holds no other)
    capped = (ln == ref.KEY) & ((dist <= info["probe"]) | (dist == ref.nearest_same_prefix(d, 4)[halo:]))
    full = np.nonzero((li >= ref.KEY) & (li < ml[i]) & ~carried[i] & ~capped[i])[0]
    pad = np.concatenate([d, np.zeros(1, dtype=np.uint8)])
    short = full[pad[a[full] + li[full]] == pad[q[full] + li[full]]]
    bad = np.zeros(n, dtype=bool)
    bad[i[short]] = True
    fails += report("not extended to the first differing byte", bad, res)
    return fails, n, int(i.size)


def completeness(res, best, dist, info):
    """check 2 on one result; returns (failure texts, positions with L* >= 8)"""
    ln = fields(res)[0].astype(np.int64)
    ln[res == UNWRITTEN] = 0
    ls = best.astype(np.int64)
    have = ls >= ref.KEY
    nice, skip = info["nice_len"], info["skip_len"]
    fails = report("below min(L*, nice_len, skip_len - 1)", have & (ln < np.minimum(ls, min(nice, skip - 1))), res, best,
                   dist)
    # where the previous position's match was not taken without a search and
    # the walk did not stop at nice_len, this bound and check 1's force L* itself
    prev = np.concatenate([[0], ln[:-1]])
    fails += report("not L* although neither nice_len nor skip_len applies",
                    have & (prev < skip) & (ln < nice) & (ln != ls), res, best, dist)
    return fails, int(have.sum())


def run(zt, case, level, halo=0, **extra):
    with env(**dict(case.env, **extra)):
        return zt.debug_match(case.halo_data if halo else case.data, level=level, halo=halo)


@pytest.mark.parametrize("halo", [0, HALO])
@pytest.mark.parametrize("name", NAMES)
def test_coverage_and_soundness(zt, cases, name, halo):
    case = cases[name]
    fails = []
    for level in LEVELS:
        res, store, info = run(zt, case, level, halo)
        assert info["blocks_per_wg"] == (4 if name == "super4" else 1)
        f, npos, nmatch = soundness(res, store, case.halo_data if halo else case.data, halo, info)
        print("%s halo %d level %d: %d positions, %d matches checked" % (name, halo, level, npos, nmatch))
        fails += ["level %d: %s" % (level, x) for x in f]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("params", sorted(EXHAUSTIVE))
@pytest.mark.parametrize("name", NAMES)
def test_exhaustive_completeness(zt, cases, name, params):
    case = cases[name]
    res, store, info = run(zt, case, 9, ZT_DF_PARAMS=EXHAUSTIVE[params])
    assert info["max_chain"] == 512 and info["klen"] == ref.KEY
    if EXHAUSTIVE[params]:
        assert [info[k] for k in ("nice_len", "skip_len", "good")] == [int(v) for v in
                                                                       np.array(EXHAUSTIVE[params].split(","))[[1, 3, 6]]]
    best, dist, mult = case.ref
    fails, have = completeness(res, best, dist, info)
    fails += soundness(res, store, case.data, 0, info)[0]
    print("%s %s: %d positions with L* >= 8, key multiplicity %d" % (name, params, have, mult))
    assert have > 500
    assert not fails, "\n".join(fails)


def test_exhaustive_completeness_with_a_halo(zt, cases):
    """the shard case: sources in the halo, the window's edge inside it"""
    for name in ("matrix", "super4", "vocab"):
        case = cases[name]
        res, store, info = run(zt, case, 9, HALO, ZT_DF_PARAMS=EXHAUSTIVE["nice258"])
        best, dist, mult = case.halo_ref
        fails, have = completeness(res, best, dist, info)
        assert best[64 + 1000] == 258 and dist[64 + 1000] == info["maxdist"], "the halo's copy at the window's edge"
        if name != "vocab":  # (text repeats anyway)
            assert best[64 + 1500] == 0, "the halo's copy beyond the window"
        print("%s halo: %d positions with L* >= 8" % (name, have))
        assert not fails, "\n".join(fails)


def test_ways_of_measuring_give_the_same_words(zt, cases):
    case = cases["vocab"]
    zt.debug_match_modes()  # (clears)
    base = run(zt, case, 6, ZT_DF_MQ=0)[0]
    assert zt.debug_match_modes()[0] == 0
    queued = run(zt, case, 6, ZT_DF_MQ=1)[0]
    assert zt.debug_match_modes()[0] >= 1, "no block measured through the queues"
    assert not (base == UNWRITTEN).any()
    for what, other in (("ZT_DF_MQ=1", queued), ("ZT_DF_HEADS=16", run(zt, case, 6, ZT_DF_HEADS=16)[0]),
                        ("ZT_DF_HEADS=32", run(zt, case, 6, ZT_DF_HEADS=32)[0])):
        assert not report(what + " differs from ZT_DF_MQ=0", other != base, other)


def token_cover(blocks, n, history=0):
    """dist_at[n]: the distance of the match token over each position (0: a literal)"""
    cover = np.zeros(n, dtype=np.int64)
    at = 0
    for b in blocks:
        for t in b.tokens:
            if isinstance(t, tuple):
                cover[at:at + t[0]] = t[1]
                at += t[0]
            else:
                at += 1
    assert at == n
    return cover


def stream_check(cover, copies, g, what):
    must, never = inputs.coverable(copies, g), inputs.forbidden(copies, g)
    share = [inputs.covered(cover, c) / c.length for c in must]
    fails = ["%s: %d of %d bytes at distance %d: %s" % (what, inputs.covered(cover, c), c.length, c.dist, (c,))
             for c in must if inputs.covered(cover, c) < c.length - 16]
    fails += ["%s: covered at a distance no match may have: %s" % (what, (c,)) for c in never if inputs.covered(cover, c)]
    return fails, len(must), len(never), min(share)


@pytest.mark.parametrize("level", LEVELS)
def test_shipped_levels_cover_the_planted_copies(zt, cases, info, level):
    case = cases["matrix"]
    stream = zt.deflate_raw(case.data, level=level)
    assert zlib.decompress(stream, -15) == case.data
    cover = token_cover(deflate_audit.parse(stream), len(case.data))
    fails, nmust, nnever, low = stream_check(cover, case.copies, geom(info), "level %d" % level)
    print("level %d: %d copies to cover, least share %.4f; %d copies not to cover" % (level, nmust, low, nnever))
    assert nmust > 300 and nnever > 100
    assert not fails, "\n".join(fails)


def test_dictionary_batch_covers_copies_from_the_dictionary(zt, info):
    g = geom(info)
    d, items, copies = inputs.dictionary_case(g, info["sub"])
    assert len(d) < info["sub"]
    for level in LEVELS:
        streams = zt.deflate_raw_batch(items, level=level, dictionary=d)
        for k, (stream, item, cs) in enumerate(zip(streams, items, copies)):
            o = zlib.decompressobj(-15, zdict=d)
            assert o.decompress(stream) + o.flush() == item
            cover = token_cover(deflate_audit.parse(stream, history=d), len(item))
            fails, nmust, _, low = stream_check(cover, cs, g, "level %d item %d" % (level, k))
            print("dictionary level %d item %d: %d copies, least share %.4f" % (level, k, nmust, low))
            assert nmust == len(cs)
            assert not fails, "\n".join(fails)
