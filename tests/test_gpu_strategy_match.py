"""The strategies' producer of res held to its definition, word for word.

ztamd.debug_match_strategy returns what strategy_kernel
(csrc/deflate_strategy.hip) wrote over a result buffer filled with 0xFFFFFFFF,
launched as the strategy calls launch it.  Unlike the hash chains' result it is
a function of the input alone, so every one of the n words must equal
tests/strategy_ref.py's, and none may be left unwritten.  Every constant comes
from the library's record (info)."""
import os

import numpy as np
import pytest

import lz77_ref
import strategy_ref as sr

pytestmark = pytest.mark.gpu

UNWRITTEN = 0xFFFFFFFF


@pytest.fixture(scope="module")
def zt():
    import ztamd

    return ztamd


@pytest.fixture(scope="module")
def geom(zt):
    _, _, info = zt.debug_match_strategy(b"\0" * 64, sr.RLE)
    return lz77_ref.Geom(info["block"], info["segment"], 0)


def check(zt, strategy, data, g, halo=0, level=6):
    d = np.asarray(data, dtype=np.uint8)
    res, _, info = zt.debug_match_strategy(d.tobytes(), strategy, level=level, halo=halo)
    assert (info["block"], info["segment"]) == (g.block, g.segment)
    assert res.size == d.size - halo
    assert not (res == UNWRITTEN).any(), np.flatnonzero(res == UNWRITTEN)[:8]
    want = sr.words(strategy, d, g, halo)
    bad = np.flatnonzero(res != want)
    assert bad.size == 0, [(int(i), hex(int(res[i])), hex(int(want[i]))) for i in bad[:8]]
    return res


def test_matrix_rle_and_huffman_only(zt, geom):
    d, runs = sr.matrix(geom.block)
    res = check(zt, sr.RLE, d, geom)
    assert ((res >> 15) & 511).max() == 258
    res = check(zt, sr.HUFFMAN_ONLY, d, geom)
    assert np.array_equal(res, d.astype(np.uint32) << 24)


@pytest.mark.parametrize("level", [1, 9])
def test_level_and_search_hooks_do_not_reach_the_kernel(zt, geom, level):
    d, _ = sr.matrix(geom.block, seed=8)
    d = d[:3 * geom.block + 777]
    hooks = {"ZT_DF_PARAMS": "4,16,0,16,4,2", "ZT_DF_ADAPT": "2,1", "ZT_DF_MQ": "1", "ZT_DF_HEADS": "16"}
    old = {k: os.environ.get(k) for k in hooks}
    os.environ.update(hooks)
    try:
        check(zt, sr.RLE, d, geom, level=level)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def test_runs_straddle_the_segment_start(zt, geom):
    # no match at S (its segment starts there), matches resume at S + 1
    S = geom.segment
    base = sr.no_repeats(S + 8192, 11)
    for ln in sr.RUN_LENGTHS:
        for j in sr.straddles(ln):
            d = base.copy()
            before, after = int(d[S - j - 1]), int(d[S - j + ln])
            d[S - j:S - j + ln] = next(x for x in range(256) if x not in (before, after))
            res = check(zt, sr.RLE, d, geom)
            assert (res[S] >> 15) & 511 == 0
            if ln - j >= 4:
                assert (res[S + 1] >> 15) & 511 == min(ln - j - 1, 258)


def test_ragged_ends(zt, geom):
    B = geom.block
    for n in (1, 2, 3, 4, 15, 16, 17, B - 1, B, B + 1):
        for ln in sr.RUN_LENGTHS:
            d = sr.no_repeats(n, 13 + ln)
            k = min(ln, n)  # the run runs into the end of the data
            d[n - k:] = next(x for x in range(256) if n - k == 0 or x != int(d[n - k - 1]))
            for strategy in (sr.RLE, sr.HUFFMAN_ONLY):
                check(zt, strategy, d, geom)


def test_all_equal_three_blocks(zt, geom):
    d = np.full(3 * geom.block, 0x5A, dtype=np.uint8)
    res = check(zt, sr.RLE, d, geom)
    length = (res >> 15) & 511
    assert length[0] == 0 and length[1] == 258 and length[geom.block] == 258
    assert length[geom.block - 2] == 0 and length[geom.block - 3] == 3


def test_no_adjacent_equal_bytes_rle_is_huffman_only(zt, geom):
    d = sr.no_repeats(2 * geom.block + 4097, 17)
    a = check(zt, sr.RLE, d, geom)
    b = check(zt, sr.HUFFMAN_ONLY, d, geom)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("halo", [1, 2, 32768])
def test_run_continues_out_of_the_halo(zt, geom, halo):
    n = geom.block + 5000
    for back, fwd in ((1, 1), (1, 5), (2, 300), (halo, 2), (min(halo, 400), 259)):
        back = min(back, halo)
        d = sr.no_repeats(halo + n, 19 + fwd)
        lo, hi = halo - back, halo + fwd
        before = int(d[lo - 1]) if lo else -1
        d[lo:hi] = next(x for x in range(256) if x not in (before, int(d[hi])))
        res = check(zt, sr.RLE, d, geom, halo=halo)
        assert (res[0] >> 15) & 511 == (min(fwd, 258) if fwd >= 3 else 0)
        check(zt, sr.HUFFMAN_ONLY, d, geom, halo=halo)
    # and a halo the stream's first byte does not continue
    d = sr.no_repeats(halo + n, 23)
    check(zt, sr.RLE, d, geom, halo=halo)


@pytest.mark.parametrize("strategy", [1, 4, -1, 7])
def test_debug_refuses_other_strategies(zt, strategy):
    with pytest.raises(zt.ZtError) as e:
        zt.debug_match_strategy(b"abcd", strategy)
    assert e.value.code == -103 and "invalid strategy: %d" % strategy in str(e.value)
