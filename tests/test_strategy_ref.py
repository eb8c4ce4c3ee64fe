"""strategy_ref against two independent statements of the same thing: the
brute-force LZ77 of lz77_ref restricted to distance 1, and zlib's own Z_RLE.
Also the symbols of include/zt_strategy.h.  No GPU."""
import os
import re
import zlib

import numpy as np
import pytest

import deflate_audit
import lz77_ref
import strategy_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def naive_rle(data, g, halo):
    """longest_naive with a window of one byte: the only candidate is i - 1."""
    g1 = lz77_ref.Geom(g.block, g.segment, 1)
    n = len(data) - halo
    out = np.zeros(n, dtype=np.int64)
    for i in range(n):
        best, dist = lz77_ref.longest_naive(data, i, g1, halo)
        assert dist in (0, 1)
        out[i] = best if best >= 3 else 0
    return out


@pytest.mark.parametrize("block,segment", [(16, 64), (32, 32), (300, 600), (1 << 15, 1 << 20)])
@pytest.mark.parametrize("halo", [0, 1, 5])
def test_rle_lengths_equal_distance_one_lz77(block, segment, halo):
    g = lz77_ref.Geom(block, segment, 0)
    for seed, n in enumerate((1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 200, 700)):
        d = sr.run_structured(halo + n, seed, alphabet=2 + seed % 3, mean=3 + seed % 5)
        for cont in (False, True):  # a run continuing out of the halo, or not
            if halo:
                d[halo - 1] = d[halo] if cont else d[halo] ^ 1
            want = naive_rle(d, g, halo)
            got = sr.rle_lengths(d, g, halo)
            assert np.array_equal(got, want), (n, halo, cont, np.flatnonzero(got != want)[:8])
            w = sr.rle_words(d, g, halo)
            assert np.array_equal(w >> 24, d[halo:])
            assert np.array_equal((w >> 15) & 511, want)
            assert np.array_equal(w & 0x7FFF, (want > 0).astype(np.uint32))


def test_no_repeats_has_no_match_and_equals_huffman_only():
    d = sr.no_repeats(5000, 3)
    assert (d[1:] != d[:-1]).all()
    g = lz77_ref.Geom(1 << 15, 1 << 20, 0)
    assert np.array_equal(sr.rle_words(d, g), sr.huffman_words(d))


def test_matrix_plants_every_length_on_every_offset():
    block = 1 << 15
    d, runs = sr.matrix(block)
    g = lz77_ref.Geom(block, 1 << 20, 0)
    length = sr.rle_lengths(d, g)
    for ln in sr.RUN_LENGTHS:
        starts = {p % 16 for p, k in runs if k == ln}
        assert starts == set(range(16)), ln
        if ln > 1:
            assert any(p // block != (p + ln - 1) // block for p, k in runs if k == ln), ln
            assert any(p // 1024 != (p + ln - 1) // 1024 and p // block == (p + ln - 1) // block
                       for p, k in runs if k == ln), ln
    for p, k in runs:  # a planted run is exactly k long: its second position says so
        if k >= 4 and (p + 1) // block == (p + k - 1) // block:
            assert length[p + 1] == min(k - 1, 258), (p, k)
        assert length[p] == 0


@pytest.mark.parametrize("seed", range(6))
def test_zlib_rle_tokens_are_the_definition(seed):
    # zlib's deflate_rle emits, where it emits a match, the whole run at distance
    # 1 up to 258: L(p) without the block cap (zlib's blocks are not this engine's)
    d = sr.run_structured(60000, 100 + seed, alphabet=3 + seed, mean=4 + seed)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
    stream = c.compress(d.tobytes()) + c.flush()
    blocks = deflate_audit.parse(stream)
    assert deflate_audit.expand_blocks(blocks) == d.tobytes()
    g = lz77_ref.Geom(1 << 30, 1 << 30, 0)
    length = sr.rle_lengths(d, g)
    matches = 0
    for p, t in sr.token_positions(blocks):
        if isinstance(t, tuple):
            matches += 1
            assert (t[0], t[1]) == (length[p], 1), (p, t, length[p])
    assert matches > 100
    assert sr.check_tokens(sr.RLE, blocks, d, g) == matches


def test_huffman_only_zlib_stream_has_no_match():
    d = sr.run_structured(20000, 9)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
    blocks = deflate_audit.parse(c.compress(d.tobytes()) + c.flush())
    assert sr.check_tokens(sr.HUFFMAN_ONLY, blocks, d, lz77_ref.Geom(1 << 15, 1 << 20, 0)) == 0


def test_strategy_constants_are_zlibs():
    import ztamd

    assert (ztamd.STRATEGY_DEFAULT, ztamd.STRATEGY_HUFFMAN_ONLY, ztamd.STRATEGY_RLE) == (
        zlib.Z_DEFAULT_STRATEGY, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)
    assert (sr.HUFFMAN_ONLY, sr.RLE) == (zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)


def test_header_symbols_are_exported_and_bound():
    import ztamd

    text = open(os.path.join(ROOT, "include", "zt_strategy.h")).read()
    declared = sorted(set(re.findall(r"^int (zt_\w+)\(", text, flags=re.M)))
    assert declared == sorted(ztamd.STRATEGY_SYMBOLS)
    for name in declared + ["zt_debug_match_strategy"]:
        f = getattr(ztamd.lib, name, None)
        assert f is not None and f.argtypes is not None, name


def test_python_strategy_with_dictionary_raises():
    import ztamd

    for call in (ztamd.deflate_raw, ztamd.zlib_compress):
        with pytest.raises(ValueError):
            call(b"abc", dictionary=b"abc", strategy=ztamd.STRATEGY_RLE)
    for call in (ztamd.deflate_raw_batch, ztamd.zlib_compress_batch):
        with pytest.raises(ValueError):
            call([b"abc"], dictionary=b"abc", strategy=ztamd.STRATEGY_RLE)
