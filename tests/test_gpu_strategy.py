"""The deflate strategies (include/zt_strategy.h) as streams: every new call's
output decodes to its input with Python's zlib / gzip and the oracle inflate,
its tokens obey the strategy (deflate_audit.parse + tests/strategy_ref.py),
and the equalities the header promises hold byte for byte."""
import gzip
import struct
import zlib

import numpy as np
import pytest

import deflate_audit
import lz77_ref
import strategy_ref as sr

pytestmark = pytest.mark.gpu

STRATEGIES = [sr.RLE, sr.HUFFMAN_ONLY]
SIZES = [1, 2, 3, 258, 32767, 32768, 32769, 100000, (1 << 20) + 3]
GENERATORS = ["wordsalad", "structured", "xorshift32", "runs"]
# the size gate (profiles/strategy_gate.txt): worst window of this build's
# bytes over zlib's at the same strategy and level 6, rounded up to the next 0.005
# (recorded worst: RLE 1.01875, Huffman-only 1.01877, both on structured:101)
GATE = {sr.RLE: 1.020, sr.HUFFMAN_ONLY: 1.020}


@pytest.fixture(scope="module")
def zt():
    import ztamd

    return ztamd


@pytest.fixture(scope="module")
def geom(zt):
    _, _, info = zt.debug_match_strategy(b"\0" * 64, sr.RLE)
    return lz77_ref.Geom(info["block"], info["segment"], 0)


@pytest.fixture(scope="module")
def corpus(oracle):
    """generator -> (1 MiB + 3) bytes; a test's input is a prefix."""
    n = max(SIZES)
    c = {k: oracle.gen(k, 31, n) for k in GENERATORS if k != "runs"}
    c["runs"] = sr.run_structured(n, 5).tobytes()
    return c


def gen_bytes(corpus, kind, n):
    return corpus[kind][:n]


def zlib_size(data, strategy):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strategy)
    return len(c.compress(data) + c.flush())


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("kind", GENERATORS)
def test_raw_streams_decode(zt, oracle, corpus, kind, strategy):
    for n in SIZES:
        d = gen_bytes(corpus, kind, n)
        for ctype in (1, 2):
            for level in (1, 6, 9):
                s = zt.deflate_raw(d, compression_type=ctype, level=level, strategy=strategy)
                assert zlib.decompress(s, -15) == d, (n, ctype, level)
                if level == 6:
                    out, ip = oracle.raw_inflate(s)
                    assert out == d and ip == len(s), (n, ctype)
    # compression type NONE and level 0 still write stored blocks
    d = gen_bytes(corpus, kind, 70000)
    assert zt.deflate_raw(d, compression_type=0, strategy=strategy) == zt.deflate_raw(d, compression_type=0)
    assert zt.deflate_raw(d, level=0, strategy=strategy) == zt.deflate_raw(d, level=0)


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_containers_decode_and_trailers(zt, oracle, corpus, strategy):
    for kind in GENERATORS:
        for n in (1, 32769, 300001):
            d = gen_bytes(corpus, kind, n)
            for ctype in (1, 2):
                z, adler = zt.zlib_compress(d, compression_type=ctype, strategy=strategy)
                assert zlib.decompress(z) == d and adler == zlib.adler32(d)
                assert struct.unpack(">I", z[-4:])[0] == zlib.adler32(d)
                assert z[:2] == zt.zlib_compress(d, compression_type=ctype)[0][:2]  # CMF, FLG (FLEVEL) as the plain call's
                out, _ = oracle.zlib_inflate(z, verify=True)
                assert out == d
                g, crc = zt.gzip_compress(d, name=b"a.bin", compression_type=ctype, strategy=strategy)
                assert gzip.decompress(g) == d and crc == zlib.crc32(d)
                assert struct.unpack("<II", g[-8:]) == (zlib.crc32(d), n & 0xFFFFFFFF)
                assert oracle.gunzip(g)[0] == d


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_tokens(zt, corpus, geom, strategy):
    seen = 0
    for kind in GENERATORS:
        d = gen_bytes(corpus, kind, 100000)
        for ctype, level in ((2, 1), (2, 6), (1, 6), (2, 9)):
            s = zt.deflate_raw(d, compression_type=ctype, level=level, strategy=strategy)
            blocks = deflate_audit.parse(s)
            assert deflate_audit.expand_blocks(blocks) == d
            seen += sr.check_tokens(strategy, blocks, d, geom)
    assert (seen > 1000) if strategy == sr.RLE else (seen == 0)


def test_strategy_default_is_the_plain_call(zt, corpus):
    d = gen_bytes(corpus, "wordsalad", 200001)
    for ctype in (1, 2):
        for level in (1, 6):
            assert zt.deflate_raw(d, compression_type=ctype, level=level, strategy=0) == zt.deflate_raw(
                d, compression_type=ctype, level=level)
    assert zt.zlib_compress(d, strategy=0) == zt.zlib_compress(d)
    assert zt.gzip_compress(d, strategy=0) == zt.gzip_compress(d)
    items = [d[:5], d[:40000], b""]
    assert zt.deflate_raw_batch(items, strategy=0) == zt.deflate_raw_batch(items)
    assert zt.zlib_compress_batch(items, strategy=0) == zt.zlib_compress_batch(items)
    assert zt.gzip_compress_batch(items, strategy=0) == zt.gzip_compress_batch(items)
    # and a strategy call leaves nothing behind for the plain call that follows it
    plain = zt.deflate_raw(d)
    zt.deflate_raw(d, strategy=sr.RLE)
    assert zt.deflate_raw(d) == plain


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_levels_1_to_3_write_the_same_stream(zt, corpus, strategy):
    for kind in ("runs", "structured"):
        d = gen_bytes(corpus, kind, 150000)
        for ctype in (1, 2):
            s = [zt.deflate_raw(d, compression_type=ctype, level=lv, strategy=strategy) for lv in (1, 2, 3)]
            assert s[0] == s[1] == s[2]


def test_rle_is_huffman_only_without_adjacent_equal_bytes(zt):
    d = sr.no_repeats(150001, 29).tobytes()
    for ctype in (1, 2):
        for level in (1, 6):
            a = zt.deflate_raw(d, compression_type=ctype, level=level, strategy=sr.RLE)
            b = zt.deflate_raw(d, compression_type=ctype, level=level, strategy=sr.HUFFMAN_ONLY)
            assert a == b and zlib.decompress(a, -15) == d


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_batch_items_are_the_single_calls(zt, geom, strategy):
    # items after the first begin with zeros: packing zero-pads between items,
    # and no match at an item's position 0 may reach into that padding
    sizes = [1, 3, 32767, 32768, 32769, 70000]
    items = []
    for k, n in enumerate(sizes):
        body = sr.run_structured(n, 40 + k).tobytes()
        items.append(body if k == 0 else (b"\0" * min(n, 300) + body)[:n])
    items.insert(3, b"")
    outs = zt.deflate_raw_batch(items, strategy=strategy)
    for d, s in zip(items, outs):
        assert zlib.decompress(s, -15) == d
        assert s == zt.deflate_raw(d, strategy=strategy), len(d)
        blocks = deflate_audit.parse(s)
        toks = sr.token_positions(blocks)
        assert not toks or not isinstance(toks[0][1], tuple)  # position 0 is a literal
        sr.check_tokens(strategy, blocks, d, geom)
    for ctype in (1, 2):
        zs = zt.zlib_compress_batch(items, compression_type=ctype, strategy=strategy)
        gs = zt.gzip_compress_batch(items, compression_type=ctype, strategy=strategy)
        for d, z, g in zip(items, zs, gs):
            assert zlib.decompress(z) == d and gzip.decompress(g) == d
            assert z == zt.zlib_compress(d, compression_type=ctype, strategy=strategy)[0]
            assert g == zt.gzip_compress(d, compression_type=ctype, strategy=strategy)[0]


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_device_plan(zt, geom, strategy):
    import torch

    n = 3 * (1 << 20) + 12345
    host = sr.run_structured(n, 51)
    host[(1 << 20) - 100:(1 << 20) + 100] = 7  # a run across the first restart point and the shard cut
    d = torch.from_numpy(host).cuda()
    o = torch.empty(zt.deflate_bound(n), dtype=torch.uint8, device="cuda")
    p = zt.DeflatePlan(n, strategy=strategy)
    m = p.run(d.data_ptr(), n, o.data_ptr())
    whole = bytes(o[:m].cpu().numpy())
    assert whole == zt.deflate_raw(host.tobytes(), strategy=strategy)
    # two shards, the second with the 32 KiB in front of it as its halo
    cut = 1 << 20
    m0 = p.run(d.data_ptr(), cut, o.data_ptr(), halo=0, final=0)
    first = bytes(o[:m0].cpu().numpy())
    m1 = p.run(d.data_ptr() + cut, n - cut, o.data_ptr(), halo=32768, final=1)
    second = bytes(o[:m1].cpu().numpy())
    s = first + second
    assert zlib.decompress(s, -15) == host.tobytes()
    if strategy == sr.RLE:  # the halo is used: the run goes on across the cut
        toks = sr.token_positions(deflate_audit.parse(second, history=host[cut - 32768:cut].tobytes()))
        assert isinstance(toks[0][1], tuple) and toks[0][1][1] == 1
    # the plan goes back to the search
    p.set_strategy(0)
    m = p.run(d.data_ptr(), n, o.data_ptr())
    assert bytes(o[:m].cpu().numpy()) == zt.deflate_raw(host.tobytes())
    p.close()


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_piece_pipeline(zt, oracle, strategy):
    # 64 MiB and more go through the host pipeline in pieces
    n = (65 << 20)
    unit = oracle.gen("structured", 61, 1 << 20) + sr.run_structured(1 << 20, 62).tobytes()
    d = (unit * (n // len(unit) + 1))[:n]
    s = zt.deflate_raw(d, strategy=strategy)
    assert zlib.decompress(s, -15) == d


@pytest.mark.parametrize("strategy", [1, 4, -1, 7])
def test_invalid_strategy(zt, strategy):
    calls = [
        lambda: zt.deflate_raw(b"abc", strategy=strategy),
        lambda: zt.deflate_raw_batch([b"abc"], strategy=strategy),
        lambda: zt.zlib_compress(b"abc", strategy=strategy),
        lambda: zt.gzip_compress(b"abc", strategy=strategy),
        lambda: zt.zlib_compress_batch([b"abc"], strategy=strategy),
        lambda: zt.gzip_compress_batch([b"abc"], strategy=strategy),
        lambda: zt.DeflatePlan(1000, strategy=strategy),
    ]
    for call in calls:
        with pytest.raises(zt.ZtError) as e:
            call()
        assert e.value.code == -103 and e.value.msg == "invalid strategy: %d" % strategy


def test_strategy_with_dictionary_raises(zt):
    with pytest.raises(ValueError):
        zt.deflate_raw(b"abcabc", dictionary=b"abc", strategy=sr.RLE)
    with pytest.raises(ValueError):
        zt.zlib_compress_batch([b"abcabc"], dictionary=b"abc", strategy=sr.HUFFMAN_ONLY)


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_size_against_zlib(zt, oracle, strategy):
    """One 4 MiB window per generator of the ratio gate's corpus: this build's
    bytes over zlib's at the same strategy, level 6.  Deterministic on both
    sides: the bound is the recorded worst window (profiles/strategy_gate.txt,
    all 16 windows) rounded up to the next 0.005."""
    import ratio_corpus

    wins = ratio_corpus.windows(oracle)
    worst = 0.0
    for kind in ratio_corpus.GENERATORS:
        label, data = next((w[1], w[2]) for w in wins if w[0] == kind)
        ours = len(zt.deflate_raw(data, level=6, strategy=strategy))
        ratio = ours / zlib_size(data, strategy)
        print("strategy %d %s: %d bytes, ratio %.4f" % (strategy, label, ours, ratio))
        worst = max(worst, ratio)
    assert worst <= GATE[strategy], worst
