"""The block parser (tests/deflate_audit.py) on streams other encoders wrote:
zlib's, stored ones and the hand-built catalogue, whose tokens are known."""
import zlib

import pytest

import deflate_audit as da
import deflate_builder as db
from audit_inputs import dense_input, oracle_input

VALID = sorted(n for n, c in db.CASES.items() if c.cls == "valid")
BAD_CODES = ["a7_incomplete_cl", "a7_incomplete_lit", "a7_incomplete_dist", "a7_over_cl", "a7_over_lit",
             "a7_over_dist"]


def zlib_raw(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def check_blocks(blocks, data, history=b""):
    tokens = [t for b in blocks for t in b.tokens]
    assert db.expand(tokens, history) == data
    assert da.expand_blocks(blocks) == data
    assert blocks[-1].final and not any(b.final for b in blocks[:-1])
    pos = 0
    for b in blocks:
        assert b.bit_start == pos and b.bit_end > b.bit_start
        pos = b.bit_end
        if b.btype == 0:
            assert b.stored_len == len(b.out)
            continue
        # the histograms are those of the tokens, end-of-block included
        lit, dist = [0] * 286, [0] * 30
        lit[256] = 1
        for t in b.tokens:
            if isinstance(t, int):
                lit[t] += 1
            else:
                lit[db.len_symbol(t[0], len(t) > 2)[0]] += 1
                dist[db.dist_symbol(t[1])[0]] += 1
        assert (lit, dist) == (b.lit_hist, b.dist_hist)
        if b.btype == 2:
            assert len(b.lit_lens) == b.hlit and len(b.dist_lens) == b.hdist
            assert sum(b.cl_hist) == len(b.cl_syms)
            # the code-length symbols as read expand to the lengths
            lens = []
            for s, x in b.cl_syms:
                lens += [s] if s < 16 else [lens[-1] if s == 16 else 0] * (db.CL_REP0[s] + x)
            assert lens == b.lit_lens + b.dist_lens


@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("name", ["dense", "wordsalad", "structured"])
def test_zlib_streams(name, level):
    data = dense_input() if name == "dense" else oracle_input(name)
    blocks = da.parse(zlib_raw(data, level))
    assert any(b.btype == 2 for b in blocks)
    check_blocks(blocks, data)


def test_zlib_fixed_stream():
    data = oracle_input("wordsalad")[:40000]
    blocks = da.parse(zlib_raw(data, 6, zlib.Z_FIXED))
    assert {b.btype for b in blocks} == {1}
    check_blocks(blocks, data)
    assert blocks[0].lit_lens == db.FIXED_LIT and blocks[0].header_bits == 3


def test_zlib_history():
    """A stream written with a preset dictionary: distances reach into it."""
    data = oracle_input("wordsalad")
    hist, body = data[:5000], data[3000:9000]
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, hist)
    stream = c.compress(body) + c.flush()
    check_blocks(da.parse(stream, hist), body, hist)
    with pytest.raises(da.AuditError):
        da.parse(stream)


def test_stored_streams():
    data = dense_input()
    blocks = da.parse(zlib_raw(data, 0))
    assert {b.btype for b in blocks} == {0} and sum(b.stored_len for b in blocks) == len(data)
    check_blocks(blocks, data)
    s = db.Stream()
    s.stored(b"", False)
    s.stored(b"abc", False, pad_bits=0x55)
    s.stored(bytes(65535), True)
    blocks = da.parse(s.getvalue() + b"trailing")
    assert [b.stored_len for b in blocks] == [0, 3, 65535]
    assert blocks[-1].bit_end == 8 * s.nbytes
    check_blocks(blocks, b"abc" + bytes(65535))


@pytest.mark.parametrize("name", VALID)
def test_builder_streams(name):
    case = db.CASES[name]
    blocks = da.parse(case.stream, case.s.history)
    assert [tuple(t[:2]) if not isinstance(t, int) else t for b in blocks for t in b.tokens] == \
        [tuple(t[:2]) if not isinstance(t, int) else t for t in case.tokens]
    check_blocks(blocks, case.expected, case.s.history)
    assert [b.btype for b in blocks] == case.s.block_types
    dyn = [b for b in blocks if b.btype == 2]
    assert len(dyn) == len(case.s.headers)
    for b, h in zip(dyn, case.s.headers):
        assert (b.hlit, b.hdist, b.hclen, b.cl_lens) == (h["hlit"], h["hdist"], h["hclen"], h["cl_lens"])
        assert db.cl_runs(b.cl_syms) == h["runs"]


def test_length_258_both_ways():
    blocks = da.parse(db.CASES["b1_short"].stream)
    t258 = [t for b in blocks for t in b.tokens if not isinstance(t, int) and t[0] == 258]
    assert any(len(t) == 3 for t in t258) and any(len(t) == 2 for t in t258)


@pytest.mark.parametrize("variant", ["short", "long"])  # the bad block first, or after valid ones
@pytest.mark.parametrize("name", BAD_CODES)
def test_bad_codes_raise(name, variant):
    case = db.CASES[name + "_" + variant]
    assert case.cls == "invalid"
    with pytest.raises(da.AuditError, match="over-subscribed|incomplete"):
        da.parse(case.stream)


def test_other_malformed_streams_raise():
    for name in ("a7_first16_short", "a7_overflow_short", "a7_no_eob_short", "a3_code1_short", "a4_length_short",
                 "b4_first_short_over"):
        with pytest.raises(da.AuditError):
            da.parse(db.CASES[name].stream)
    with pytest.raises(da.AuditError):
        da.parse(zlib_raw(b"hello hello hello", 6)[:-2])
