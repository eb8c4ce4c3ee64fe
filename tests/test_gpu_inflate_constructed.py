"""Hand-built DEFLATE streams (tests/deflate_builder.py) on every decode path.

Encoders never write most of what RFC 1951 allows; these streams do: 48-bit
tokens, 15-bit codes, header minima, thousands of empty blocks, matches at
the edge of the output produced, malformed headers.  Every valid case goes
through one wave, strict, the two-phase batch, the sync-point path
(`framed`), the general path (`long`), the device plan, resume and -- for
its own streams -- the preset dictionary, with the `inflate_paths` counters
as evidence of the path.  Rules:

* valid per zlib: every path gives zlib's output (= `expand` of the tokens
  written) and zlib's end position;
* invalid per zlib: every path gives the status of the one-wave decode of
  the same stream; that status is non-zero, or the case's kind is in
  ACCEPTED_INVALID and every path's output equals the reference fixture's
  (tests/golden/inflate_constructed.json);
* strict: output, `.ip` and error text equal the fixture's, but for the
  engine-only rejections (statuses -15, -16, -17);
* truncation: never status 0 with a wrong output; through resume "needs
  more" while more may come, an error once it cannot.
"""
import hashlib
import random

import pytest

import deflate_builder as B

pytestmark = pytest.mark.gpu

# Malformed headers the engine decodes as the reference does (DESIGN.md
# section 2 has the same list): kinds of tests/deflate_builder.py's cases.
ACCEPTED_INVALID = {
    "first16": "repeat-previous as the first code-length symbol repeats length 0",
    "run_overflow": "run lengths past HLIT + HDIST are dropped",
    "hlit_over_286": "HLIT = 287 / 288 with length 0 for symbols 286 and 287 (a code for either: ZT_E_BAD_TREE)",
}
# `framed` / `long` cases that leave their parallel path for one wave, with the
# library's own reason (ZT_INF_DEBUG=1).  No D case may be listed.
BY_DESIGN_FALLBACK = {
    # a unit's token slot is bounded by the input up to the next sync candidate;
    # the candidates inside the stored payload make unit 0's too small for it
    "c2_false_sync_framed": "[zt inflate] unit 0 (chain 0): status -102 detail 0 ntok 1 out 1",
    # a sync-point unit holds at most 32 KiB + 64 tokens (the blocks this engine's
    # deflate writes); the 65535-byte stored block is more
    "c2_len_framed": "[zt inflate] unit 1 (chain 1): status -102 detail 0 ntok 1 out 1",
    # a restart marker starts an independent segment; a match that reaches
    # behind it is found while resolving (zt_inflate_raw once answered such a
    # stream with ZT_E_ARG: the general path was handed the abandoned output)
    "c4_restart_framed": "[zt inflate] unit 2 of 147 (chain): status -15",
}
ENGINE_ONLY = {-15, -16, -17}  # ZT_E_INVALID_DISTANCE, ZT_E_INVALID_SYMBOL, ZT_E_BAD_TREE

VALID = [c.name for c in B.CASES.values() if c.cls == "valid"]
INVALID = [c.name for c in B.CASES.values() if c.cls == "invalid"]
SHORT = [n for n in VALID if B.CASES[n].variant == "short"]
FRAMED = [n for n in VALID if B.CASES[n].variant == "framed"]
LONG = [n for n in VALID if B.CASES[n].variant == "long"]


@pytest.fixture(scope="module")
def zt():
    import ztamd

    assert ztamd.device_count() > 0, "no GPU visible"
    return ztamd


@pytest.fixture(scope="module")
def ref():
    return B.reference_records()


_want = {}


def want(name):
    """(zlib's output, zlib's consumed count) of a valid case; the output is
    expand(tokens) too."""
    if name not in _want:
        c = B.CASES[name]
        out, used = B.zlib_inflate(c.stream)
        assert out == c.expected
        _want[name] = (out, used)
    return _want[name]


def counters(zt):
    t = zt.timing_read()
    return list(t["inflate_paths"]), t["inflate_toks"]


def delta(zt, before):
    p, toks = counters(zt)
    return [a - b for a, b in zip(p, before[0])], toks - before[1]


def run(fn):
    """(status, output, end position) of a call that raises ZtError."""
    import ztamd

    try:
        out, ip = fn()
    except ztamd.ZtError as e:
        return e.code, None, None
    return 0, out, ip


def plan_run(zt, stream, cap, offset):
    """InflatePlan.run on device input at pointer offset `offset`; the output stays on the device."""
    import numpy as np
    import torch
    import ztamd

    d_in = torch.zeros(len(stream) + offset + 64, dtype=torch.uint8, device="cuda")
    d_in[offset:offset + len(stream)] = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    plan = zt.InflatePlan(len(stream), cap)
    try:
        olen, ip = plan.run(d_in.data_ptr() + offset, len(stream), d_out.data_ptr(), cap)
    except ztamd.ZtError as e:
        return e.code, None, None
    finally:
        plan.close()
    torch.cuda.synchronize()
    return 0, d_out[:olen], ip


def feed(zt, stream, pieces):
    """RawInflateStream fed the prefixes ending at `pieces`, then finished."""
    st = zt.RawInflateStream()
    out = []
    for k in pieces:
        out.append(st.decompress(stream[:k]))
    out.append(st.finish(stream))
    return b"".join(out), st.ip + (1 if st.bit else 0)


# ---- valid cases --------------------------------------------------------------
@pytest.mark.parametrize("name", VALID)
def test_one_wave(zt, name):
    c = B.CASES[name]
    out, used = want(name)
    b = counters(zt)
    (got,) = zt.inflate_raw_batch([c.stream])
    assert got[0] == 0 and got[1] == out and got[2] == used
    assert delta(zt, b)[0][2] == 1
    if c.variant == "short":
        b = counters(zt)
        assert zt.inflate_raw(c.stream) == (out, used)
        assert delta(zt, b)[0] == [0, 0, 1]


@pytest.mark.parametrize("name", list(B.CASES))
def test_strict(zt, ref, name):
    """ref_strict against the reference itself: output, .ip, error text."""
    import ztamd

    r = ref[name]
    b = counters(zt)
    try:
        out, ip = zt.inflate_raw(B.CASES[name].stream, ref_strict=True)
        err = None
    except ztamd.ZtError as e:
        err = e
    assert delta(zt, b)[0] == [0, 0, 1]
    if err is not None and err.code in ENGINE_ONLY:
        assert B.CASES[name].cls == "invalid"   # what zlib rejects too, and only that
        return
    assert r.get("reference") != "no result"
    if "error" in r:
        assert err is not None and err.msg == r["error"]
    else:
        assert err is None
        assert len(out) == r["out"]["len"] and hashlib.sha256(out).hexdigest() == r["out"]["sha256"]
        assert ip == r["ip"]


def test_batch_two_phase(zt):
    """All valid cases in one batch, in a fixed shuffled order."""
    names = list(VALID)
    random.Random(5).shuffle(names)
    assert len(names) >= 8
    b = counters(zt)
    res = zt.inflate_raw_batch([B.CASES[n].stream for n in names])
    left = delta(zt, b)[0][2]
    for n, (st, out, ip) in zip(names, res):
        assert st == 0 and (out, ip) == want(n), n
    assert left < len(names)
    # which ones the two-phase pass leaves to one wave: eight copies of a case
    # at a time (the cases with the largest outputs are not probed)
    stay = []
    for n in names:
        if len(want(n)[0]) > (1 << 20):
            continue
        b = counters(zt)
        res = zt.inflate_raw_batch([B.CASES[n].stream] * 8)
        assert all(st == 0 and (out, ip) == want(n) for st, out, ip in res), n
        if delta(zt, b)[0][2]:
            stay.append(n)
    print("two-phase batch left %d of %d streams to one wave; alone in a batch of 8: %s" % (left, len(names), stay))


@pytest.mark.parametrize("name", FRAMED)
def test_sync_point_path(zt, name):
    zt.timing_enable(True)   # (inflate_toks counts timed tokenize passes)
    try:
        b = counters(zt)
        assert zt.inflate_raw(B.CASES[name].stream) == want(name)
        paths, toks = delta(zt, b)
    finally:
        zt.timing_enable(False)
    if name in BY_DESIGN_FALLBACK:
        assert paths == [0, 1, 0]   # the general path takes it
    else:
        assert paths == [1, 0, 0] and toks == 1


@pytest.mark.parametrize("name", LONG)
def test_general_path(zt, name):
    b = counters(zt)
    assert zt.inflate_raw(B.CASES[name].stream) == want(name)
    paths, _ = delta(zt, b)
    if name in BY_DESIGN_FALLBACK:
        assert paths[1] == 0
    else:
        assert paths[1] == 1 and paths[2] == 0


def test_fallback_list_is_closed():
    for n in BY_DESIGN_FALLBACK:
        assert n in FRAMED + LONG and not B.CASES[n].group.startswith("d"), n


@pytest.mark.parametrize("name", FRAMED + LONG)
def test_device_plan(zt, name):
    import numpy as np
    import torch

    out, used = want(name)
    d_want = torch.from_numpy(np.frombuffer(out, dtype=np.uint8).copy()).cuda() if out else None
    for offset in (0, 3):
        st, d_out, ip = plan_run(zt, B.CASES[name].stream, len(out) + 64, offset)
        assert st == 0 and ip == used and d_out.numel() == len(out)
        assert d_want is None or torch.equal(d_out, d_want)


@pytest.mark.parametrize("name", VALID)
def test_resume(zt, name):
    c = B.CASES[name]
    out, used = want(name)
    n = len(c.stream)
    strides = [1] if c.variant == "short" else [1021, 4093]
    assert c.variant != "short" or n <= 4096
    for step in strides:
        got, end = feed(zt, c.stream, range(step, n, step))
        assert got == out and end == used


@pytest.mark.parametrize("k", range(1, 17))
def test_index_alignments(zt, k):
    """`index` > 0 at each of 16 input alignments, on each decode path."""
    pre = bytes(range(1, k + 1))
    for name, path in (("a2_short", 2), ("a2_framed", 0), ("a2_long", 1), ("c4_long", 1)):
        out, used = want(name)
        b = counters(zt)
        assert zt.inflate_raw(pre + B.CASES[name].stream, index=k) == (out, k + used)
        assert delta(zt, b)[0][path] == 1


@pytest.mark.parametrize("dlen", [1, 4097, 32768])
def test_dictionary(zt, dlen):
    """First tokens reaching 1, len(dict) and len(dict) + 1 bytes back into a
    preset dictionary (32769 cannot be written), single and batch."""
    import zlib

    d = random.Random(dlen).randbytes(dlen)
    for dist in (1, dlen, dlen + 1):
        if dist > 32768:
            continue
        s = B.dict_stream(dist)
        stream = s.getvalue()
        if dist <= dlen:
            out, used = B.zlib_inflate(stream, zdict=d)
            assert out == B.expand(s.tokens, history=d)
            assert zt.inflate_raw(stream, dictionary=d) == (out, used)
            for st, o, ip in zt.inflate_raw_batch([stream] * 9, dictionary=d):
                assert st == 0 and o == out and ip == used
        else:
            with pytest.raises(zlib.error):
                B.zlib_inflate(stream, zdict=d)
            assert run(lambda: zt.inflate_raw(stream, dictionary=d))[0] == -15
            assert [st for st, _, _ in zt.inflate_raw_batch([stream] * 9, dictionary=d)] == [-15] * 9


# ---- C6: truncation -------------------------------------------------------------
@pytest.mark.parametrize("name", SHORT)
def test_truncation(zt, name):
    """The short variants cut at every byte."""
    import ztamd

    c = B.CASES[name]
    out, used = want(name)
    cuts = [c.stream[:k] for k in range(used)]
    for k, (st, o, ip) in enumerate(zt.inflate_raw_batch(cuts)):
        assert st != 0 or o == out, k                 # never status 0 with a wrong output
    for k, (st, o, ip) in enumerate(zt.inflate_raw_batch(cuts[-4:])):   # (fewer than 8: one wave)
        assert st != 0 or o == out, k
    for k in range(used):
        s = zt.RawInflateStream()
        part = s.decompress(cuts[k])                  # more may come: no error
        assert out.startswith(part) and not s.bfinal
        with pytest.raises(ztamd.ZtError):
            zt.RawInflateStream(cuts[k]).finish()     # nothing more comes: an error


@pytest.mark.parametrize("name", ["a1_long", "a2_framed", "c3_long", "d3_density_long"])
def test_truncation_long(zt, name):
    c = B.CASES[name]
    out, used = want(name)
    for k in (used - 1, used - 2, used // 2, 16384, 16385):
        for st, o, ip in (run(lambda: zt.inflate_raw(c.stream[:k])), zt.inflate_raw_batch([c.stream[:k]])[0]):
            assert st != 0, k


# ---- invalid cases ----------------------------------------------------------------
@pytest.mark.parametrize("name", INVALID)
def test_invalid_same_status_on_every_path(zt, ref, name):
    import ztamd

    c = B.CASES[name]
    s = c.stream
    st0, out0, ip0 = zt.inflate_raw_batch([s])[0]      # one wave: the yardstick
    got = {"auto": run(lambda: zt.inflate_raw(s))}
    for i, r in enumerate(zt.inflate_raw_batch([s] * 8)):
        got["batch%d" % i] = r
    cap = (ref[name].get("out", {}).get("len", 0)) + (1 << 20)
    for offset in (0, 3):
        st, d_out, ip = plan_run(zt, s, cap, offset)
        got["plan%d" % offset] = (st, None if st else d_out.cpu().numpy().tobytes(), ip)
    try:
        o = zt.RawInflateStream(s)
        data = o.finish()
        got["resume"] = (0, data, o.ip + (1 if o.bit else 0))
    except ztamd.ZtError as e:
        got["resume"] = (e.code, None, None)
    for path, (st, out, ip) in got.items():
        assert st == st0, (path, st, st0)
    if st0 == 0:
        assert c.kind in ACCEPTED_INVALID, "decoded what zlib rejects"
        r = ref[name]
        for path, (st, out, ip) in [("one wave", (st0, out0, ip0))] + list(got.items()):
            assert len(out) == r["out"]["len"] and hashlib.sha256(out).hexdigest() == r["out"]["sha256"], path
            assert ip == r["ip"], path
