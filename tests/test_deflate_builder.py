"""The hand-built DEFLATE catalogue (tests/deflate_builder.py) checked on the
CPU: the writer against zlib and against `expand`, the catalogue against what
each case was built for, the oracle against the reference fixture
(tests/golden/inflate_constructed.json), and the table of malformed cases
with zlib's and the reference's verdict -- what DESIGN.md section 2's
accepted-invalid list is applied to."""
import hashlib
import os
import zlib

import pytest

import deflate_builder as B

VALID = [c.name for c in B.CASES.values() if c.cls == "valid"]
INVALID = [c.name for c in B.CASES.values() if c.cls == "invalid"]


@pytest.fixture(scope="module")
def ref():
    return B.reference_records()


def test_bitwriter():
    w = B.BitWriter()
    w.bits(0b101, 3)      # LSB first
    w.code(0b110, 3)      # MSB first: written as 0 1 1
    w.align(0xFF)
    assert w.getvalue() == bytes([0b11011101])
    w.bits(0x1234, 16)
    assert w.getvalue() == bytes([0b11011101, 0x34, 0x12]) and w.bitpos == 24


def test_expand_overlap_and_history():
    assert B.expand([97, 98, (5, 2), (3, 7)]) == b"abababaaba"
    assert B.expand([(4, 3), 120, (2, 1)], history=b"xyz") == b"xyzxxxx"
    with pytest.raises(ValueError):
        B.expand([97, (3, 2)])


def test_symbol_tables():
    for length in range(3, 259):
        s, xb, xv = B.len_symbol(length)
        assert B.LEN_BASE[s - 257] + xv == length and xv < (1 << xb) and xb == B.LEN_EXTRA[s - 257]
    assert B.len_symbol(258) == (285, 0, 0) and B.len_symbol(258, True) == (284, 5, 31)
    for dist in list(range(1, 600)) + [4096, 4097, 24576, 24577, 32768]:
        s, xb, xv = B.dist_symbol(dist)
        assert B.DIST_BASE[s] + xv == dist and xv < (1 << xb) and xb == B.DIST_EXTRA[s]
    assert B.kraft(B.FIXED_LIT) == 32768 and B.canonical_codes(B.FIXED_LIT)[286] == 0xC6


@pytest.mark.parametrize("name", VALID)
def test_builder_vs_zlib_and_expand(name):
    """zlib decodes every valid case to expand(tokens), to the end, and
    consumes the stream without its trailing bytes."""
    c = B.CASES[name]
    out, used = B.zlib_inflate(c.stream)
    assert out == c.expected
    assert used == len(c.stream) - len(c.trailing)


@pytest.mark.parametrize("name", INVALID)
def test_invalid_cases_are_invalid_for_zlib(name):
    with pytest.raises(zlib.error):
        B.zlib_inflate(B.CASES[name].stream)


def test_variants_and_sizes():
    groups = {}
    for c in B.CASES.values():
        groups.setdefault((c.group, c.cls), set()).add(c.variant)
        n = len(c.stream)
        if c.variant == "short":
            assert n < 2048 or c.group.startswith("c2_false"), c.name   # (the payload of false candidates is 3.5 KiB)
        else:
            assert 16384 + 16 <= n <= 70000, c.name
    for (g, cls), v in groups.items():
        if g[0] == "d":
            assert "short" not in v
        else:
            assert v & {"framed", "long"}, g
            assert "short" in v or g == "c2_len", g
    # a `long` case holds no sync marker, a `framed` one does
    for c in B.CASES.values():
        has = b"\x00\x00\xff\xff" in c.stream[: len(c.stream) - len(c.trailing)]
        if c.variant == "long":
            assert not has, c.name
        if c.variant == "framed":
            assert has, c.name


def _st(name):
    return B.CASES[name].stats


def test_catalogue_intent_code_tables():
    for n in ("a1_short", "a1_framed", "a1_long", "d1_chain_long", "d4_resync_long"):
        st = _st(n)
        assert st["widest"] == 48, n                       # 15 + 5 + 15 + 13
        assert 15 in st["lit_code_lens"] and 15 in st["dist_code_lens"]
        assert {284} <= set(st["len_syms"]) and {28, 29} & set(st["dist_syms"])
    for n in ("a2_short", "a2_framed", "a2_long"):
        st = _st(n)
        assert set(B.A2_LIT) - {0} == set(range(1, 16)) and set(B.A2_DIST) - {0} == set(range(1, 16))
        assert {8, 9, 15} <= set(st["lit_code_lens"]) and {8, 9, 15} <= set(st["dist_code_lens"])
        assert st["allones15"] == [True, True]             # lim[15] == 1 << 32 is reached
    s = B.CASES["a2_long"].s
    assert set(range(1, 16)) <= s.lit_code_lens and set(range(1, 16)) <= s.dist_code_lens
    assert _st("a3_short")["dist_code_lens"] == [1] and _st("a3_short")["dist_syms"] == [0]
    assert _st("a4_short")["dist_syms"] == [] and B.CASES["a4_short"].s.headers[0]["hdist"] == 1
    h = B.CASES["a5_short"].s.headers
    assert h[0]["hlit"] == 257 and h[0]["hclen"] == 5 and sorted(set(h[0]["cl_lens"])) == [0, 1]
    assert {s for _, s, _ in h[0]["runs"]} == {0, 8}
    assert h[1]["hclen"] == 19 and max(h[1]["cl_lens"]) == 7 and h[1]["cl_lens"][1] == 7
    assert any(s == 1 for _, s, _ in h[1]["runs"])         # a 7-bit code-length code is used


def test_catalogue_intent_run_lengths():
    h = B.CASES["a6_short"].s.headers
    runs = [r for x in h for r in x["runs"]]
    # a 16-run from the lit/len lengths into the distance lengths
    assert any(s == 16 and i < h[0]["hlit"] < i + rep for i, s, rep in h[0]["runs"])
    # an 18-run and a 17-run ending exactly at HLIT + HDIST
    for sym, k in ((18, 1), (17, 2)):
        i, s, rep = h[k]["runs"][-1]
        assert s == sym and i + rep == h[k]["hlit"] + h[k]["hdist"]
    assert (18, 138) in {(s, rep) for _, s, rep in runs} and (16, 6) in {(s, rep) for _, s, rep in runs}
    assert {x["first"] for x in h} >= {17, 18}


def test_catalogue_intent_malformed_headers():
    s = B.CASES["a7_first16_short"].s
    assert s.headers[0]["first"] == 16
    s = B.CASES["a7_overflow_short"].s
    i, sym, rep = s.headers[0]["runs"][-1]
    assert i + rep > s.headers[0]["hlit"] + s.headers[0]["hdist"]
    assert B.CASES["a7_hlit287_short"].s.headers[0]["hlit"] == 287
    assert B.CASES["a7_hlit288_short"].s.headers[0]["hlit"] == 288
    assert B.CASES["a7_hlit288z_short"].s.headers[0]["hlit"] == 288
    for n in ("a7_hlit287_short", "a7_hlit288_short", "a7_hlit288z_short"):
        assert not set(B.CASES[n].s.len_syms) & {286, 287}
    assert B.kraft(B.CASES["a7_incomplete_cl_short"].s.headers[0]["cl_lens"]) < 32768
    assert B.kraft(B.CASES["a7_over_cl_short"].s.headers[0]["cl_lens"]) > 32768


def test_catalogue_intent_tokens():
    toks = [t for t in B.CASES["b1_short"].tokens if not isinstance(t, int)]
    assert {t[0] for t in toks} == set(range(3, 259))
    assert set(range(257, 286)) <= set(_st("b1_short")["len_syms"])
    bits = B.CASES["b1_short"].s
    assert 284 in bits.len_syms and 285 in bits.len_syms
    assert sum(1 for t in toks if t[0] == 258) >= 2        # symbol 285, and symbol 284 with extra bits 31
    assert _st("b2_short")["dist_syms"] == list(range(30))
    d2 = {t[1] for t in B.CASES["b2_short"].tokens if not isinstance(t, int)}
    for ds in range(30):
        assert {B.DIST_BASE[ds], B.DIST_BASE[ds] + (1 << B.DIST_EXTRA[ds]) - 1} <= d2
    assert 32768 in d2
    pairs = {(t[1], t[0]) for t in B.CASES["b3_short"].tokens if not isinstance(t, int)}
    for D in B.B3_D:
        for L in (3, D - 1, D, D + 1, 258):
            assert L < 3 or (D, L) in pairs
    for n, c in B.CASES.items():
        if c.group == "b4" and c.cls == "valid":
            seen = 0
            for t in c.tokens[:-2]:
                seen += 1 if isinstance(t, int) else t[0]
            assert c.tokens[-2][1] == min(seen, 32768), n
    assert B.CASES["b4_far_long_eq"].tokens[-2][1] == 32768 and len(B.CASES["b4_far_long_eq"].expected) > 40000


def test_catalogue_intent_blocks():
    assert _st("c1_fixed_short")["phases"] == list(range(8)) and _st("c1_fixed_short")["nblocks"] == 100
    assert B.CASES["c1_fixed_short"].s.block_types.count(1) == 99
    assert _st("c1_fixed_long")["nblocks"] >= 14000 and B.CASES["c1_fixed_long"].expected == b""
    assert _st("c1_dynamic_long")["block_types"] == [2] and _st("c1_dynamic_long")["nblocks"] > 1000
    assert _st("c1_stored_framed")["block_types"] == [0] and _st("c1_stored_framed")["nblocks"] > 4000
    assert _st("c1_mix_short")["block_types"] == [0, 1, 2] and len(B.CASES["c1_mix_short"].expected) == 1
    s = B.CASES["c2_phase_short"].s
    stored_phases = {p for p, t in zip(s.phases, s.block_types) if t == 0}
    assert stored_phases == set(range(8))
    assert {k for k, v in s.stored_pads if v == (1 << k) - 1} == {1, 2, 3, 4, 5, 6, 7}   # every padding width, bits set
    lens = [len(B.CASES["c2_len_framed"].expected)]
    assert lens == [0 + 1 + 65535]
    assert b"\x00\x00\xff\xff" in B.CASES["c2_false_sync_short"].expected
    assert b"\x00\x00\x00\xff\xff\x00\x00\x00\xff\xff" in B.CASES["c2_false_sync_short"].expected
    assert b"\x00\x00\xff\xff" not in B.CASES["c2_false_hdr_long"].stream
    st = _st("c3_long")
    assert st["block_types"] == [0, 1, 2] and st["nblocks"] > 2000 and st["phases"] == list(range(8))
    assert B.CASES["c5_lastbit_short"].s.w.bitpos % 8 == 0
    assert B.CASES["c5_pad7_short"].s.w.bitpos % 8 == 1


def test_catalogue_intent_parallel_paths():
    c = B.CASES["d1_chain_long"]
    assert all(isinstance(t, int) for t in c.tokens[:32768])
    assert set(c.tokens[32768:]) == {(258, 32768)} and 650000 < len(c.expected) < 750000
    c = B.CASES["d2_ratio_long"]
    assert c.stats["widest"] == 2 and len(c.stream) >= 16384 and len(c.expected) > 16 << 20
    c = B.CASES["d3_density_long"]
    assert c.stats["widest"] == 1 and len(c.tokens) >= 8 * (len(c.stream) - 64)
    c = B.CASES["d4_resync_long"]
    assert len({t[1] for t in c.tokens if not isinstance(t, int)}) > 3000
    s = B.CASES["d5_syncs_framed"].stream
    assert b"\x00\x00\xff\xff\x00\x00\x00\xff\xff" in s     # two sync points back to back
    assert s[-7:-2] in (b"\x00\x00\x00\xff\xff", ) or b"\x00\x00\xff\xff" in s[-8:]   # one directly before the final block
    st = B.CASES["d5_syncs_framed"].s
    assert {p for p, t in zip(st.phases, st.block_types) if t == 0} == set(range(8))


def test_fixture_matches_catalogue(ref):
    """The committed reference fixture was made from these very streams."""
    assert set(ref) == set(B.CASES)
    for name, c in B.CASES.items():
        r = ref[name]["stream"]
        assert r["len"] == len(c.stream) and r["sha256"] == hashlib.sha256(c.stream).hexdigest(), name
        assert ("hex" in r) == (len(c.stream) <= 4096)
        if "hex" in r:
            assert bytes.fromhex(r["hex"]) == c.stream
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(golden, "inflate_constructed.json")) <= os.path.getsize(
        os.path.join(golden, "inflate.json"))


def _oracle_verdict(oracle, stream):
    import zt_oracle

    try:
        out, ip = oracle.raw_inflate(stream)
    except zt_oracle.OracleError as e:
        return {"error": e.msg}
    return {"out": {"len": len(out), "sha256": hashlib.sha256(out).hexdigest()}, "ip": ip}


@pytest.mark.parametrize("name", list(B.CASES))
def test_oracle_vs_fixture(oracle, ref, name):
    """The oracle's RawInflate does what the reference's did: output, `.ip`,
    error text.  (A case the reference gave no result for -- it can loop on
    an incomplete set -- is not run through the oracle either.)"""
    r = ref[name]
    if r.get("reference") == "no result":
        assert B.CASES[name].cls == "invalid"
        return
    got = _oracle_verdict(oracle, B.CASES[name].stream)
    want = {k: r[k] for k in ("out", "ip", "error") if k in r}
    assert got == want
    if B.CASES[name].cls == "valid" and "out" in r:
        assert r["out"]["sha256"] == hashlib.sha256(B.CASES[name].expected).hexdigest()


def test_class_table(ref, capsys):
    """Every malformed case with zlib's verdict and the reference's."""
    rows = []
    for name in INVALID:
        c = B.CASES[name]
        try:
            B.zlib_inflate(c.stream)
            z = "accepts"
        except zlib.error as e:
            z = str(e).split(": ", 1)[-1]
        r = ref[name]
        rv = r.get("reference") or r.get("error") or "decodes %d bytes, ip %d" % (r["out"]["len"], r["ip"])
        rows.append((name, c.kind, z, rv))
    with capsys.disabled():
        print("\n%-26s %-24s %-42s %s" % ("case", "kind", "zlib", "reference"))
        for row in rows:
            print("%-26s %-24s %-42s %s" % row)
    assert len(rows) == len(INVALID) and all(z != "accepts" for _, _, z, _ in rows)
    kinds = {k for _, k, _, _ in rows}
    assert {"first16", "run_overflow", "hlit_over_286", "hlit_over_286_coded", "no_eob", "incomplete_cl", "incomplete_litlen",
            "incomplete_dist", "oversubscribed", "reserved_symbol", "distance_too_far",
            "unassigned_distance_code"} == kinds


def test_design_tables_mirror_the_lists():
    """ACCEPTED_INVALID and BY_DESIGN_FALLBACK of the GPU test are closed
    lists, each with its row in DESIGN.md section 2."""
    import test_gpu_inflate_constructed as G

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "DESIGN.md")) as f:
        text = f.read()
    assert set(G.ACCEPTED_INVALID) <= {"first16", "run_overflow", "hlit_over_286"}
    for kind in G.ACCEPTED_INVALID:
        assert "`%s`" % kind in text
    for name in G.BY_DESIGN_FALLBACK:
        assert "`%s`" % name in text
        assert B.CASES[name].variant in ("framed", "long") and not B.CASES[name].group.startswith("d")
