"""Audit of the blocks block_kernel emits: every stream is opened with the
block parser (tests/deflate_audit.py) and what the kernel decided -- code
lengths, HLIT / HDIST / HCLEN, the run-length coding of the lengths, the
block type -- is held against an independent computation.

The other deflate tests see a stream from the outside only.  A dynamic form
that is wrong or too large loses the size comparison against the fixed form,
the stream stays valid and nothing fails; here such a block is caught by its
cost (it is not the package-merge optimum) or by its type (not the smallest
of the three forms for its own tokens).

The size accounting is block_kernel's: a Huffman block is followed by a sync
point (an empty stored block), so its form costs its bits + the 3-bit header
of the sync block, padded to a byte, + 4 bytes; the stored form costs
len + 5 * ceil(len / 65535) + 5 bytes.  Ties go to stored, then dynamic.
For the dynamic size of a block that was emitted in another form, the code
lengths come from zt_debug_huffman (the kernel's own tie-breaking decides a
few header bits); tests/test_gpu_huffman.py checks those against the
reference.
"""
import pytest

import audit_inputs as ai
import deflate_audit as da
import deflate_builder as db
import huffman_ref as hr

pytestmark = pytest.mark.gpu

LEVELS = [1, 6, 9]
INPUTS = {
    "dense": ai.dense_input,
    "wordsalad": lambda: ai.oracle_input("wordsalad"),
    "structured": lambda: ai.oracle_input("structured"),
    "zeros": ai.zeros_input,
    "period5": ai.period5_input,
    "random7bit": ai.seven_bit_input,
    "nomatch200": ai.no_match_input,     # empty distance histogram: two dummy codes
    "abab": lambda: b"ab" * 3000,        # one distance code in use
    "tiny1": lambda: b"x",
    "tiny2": lambda: b"xy",
    "tiny3": lambda: b"xyz",
}
CASES = [(name, level, 2) for name in INPUTS for level in LEVELS] + \
        [("dense", level, ctype) for ctype in (0, 1) for level in LEVELS]
MANY_SYMBOLS = 274  # used literal/length symbols from which 2m - 2 passes 544


@pytest.fixture(scope="module")
def zt():
    import ztamd

    return ztamd


@pytest.fixture(scope="module")
def streams(zt):
    """(name, level, ctype) -> (data, stream, blocks, blocks_unsearched), each
    made and parsed once."""
    cache = {}

    def get(name, level, ctype):
        key = (name, level, ctype)
        if key not in cache:
            data = INPUTS[name]()
            zt.timing_enable(True)
            s = zt.deflate_raw(data, compression_type=ctype, level=level)
            unsearched = zt.timing_read()["blocks_unsearched"]
            zt.timing_enable(False)
            cache[key] = (data, s, da.parse(s), unsearched)
        return cache[key]

    return get


def units(blocks):
    """[(blocks of the unit, its sync block)]: a Huffman block, or a run of
    non-empty stored blocks, followed by the empty stored block that makes
    the sync point."""
    out, i = [], 0
    while i < len(blocks):
        j = i + 1
        if blocks[i].btype == 0:
            assert blocks[i].stored_len > 0, "an empty stored block where a unit starts"
            while j < len(blocks) and blocks[j].btype == 0 and blocks[j].stored_len > 0:
                j += 1
        assert j < len(blocks) and blocks[j].btype == 0 and blocks[j].stored_len == 0, "no sync point after block %d" % i
        out.append((blocks[i:j], blocks[j]))
        i = j + 1
    return out


def body_bits(lit_hist, dist_hist, lit_lens, dist_lens):
    lit_lens = list(lit_lens) + [0] * (286 - len(lit_lens))
    dist_lens = list(dist_lens) + [0] * (30 - len(dist_lens))
    assert all(lit_lens[i] for i in range(286) if lit_hist[i]) and all(dist_lens[i] for i in range(30) if dist_hist[i])
    return sum(f * (lit_lens[i] + (db.LEN_EXTRA[i - 257] if i > 256 else 0)) for i, f in enumerate(lit_hist)) + \
        sum(f * (dist_lens[i] + db.DIST_EXTRA[i]) for i, f in enumerate(dist_hist))


def minimal(lens, floor):
    """The count of lengths to transmit: trailing zeros dropped, not below the format's minimum."""
    n = len(lens)
    while n > floor and lens[n - 1] == 0:
        n -= 1
    return n


def header_bits(hclen, cl_syms, cl_lens):
    return 3 + 5 + 5 + 4 + 3 * hclen + sum(cl_lens[s] + db.CL_EXTRA.get(s, 0) for s, _ in cl_syms)


def kernel_dynamic_bits(zt, lit_hist, dist_hist):
    """Bits of the dynamic form as block_kernel builds it for these histograms."""
    lit = zt.debug_huffman(lit_hist, 286, 15)[0][0].tolist()
    dist = zt.debug_huffman(dist_hist, 30, 15)[0][0].tolist()
    lit, dist = lit[:minimal(lit, 257)], dist[:minimal(dist, 1)]
    syms = hr.rle_greedy(lit + dist)
    cl_hist = [0] * 19
    for s, _ in syms:
        cl_hist[s] += 1
    cl = zt.debug_huffman(cl_hist, 19, 7)[0][0].tolist()
    hclen = minimal([cl[s] for s in db.CL_ORDER], 4)
    return header_bits(hclen, syms, cl) + body_bits(lit_hist, dist_hist, lit, dist), (lit, dist, cl)


def form_bytes(bits):
    return ((bits + 3 + 7) // 8) + 4


def stored_bytes(n):
    return n + 5 * ((n + 65534) // 65535) + 5


def audit_tokens(b, produced):
    for t in b.tokens:
        if isinstance(t, int):
            produced += 1
            continue
        assert len(t) == 2, "length 258 written as symbol 284 + 31"
        assert 3 <= t[0] <= 258 and 1 <= t[1] <= 32768 and t[1] <= produced, (t, produced)
        produced += t[0]
    return produced


def audit_dynamic(zt, b):
    """One dynamic block against the reference."""
    lit = b.lit_lens + [0] * (286 - b.hlit)
    dist = b.dist_lens + [0] * (30 - b.hdist)
    for lens, limit, what in ((lit, 15, "literal/length"), (dist, 15, "distance"), (b.cl_lens, 7, "code-length")):
        assert hr.kraft_at(lens, limit) == 1 << limit and max(lens) <= limit, "%s code is not complete" % what
    for hist, lens, limit, what in ((b.lit_hist, lit, 15, "literal/length"), (b.dist_hist, dist, 15, "distance"),
                                    (b.cl_hist, b.cl_lens, 7, "code-length")):
        want = hr.package_merge(hist, limit)
        assert hr.cost(hist, lens) == hr.cost(hist, want), \
            "%s cost %d, optimum %d (%d symbols used)" % (what, hr.cost(hist, lens), hr.cost(hist, want),
                                                          sum(1 for f in hist if f))
        # no code for an unused symbol beyond what the two-symbol rule adds
        assert sum(1 for l in lens if l) == max(2, sum(1 for f in hist if f)), what
    assert b.hlit == minimal(lit, 257) and b.hdist == minimal(dist, 1)
    assert b.hclen == minimal([b.cl_lens[s] for s in db.CL_ORDER], 4)
    assert b.cl_syms == hr.rle_greedy(b.lit_lens + b.dist_lens)
    assert b.header_bits == header_bits(b.hclen, b.cl_syms, b.cl_lens)


def audit(zt, data, blocks, ctype):
    """Every unit of one stream; returns [(block type, used literal/length symbols)]."""
    assert da.expand_blocks(blocks) == data
    assert blocks[-1].final and not any(b.final for b in blocks[:-1])
    if ctype == 0:
        assert all(b.btype == 0 and 0 < b.stored_len <= 65535 for b in blocks)
        return [(0, 0)] * len(blocks)
    kinds, produced = [], 0
    for us, sync in units(blocks):
        first = us[0]
        assert first.bit_start % 8 == 0 and sync.bit_end % 8 == 0
        emitted = (sync.bit_end - first.bit_start) // 8
        blen = sum(len(b.out) for b in us)
        assert 0 < blen <= 32768
        if first.btype == 0:
            # stored: judged with its bytes as literals (what a block without matches would cost)
            lit_hist, dist_hist = [0] * 286, [0] * 30
            for b in us:
                for c in b.out:
                    lit_hist[c] += 1
            lit_hist[256] = 1
            produced += blen
        else:
            assert len(us) == 1
            produced = audit_tokens(first, produced)
            lit_hist, dist_hist = first.lit_hist, first.dist_hist
            assert sum(lit_hist[257:]) == sum(dist_hist)
        fix = form_bytes(3 + body_bits(lit_hist, dist_hist, db.FIXED_LIT[:286], db.FIXED_DIST))
        dyn_k, (klit, kdist, kcl) = kernel_dynamic_bits(zt, lit_hist, dist_hist)
        dyn = form_bytes(dyn_k)
        if first.btype == 2:
            audit_dynamic(zt, first)
            # the block's own header and codes give the size the kernel planned
            mine = form_bytes(first.header_bits + body_bits(lit_hist, dist_hist, first.lit_lens, first.dist_lens))
            assert first.bit_end - first.bit_start == first.header_bits + body_bits(lit_hist, dist_hist, first.lit_lens,
                                                                                   first.dist_lens)
            assert (first.lit_lens, first.dist_lens, first.cl_lens) == (klit, kdist, kcl), \
                "block_kernel and zt_debug_huffman disagree on the same histogram"
            assert mine == dyn
        sto = stored_bytes(blen)
        if ctype == 1:
            want = 1
        else:
            want = 0 if sto <= dyn and sto <= fix else 2 if dyn <= fix else 1
        assert first.btype == want, "type %d emitted; stored %d, fixed %d, dynamic %d bytes" % (first.btype, sto, fix, dyn)
        assert emitted == (sto, fix, dyn)[first.btype], (emitted, first.btype, sto, fix, dyn)
        kinds.append((first.btype, sum(1 for f in lit_hist if f)))
    assert produced == len(data)
    return kinds


@pytest.mark.parametrize("name,level,ctype", CASES)
def test_blocks(zt, streams, name, level, ctype):
    data, s, blocks, _ = streams(name, level, ctype)
    kinds = audit(zt, data, blocks, ctype)
    if ctype == 2 and name in ("nomatch200", "abab", "zeros", "period5", "wordsalad", "structured", "random7bit", "dense"):
        assert 2 in [k for k, _ in kinds], "no dynamic block: the audit of the dynamic form did not run"
    if name == "nomatch200" and ctype == 2:
        b = blocks[0]
        assert sum(b.dist_hist) == 0 and [l for l in b.dist_lens if l] == [1, 1]
    if name == "abab" and ctype == 2:
        assert sum(1 for f in blocks[0].dist_hist if f) == 1


@pytest.mark.parametrize("level", LEVELS)
def test_dense_engages_the_many_symbol_path(zt, streams, level):
    """The `dense` input is searched (not stored by the classifier), and a
    block using at least 274 literal/length symbols comes out dynamic: its
    package-merge lists pass 544 entries."""
    data, s, blocks, unsearched = streams("dense", level, 2)
    assert unsearched == 0
    kinds = [(b.btype, b.used_lit) for b in blocks if b.btype]
    print("dense level %d: %d bytes, blocks (type, symbols used) %r" % (level, len(s), kinds))
    assert any(k == 2 and used >= MANY_SYMBOLS for k, used in kinds), kinds
