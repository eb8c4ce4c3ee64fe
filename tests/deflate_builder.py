"""Bit-level RFC 1951 writer and a catalogue of hand-built DEFLATE streams.

Every inflate test so far decodes what some encoder wrote; encoders never
write most of what RFC 1951 allows.  This module writes streams bit by bit --
48-bit tokens, 15-bit codes, header minima and malformed headers, thousands
of empty blocks, matches at the edge of the output produced -- and keeps for
each one the tokens it wrote, so that `expand` (a naive byte-at-a-time copy)
gives the expected output without zlib or the oracle.

    python tests/deflate_builder.py --dump DIR   # <name>.bin per case + index.json
    python tests/deflate_builder.py --list

Tokens are `int` literals, `(length, distance)` pairs, `(258, distance,
True)` for length 258 written as symbol 284 with extra bits 31, and for
deliberately invalid bodies `("code", value, nbits)` (MSB first, as Huffman
codes are packed) and `("bits", value, nbits)` (LSB first).
"""
import hashlib
import json
import os
import random
import sys

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


def len_symbol(length, alt258=False):
    """(symbol, extra bits, extra value) of a match length."""
    if alt258:
        assert length == 258
        return 284, 5, 31
    if length == 258:
        return 285, 0, 0
    for i in range(27, -1, -1):
        if length >= LEN_BASE[i]:
            return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]
    raise ValueError(length)


def dist_symbol(dist):
    for i in range(29, -1, -1):
        if dist >= DIST_BASE[i]:
            return i, DIST_EXTRA[i], dist - DIST_BASE[i]
    raise ValueError(dist)


def canonical_codes(lens):
    """RFC 1951 3.2.2 code assignment (codes of over-subscribed sets wrap)."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l] & ((1 << l) - 1)
            nxt[l] += 1
    return codes


def kraft(lens):
    """Sum of 2^-l in units of 2^-15: 32768 is a complete set."""
    return sum(32768 >> l for l in lens if l)


def flat_lengths(symbols, n):
    """A complete code over `symbols` (>= 2) with lengths m-1 / m."""
    symbols = sorted(symbols)
    k = len(symbols)
    assert k >= 2
    m = (k - 1).bit_length()
    short = (1 << m) - k
    lens = [0] * n
    for i, s in enumerate(symbols):
        lens[s] = m - 1 if i < short else m
    assert kraft(lens) == 32768
    return lens


def table(pairs, n):
    lens = [0] * n
    for s, l in pairs:
        lens[s] = l
    return lens


class BitWriter:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, nbits):
        """`nbits` of `value`, least significant bit first."""
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.buf.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, nbits):
        """A Huffman code: most significant bit first."""
        r = 0
        for _ in range(nbits):
            r = (r << 1) | (value & 1)
            value >>= 1
        self.bits(r, nbits)

    def align(self, fill=0):
        """Pad to a byte boundary with the low bits of `fill`."""
        if self.n:
            k = 8 - self.n
            self.bits(fill & ((1 << k) - 1), k)

    def bytes_(self, data):
        assert self.n == 0
        self.buf += data

    @property
    def bitpos(self):
        return len(self.buf) * 8 + self.n

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


def rle_plain(seq):
    return [(v, 0) for v in seq]


def rle_greedy(seq):
    """Code-length symbols with 16 / 17 / 18 runs, longest run first."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
            out += [(v, 0)] * run
        i = j
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}
CL_REP0 = {16: 3, 17: 3, 18: 11}


def cl_runs(syms):
    """[(first index, symbol, repeat)] of a code-length symbol list."""
    runs, i = [], 0
    for s, x in syms:
        rep = CL_REP0[s] + x if s >= 16 else 1
        runs.append((i, s, rep))
        i += rep
    return runs


class Stream:
    """One DEFLATE stream under construction, with what it was built from."""

    def __init__(self, history=b""):
        self.w = BitWriter()
        self.tokens = []          # everything that produces output, in order
        self.history = bytes(history)
        self.produced = len(history)
        self.widest = 0           # widest token in bits (codes + extra bits)
        self.lit_code_lens = set()
        self.dist_code_lens = set()
        self.len_syms = set()
        self.dist_syms = set()
        self.nblocks = 0
        self.phases = []          # bit phase (0-7) of every block start
        self.block_types = []
        self.headers = []         # per dynamic block: dict(hlit, hdist, hclen, runs)
        self.allones15 = [False, False]  # the all-ones 15-bit code used: lit/len, distance
        self.stored_pads = set()  # (pad bits, value) of stored blocks with padding

    # ---- blocks ------------------------------------------------------------
    def _header(self, final, btype):
        self.phases.append(self.w.bitpos & 7)
        self.block_types.append(btype)
        self.nblocks += 1
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, data, final=False, pad_bits=0, nlen=None):
        data = bytes(data)
        assert len(data) <= 65535
        self._header(final, 0)
        if self.w.n:
            self.stored_pads.add((8 - self.w.n, pad_bits & ((1 << (8 - self.w.n)) - 1)))
        self.w.align(pad_bits)
        n = len(data)
        self.w.bytes_(n.to_bytes(2, "little") + ((n ^ 0xFFFF) if nlen is None else nlen).to_bytes(2, "little"))
        self.w.bytes_(data)
        self.tokens += list(data)
        self.produced += n

    def sync_point(self):
        """An empty stored block: the byte after its 00 00 FF FF is a sync point."""
        self.stored(b"")

    def fixed(self, tokens, final=False, eob=True):
        self._header(final, 1)
        self._body(tokens, FIXED_LIT, FIXED_DIST, eob)

    def dynamic(self, tokens, lit_lens, dist_lens, final=False, cl="greedy", cl_lens=None, hclen=None, eob=True):
        """cl: "plain", "greedy", or an explicit list of (CL symbol, extra value)."""
        hlit, hdist = len(lit_lens), len(dist_lens)
        assert 257 <= hlit <= 288 and 1 <= hdist <= 32
        seq = list(lit_lens) + list(dist_lens)
        syms = rle_plain(seq) if cl == "plain" else rle_greedy(seq) if cl == "greedy" else list(cl)
        if cl_lens is None:
            used = sorted({s for s, _ in syms})
            if len(used) == 1:
                used = sorted(set(used) | {0 if used[0] else 8})
            cl_lens = flat_lengths(used, 19)
        cl_lens = list(cl_lens)
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        self._header(final, 2)
        self.w.bits(hlit - 257, 5)
        self.w.bits(hdist - 1, 5)
        self.w.bits(hclen - 4, 4)
        for i in range(hclen):
            self.w.bits(cl_lens[CL_ORDER[i]], 3)
        codes = canonical_codes(cl_lens)
        for s, x in syms:
            self.w.code(codes[s], cl_lens[s])
            if s >= 16:
                self.w.bits(x, CL_EXTRA[s])
        self.headers.append({"hlit": hlit, "hdist": hdist, "hclen": hclen, "runs": cl_runs(syms),
                             "cl_lens": cl_lens, "first": syms[0][0]})
        self._body(tokens, lit_lens, dist_lens, eob)

    def raw_bits(self, value, nbits):
        """Bits of a deliberately invalid body or header, LSB first."""
        self.w.bits(value, nbits)

    def _body(self, tokens, lit_lens, dist_lens, eob):
        lc, dc = canonical_codes(lit_lens), canonical_codes(dist_lens)
        w = self.w
        for t in tokens:
            if isinstance(t, int):
                assert lit_lens[t], "literal %d has no code" % t
                w.code(lc[t], lit_lens[t])
                self._used(0, lit_lens[t], lc[t])
                self.widest = max(self.widest, lit_lens[t])
                self.tokens.append(t)
                self.produced += 1
            elif t[0] == "code":
                w.code(t[1], t[2])
            elif t[0] == "bits":
                w.bits(t[1], t[2])
            else:
                length, dist = t[0], t[1]
                ls, lx, lv = len_symbol(length, len(t) > 2 and t[2])
                ds, dx, dv = dist_symbol(dist)
                assert lit_lens[ls] and dist_lens[ds], "token %r has no code" % (t,)
                w.code(lc[ls], lit_lens[ls])
                w.bits(lv, lx)
                w.code(dc[ds], dist_lens[ds])
                w.bits(dv, dx)
                self._used(0, lit_lens[ls], lc[ls])
                self._used(1, dist_lens[ds], dc[ds])
                self.len_syms.add(ls)
                self.dist_syms.add(ds)
                self.widest = max(self.widest, lit_lens[ls] + lx + dist_lens[ds] + dx)
                self.tokens.append((length, dist))
                self.produced += length
        if eob:
            w.code(lc[256], lit_lens[256])
            self._used(0, lit_lens[256], lc[256])

    def _used(self, which, nbits, code):
        (self.dist_code_lens if which else self.lit_code_lens).add(nbits)
        if nbits == 15 and code == 0x7FFF:
            self.allones15[which] = True

    # ---- results -----------------------------------------------------------
    def getvalue(self):
        return self.w.getvalue()

    @property
    def nbytes(self):
        return len(self.w.buf)

    def stats(self):
        return {"widest": self.widest, "lit_code_lens": sorted(self.lit_code_lens),
                "dist_code_lens": sorted(self.dist_code_lens), "len_syms": sorted(self.len_syms),
                "dist_syms": sorted(self.dist_syms), "nblocks": self.nblocks, "phases": sorted(set(self.phases)),
                "block_types": sorted(set(self.block_types)), "allones15": list(self.allones15)}


def expand(tokens, history=b""):
    """The output of a token list by naive byte-at-a-time copy."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t[0], t[1]
            if dist > len(out):
                raise ValueError("distance %d with %d bytes produced" % (dist, len(out)))
            p = len(out) - dist
            for k in range(length):
                out.append(out[p + k])
    return bytes(out[len(history):])


# =============================================================================
# The catalogue.  A feature is a function f(s, final, i) that appends the
# feature's blocks to Stream `s` (`i` = repetition number, which seeds its
# random choices); the last block it writes carries BFINAL when `final`.
# =============================================================================
LONG_BYTES = 20 << 10
LITS12 = [ord(c) for c in "etaoinshrdlu"]

# A1: lit/len lengths 1..13 on twelve literals and EOB, 15 on 281-284;
# distance lengths 1..14 on symbols 0-13, 15 on 28 and 29
A1_LIT = table([(s, i + 1) for i, s in enumerate(LITS12)] + [(256, 13)] + [(s, 15) for s in (281, 282, 283, 284)], 286)
A1_DIST = table([(s, s + 1) for s in range(14)] + [(28, 15), (29, 15)], 30)
assert kraft(A1_LIT) == 32768 and kraft(A1_DIST) == 32768


def _prime(s, target, rng):
    """Cheap A1 tokens until `target` bytes exist: a few literals, then long
    distance-1..4 matches (distance codes of 1-4 bits)."""
    toks = [rng.choice(LITS12) for _ in range(8)]
    made = s.produced + 8
    while made < target:
        L = rng.randrange(131, 259)
        toks.append((258, rng.randrange(1, 5), True) if L == 258 else (L, rng.randrange(1, 5)))
        made += L
    return toks


def _wide_tokens(rng, count, lo=16385):
    out = []
    for _ in range(count):
        L = rng.randrange(131, 259)
        d = rng.randrange(lo, 32769)
        out.append((258, d, True) if L == 258 else (L, d))
    return out


def f_a1(s, final, i):
    rng = random.Random(1000 + i)
    toks = _prime(s, 32768, rng) + _wide_tokens(rng, 40) + [(258, 32768, True)]
    s.dynamic(toks, A1_LIT, A1_DIST, final)


# A2: every code length 1..15 in both tables; 8- and 9-bit codes adjacent;
# the all-ones 15-bit code (the highest symbol of length 15) is used
A2_LIT = table(list(zip([ord("e"), ord("t"), ord("a"), ord("o"), 256, ord("i"), 257, ord("n"), ord("s"), ord("h"),
                         270, ord("r"), ord("d"), ord("l")], range(1, 15))) + [(ord("u"), 15), (285, 15)], 286)
A2_DIST = table([(0, 15)] + [(s, s) for s in range(1, 15)] + [(15, 15)], 30)
assert kraft(A2_LIT) == 32768 and kraft(A2_DIST) == 32768


def _random_tokens(rng, lit_lens, dist_lens, count, produced, force=()):
    """Tokens drawn uniformly over the coded symbols (long codes as often as
    short ones), every match within the bytes produced; `force` first."""
    lits = [x for x in range(256) if lit_lens[x]]
    lsyms = [x for x in range(257, min(len(lit_lens), 286)) if lit_lens[x]]
    dsyms = [x for x in range(min(len(dist_lens), 30)) if dist_lens[x]]
    toks = []
    pending = list(force)
    while len(toks) < count or pending:
        if pending and (isinstance(pending[0], int) or pending[0][1] <= produced):
            t = pending.pop(0)
        elif lsyms and dsyms and produced and rng.random() < 0.6:
            ls = rng.choice(lsyms) - 257
            ds = rng.choice([d for d in dsyms if DIST_BASE[d] <= produced])
            L = LEN_BASE[ls] + rng.randrange(1 << LEN_EXTRA[ls])
            d = min(DIST_BASE[ds] + rng.randrange(1 << DIST_EXTRA[ds]), produced)
            t = (L, d)
        else:
            t = rng.choice(lits)
        toks.append(t)
        produced += 1 if isinstance(t, int) else t[0]
    return toks


def f_a2(s, final, i):
    rng = random.Random(2000 + i)
    lead = [rng.choice(LITS12) for _ in range(260)] + [ord("u")]
    toks = lead + _random_tokens(rng, A2_LIT, A2_DIST, 150, s.produced + len(lead), force=[(258, 256), (3, 1)])
    s.dynamic(toks, A2_LIT, A2_DIST, final)


LIT_AB = table([(97, 1), (256, 2), (257, 3), (285, 3)], 286)  # a, EOB, length 3, length 258


def f_a3(s, final, i):
    s.dynamic([97, 97, (3, 1), 97, (258, 1), (3, 1)] * 20, LIT_AB, [1], final)  # one distance code: code 0


def f_a4(s, final, i):
    lit = table([(97, 1), (98, 2), (256, 2)], 257)
    s.dynamic([97, 98, 98, 97] * 100, lit, [0], final)  # HDIST = 1 with length 0: literals only


CL7 = table([(0, 1), (8, 2), (16, 3), (17, 4), (18, 5), (7, 6), (15, 7), (1, 7)], 19)
assert kraft(CL7) == 32768


def f_a5(s, final, i):
    # HLIT = 257, HCLEN = 5, CL lengths {0, 8} only: 256 codes of length 8
    lit8 = [8] * 255 + [0, 8]
    rng = random.Random(5000 + i)
    s.dynamic([rng.randrange(255) for _ in range(300)], lit8, [0], False, cl="plain",
              cl_lens=table([(0, 1), (8, 1)], 19))
    # HCLEN = 19 with 7-bit CL codes (length value 1 is coded in 7 bits)
    lit = table([(200, 1)] + [(x, 8) for x in range(127)] + [(256, 8)], 257)
    s.dynamic([200, 5, 200, 126, 200, 0] * 30 + [200], lit, [1, 1], final, cl_lens=CL7)


def f_a6(s, final, i):
    flat16 = table([(x, 4) for x in list(range(100, 109)) + [256] + list(range(280, 286))], 286)
    body = [100, 101, 102, 103, 104, 105, 106, 107, 108, (115, 3), (258, 9), (131, 5)] * 8
    # a 16-run from the last lit/len lengths into the distance lengths; 18 first
    s.dynamic(body, flat16, [4] * 16, False)
    # an 18-run ending exactly at HLIT + HDIST; a run of 138
    lit = flat_lengths([200, 201, 202, 256, 257], 258)
    s.dynamic([200, 201, 202, (3, 2)] * 10, lit, [1, 1] + [0] * 20, False)
    # a 17-run ending exactly at HLIT + HDIST; a 16-run of exactly 6; 17 first
    lit = table([(x, 3) for x in range(5, 12)] + [(256, 3)] + [(257, 0)], 258)
    s.dynamic([5, 6, 7, 8, 9, 10, 11] * 10, lit, [1, 1] + [0] * 7, final)


def f_b1(s, final, i):
    lit = flat_lengths([65, 66, 67, 256] + list(range(257, 286)), 286)
    dist = flat_lengths(range(0, 18), 30)
    rng = random.Random(11000 + i)
    toks = [rng.choice([65, 66, 67]) for _ in range(300)]
    for L in range(3, 259):
        toks.append((L, rng.randrange(1, 300)))
        if L % 16 == 0:
            toks.append(rng.choice([65, 66, 67]))
    toks.append((258, 7, True))
    toks.append((258, 300))
    s.dynamic(toks, lit, dist, final)


def f_b2(s, final, i):
    lit = flat_lengths([65, 66, 67, 68, 256, 257, 258, 285], 286)
    dist = flat_lengths(range(30), 30)
    rng = random.Random(12000 + i)
    toks = [rng.choice([65, 66, 67, 68]) for _ in range(40)]
    made = s.produced + 40
    while made < 32768:
        toks.append((258, rng.randrange(1, 41)))
        made += 258
    for ds in range(30):
        toks += [(3, DIST_BASE[ds]), rng.choice([65, 66, 67, 68]), (4, DIST_BASE[ds] + (1 << DIST_EXTRA[ds]) - 1)]
    s.dynamic(toks, lit, dist, final)


B3_D = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257]


def f_b3(s, final, i):
    rng = random.Random(13000 + i)
    toks = [rng.randrange(256) for _ in range(300)]
    for D in B3_D:
        for L in sorted({3, D - 1, D, D + 1, 258}):
            if L >= 3:
                toks += [(L, D), rng.randrange(256)]
    s.fixed(toks, final)


LIT_EOB_ONLY = table([(256, 1)], 257)


def f_c1_fixed(s, final, i):
    """An empty fixed block is 10 bits: block starts walk the even bit phases.
    One empty dynamic block of 93 bits in the middle moves them to the odd ones."""
    for k in range(100):
        if k == 50:
            s.dynamic([], LIT_EOB_ONLY, [0])
        else:
            s.fixed([], final and k == 99)


def f_c1_dynamic(s, final, i):
    for k in range(24):
        s.dynamic([], LIT_EOB_ONLY, [0], final and k == 23)


def f_c1_stored(s, final, i):
    for k in range(60):
        s.stored(b"", final and k == 59)


def f_c1_mix(s, final, i):
    for k in range(40):
        [lambda: s.fixed([]), lambda: s.dynamic([], LIT_EOB_ONLY, [0]), lambda: s.stored(b"", pad_bits=0x55)][k % 3]()
    s.fixed([ord("!")], final)


def f_c2_len(s, final, i):
    rng = random.Random(22000 + i)
    s.stored(b"", False)
    s.stored(b"Z", False)
    s.stored(rng.randbytes(65535), final)


def f_c2_phase(s, final, i):
    """A stored block after a Huffman block ending at each bit phase, the
    padding bits set."""
    for j in range(8):
        s.fixed([200 + j] * j, False)       # 3 + 9 j + 7 bits: j = 0..7 ends on every phase
        s.stored(bytes([48 + j] * (j + 1)), final and j == 7, pad_bits=0xFF)


def _false_candidates(with_sync):
    t = Stream()
    f_a2(t, False, 77)
    f_a5(t, False, 77)
    blob = t.getvalue()
    rng = random.Random(77)
    parts = []
    for k in range(12):
        parts.append(blob[rng.randrange(8):][: 200 + 17 * k])
        parts.append(b"\x00\x00\xff\xff" if with_sync else b"\x05\x00\xfa\xff")
        parts.append(b"\x00" * (k % 3) + b"\x00\x00\x00\xff\xff\x00\x00\x00\xff\xff" if with_sync else b"\xed\xbd")
    return b"".join(parts)


def f_c2_false_hdr(s, final, i):
    """Stored payload that parses as dynamic headers and stored LEN / NLEN pairs."""
    s.fixed([65 + i % 26], False)
    s.stored(_false_candidates(False), final, pad_bits=0x2A)


def f_c2_false_sync(s, final, i):
    """Stored payload holding 00 00 FF FF and whole restart markers."""
    s.fixed([65 + i % 26], False)
    s.stored(_false_candidates(True), final, pad_bits=0x15)


def f_c3(s, final, i):
    lit = flat_lengths([120, 121, 256, 257, 260], 286)
    rng = random.Random(23000 + i)
    s.stored(bytes(rng.randrange(256) for _ in range(6)), False)
    for k in range(30):
        last = final and k == 29
        t = rng.choice([120, 121, (3, rng.randrange(1, 7)), (6, rng.randrange(1, 7))])
        if k % 3 == 0:
            s.fixed([t], last)
        elif k % 3 == 1:
            s.dynamic([t], lit, [2, 2, 2, 3, 3], last)
        else:
            s.stored(bytes([rng.randrange(256)]), last, pad_bits=rng.randrange(256))


def f_c4(s, final, i):
    rng = random.Random(24000 + i)
    s.stored(rng.randbytes(40), False, pad_bits=0x7F)
    s.fixed([(40, 40), 33, (258, 81)], False)            # first token: a match into the stored block
    lit = flat_lengths([33, 256, 270, 285], 286)
    s.dynamic([(258, 300), 33, (25, 339 + 258 + 1)], lit, flat_lengths(range(12, 20), 30), False)
    s.stored(b"tail", False)
    s.fixed([(4, 4), (3, 600)], final)


def f_c4_restart(s, final, i):
    """A match reaching behind a restart marker (two byte-aligned empty stored
    blocks): the sync-point path would start an independent segment there."""
    s.stored(random.Random(24500 + i).randbytes(400), False)
    s.sync_point()
    s.sync_point()
    s.fixed([(5, 300), 65, (258, 401)], final)


def f_c5_lastbit(s, final, i):
    s.fixed([150] * 6, final)  # 3 + 6 * 9 + 7 = 64 bits: EOB ends on the last bit of a byte


def f_c5_pad7(s, final, i):
    s.fixed([150] * 7, final)  # 73 bits: 7 padding bits follow


# features with their catalogue entry: (group, function, holds 00 00 FF FF itself, what it is for)
VALID_FEATURES = [
    ("a1", f_a1, False, "48-bit tokens: 15 + 5 + 15 + 13"),
    ("a2", f_a2, False, "comb tables: every code length 1..15 in both trees, all-ones 15-bit code used"),
    ("a3", f_a3, False, "one distance code of length 1, code 0 only"),
    ("a4", f_a4, False, "HDIST = 1 with length 0, literals only"),
    ("a5", f_a5, False, "HLIT = 257, HCLEN = 5 with {0, 8}; HCLEN = 19 with 7-bit CL codes"),
    ("a6", f_a6, False, "run-length edges: 16 across HLIT, runs ending at HLIT + HDIST, 138, 6, 17 / 18 first"),
    ("b1", f_b1, False, "every length 3..258, 258 both ways"),
    ("b2", f_b2, False, "every distance symbol at both ends of its range"),
    ("b3", f_b3, False, "overlapping copies D x L"),
    ("c1_fixed", f_c1_fixed, False, "empty fixed blocks (and one empty dynamic block per hundred): block starts on all 8 bit phases"),
    ("c1_dynamic", f_c1_dynamic, False, "empty dynamic blocks"),
    ("c1_stored", f_c1_stored, True, "empty stored blocks"),
    ("c1_mix", f_c1_mix, True, "empty fixed / dynamic / stored blocks, then one literal"),
    ("c2_phase", f_c2_phase, False, "stored after a Huffman block ending on each bit phase, padding bits set"),
    ("c2_false_hdr", f_c2_false_hdr, False, "stored payload of plausible dynamic headers and LEN / NLEN pairs"),
    ("c2_false_sync", f_c2_false_sync, True, "stored payload holding 00 00 FF FF and restart markers"),
    ("c3", f_c3, False, "one token per block: fixed, dynamic, stored in turn"),
    ("c4", f_c4, False, "matches into earlier blocks of another type, a match as a block's first token"),
    ("c4_restart", f_c4_restart, True, "a match reaching behind a restart marker (00 00 00 FF FF 00 00 00 FF FF)"),
    ("c5_lastbit", f_c5_lastbit, False, "final EOB is the last bit of the last byte"),
    ("c5_pad7", f_c5_pad7, False, "final EOB followed by 7 padding bits"),
]


def build_short(f):
    s = Stream()
    f(s, True, 0)
    return s


def build_long(f, framed, tail=None):
    """`f` repeated until the stream is long enough for the parallel paths,
    with a sync point after every repetition when `framed`; `tail` (default:
    one more repetition) writes the final block."""
    s = Stream()
    i = 0
    while s.nbytes < LONG_BYTES:
        f(s, False, i)
        if framed:
            s.sync_point()
        i += 1
    (tail or f)(s, True, i)
    return s


class Case:
    def __init__(self, name, group, variant, cls, feature, make, kind=None):
        self.name, self.group, self.variant, self.cls, self.feature = name, group, variant, cls, feature
        self.kind = kind          # malformed cases: what is wrong (ACCEPTED_INVALID is keyed by it)
        self._make = make
        self._s = None
        self._expected = None
        self.trailing = b""

    @property
    def s(self):
        if self._s is None:
            self._s = self._make()
        return self._s

    @property
    def stream(self):
        return self.s.getvalue() + self.trailing

    @property
    def tokens(self):
        return self.s.tokens

    @property
    def stats(self):
        return self.s.stats()

    @property
    def expected(self):
        """expand(tokens): defined for every case whose tokens stay in range."""
        if self._expected is None:
            self._expected = expand(self.s.tokens, self.s.history)
        return self._expected


CASES = {}


def _add(name, group, variant, cls, feature, make, kind=None, trailing=b""):
    assert name not in CASES, name
    c = Case(name, group, variant, cls, feature, make, kind)
    c.trailing = trailing
    CASES[name] = c
    return c


for _g, _f, _sync, _what in VALID_FEATURES:
    _add(_g + "_short", _g, "short", "valid", _what, lambda f=_f: build_short(f))
    _add(_g + "_framed", _g, "framed", "valid", _what, lambda f=_f: build_long(f, True))
    if not _sync:
        _add(_g + "_long", _g, "long", "valid", _what, lambda f=_f: build_long(f, False))

# C2 LEN 0 / 1 / 65535 is long by itself and holds a sync point (LEN 0)
_add("c2_len_framed", "c2_len", "framed", "valid", "stored LEN 0, 1 and 65535", lambda: build_short(f_c2_len))
# C5: bytes after the stream
_add("c5_trailing_short", "c5_trailing", "short", "valid", "trailing bytes after the stream",
     lambda: build_short(f_c5_pad7), trailing=b"TRAILING BYTES \x00\x00\xff\xff")
_add("c5_trailing_long", "c5_trailing", "long", "valid", "trailing bytes after the stream",
     lambda: build_long(f_a2, False), trailing=b"TRAILING BYTES " * 3)


# ---- B4: distance against the output produced --------------------------------
def _b4(where, over, variant):
    """where: "first" (nothing but plain data before the match), "sync" (the
    first token after a sync point), "far" (after 40 000 bytes: D = 32768, the
    format's maximum; one more cannot be written).  `over`: the distance is
    one more than the bytes produced."""
    def make():
        s = Stream()
        rng = random.Random(14000 + len(where))
        if where == "first" and variant == "short":  # literals and the match in the first block
            s.fixed([rng.randrange(256) for _ in range(37)] + [(5, 37 + over), 65], True)
            return s
        if variant == "short":
            s.fixed([rng.randrange(256) for _ in range(37)], False)
        else:
            n = 40000 if where == "far" else LONG_BYTES
            while s.produced < n:
                s.stored(rng.randbytes(min(20000, n - s.produced)), False)
        if where == "sync" or variant == "framed":
            s.sync_point()
        s.fixed([(5, min(s.produced, 32768) + over), 65], True)
        return s
    return make


for _where, _variant in (("first", "short"), ("first", "long"), ("sync", "short"), ("sync", "framed"),
                         ("far", "long"), ("far", "framed")):
    _n = "b4_%s_%s" % (_where, _variant)
    _add(_n + "_eq", "b4", _variant, "valid", "distance equal to the bytes produced (%s)" % _where,
         _b4(_where, 0, _variant))
    if _where != "far":
        _add(_n + "_over", "b4", _variant, "invalid", "distance one more than the bytes produced (%s)" % _where,
             _b4(_where, 1, _variant), kind="distance_too_far")


# ---- malformed cases: the bad block after valid filler ------------------------
def _filler(s, final, i):
    f_a2(s, final, i)


def _invalid(name, group, what, bad, kind):
    """bad(s): appends the malformed final block."""
    _add(name + "_short", group, "short", "invalid", what, lambda: build_short(lambda s, f, i: bad(s)), kind)
    _add(name + "_framed", group, "framed", "invalid", what,
         lambda: build_long(_filler, True, lambda s, f, i: bad(s)), kind)
    _add(name + "_long", group, "long", "invalid", what,
         lambda: build_long(_filler, False, lambda s, f, i: bad(s)), kind)


def bad_a3(s):  # the one distance code's sibling, code 1
    lc = canonical_codes(LIT_AB)
    s.dynamic([97, 97, ("code", lc[257], 3), ("code", 1, 1), 97], LIT_AB, [1], True)


def bad_a4(s):  # a length symbol with no distance code at all
    lit = table([(97, 1), (256, 2), (257, 2)], 258)
    s.dynamic([97, 97, ("code", canonical_codes(lit)[257], 2), ("bits", 0, 5), 97], lit, [0], True)


_invalid("a3_code1", "a3", "single distance code: the unassigned code 1 used", bad_a3, "unassigned_distance_code")
_invalid("a4_length", "a4", "no distance code, a length symbol in the body", bad_a4, "unassigned_distance_code")

A7_LIT = table([(0, 0), (1, 0), (2, 0), (3, 0), (65, 2), (66, 2), (67, 3), (256, 3), (257, 3), (258, 3)], 259)
A7_BODY = [65, 66, 67, 65, (3, 2), (4, 1), 66]


def bad_first16(s):  # 16 with nothing before it: lengths 0-2 stay zero
    s.dynamic(A7_BODY, A7_LIT, [1, 1], True, cl=[(16, 0)] + rle_greedy(A7_LIT[3:] + [1, 1]))


def bad_overflow(s):  # the last run overflows HLIT + HDIST
    seq = A7_LIT + [1, 1, 0, 0, 0, 0]
    s.dynamic(A7_BODY, A7_LIT, [1, 1, 0, 0, 0, 0], True, cl=rle_greedy(seq[:-4]) + [(18, 100)])


def _bad_hlit(n, coded):
    def bad(s):
        syms = [65, 66, 67, 256, 257, 258]
        lit = flat_lengths(syms + [286, 287][: n - 286] if coded else syms + [259, 260], n)
        s.dynamic(A7_BODY, lit, [1, 1], True)
    return bad


def bad_no_eob(s):
    lit = table([(65, 1), (66, 2), (67, 2)], 257)
    s.dynamic([65, 66, 67] * 40, lit, [0], True, eob=False)


def bad_incomplete_cl(s):
    lit8 = [8] * 255 + [0, 8]
    s.dynamic([1, 2, 3], lit8, [0], True, cl="plain", cl_lens=table([(0, 2), (8, 2), (18, 2)], 19))


def bad_incomplete_lit(s):  # two codes of length 2; only assigned codes used
    s.dynamic([65, 65, 65], table([(65, 2), (256, 2)], 257), [0], True)


def bad_incomplete_dist(s):  # two distance codes of length 2
    s.dynamic([65, 65, (3, 1), (3, 2)], table([(65, 1), (256, 2), (257, 2)], 258), [2, 2], True)


def bad_over_cl(s):
    lit8 = [8] * 255 + [0, 8]
    s.dynamic([1, 2, 3], lit8, [0], True, cl="plain", cl_lens=table([(0, 1), (8, 1), (18, 1)], 19))


def bad_over_lit(s):
    s.dynamic([65, 66], table([(65, 1), (66, 1), (256, 1)], 257), [0], True)


def bad_over_dist(s):
    s.dynamic([65, 65, (3, 1)], table([(65, 1), (256, 2), (257, 2)], 258), [1, 1, 1], True)


_invalid("a7_first16", "a7", "repeat-previous (16) as the first code-length symbol", bad_first16, "first16")
_invalid("a7_overflow", "a7", "a run overflowing HLIT + HDIST", bad_overflow, "run_overflow")
_invalid("a7_hlit287", "a7", "HLIT = 287, symbol 286 coded but unused", _bad_hlit(287, True), "hlit_over_286_coded")
_invalid("a7_hlit288", "a7", "HLIT = 288, symbols 286 and 287 coded but unused", _bad_hlit(288, True), "hlit_over_286_coded")
_invalid("a7_hlit288z", "a7", "HLIT = 288, symbols 286 and 287 with length 0", _bad_hlit(288, False), "hlit_over_286")
_invalid("a7_no_eob", "a7", "no end-of-block code", bad_no_eob, "no_eob")
_invalid("a7_incomplete_cl", "a7", "incomplete code-length code", bad_incomplete_cl, "incomplete_cl")
_invalid("a7_incomplete_lit", "a7", "incomplete lit/len set of two codes", bad_incomplete_lit, "incomplete_litlen")
_invalid("a7_incomplete_dist", "a7", "incomplete distance set of two codes", bad_incomplete_dist, "incomplete_dist")
_invalid("a7_over_cl", "a7", "over-subscribed code-length code", bad_over_cl, "oversubscribed")
_invalid("a7_over_lit", "a7", "over-subscribed lit/len set", bad_over_lit, "oversubscribed")
_invalid("a7_over_dist", "a7", "over-subscribed distance set", bad_over_dist, "oversubscribed")

# B5: reserved symbols in a fixed block (286 / 287: 8-bit codes 11000110 / 11000111; 30 / 31: 11110 / 11111)
for _sym, _toks in ((286, [("code", 0xC6, 8), ("bits", 0, 5)]), (287, [("code", 0xC7, 8), ("bits", 0, 5)]),
                    (30, [("code", 0x01, 7), ("code", 30, 5)]), (31, [("code", 0x01, 7), ("code", 31, 5)])):
    _invalid("b5_sym%d" % _sym, "b5", "reserved symbol %d in a fixed block" % _sym,
             lambda s, t=_toks: s.fixed([65, 66, 67, 68] + t + [65], True), "reserved_symbol")


# ---- D: built against the parallel paths (long only) ---------------------------
def make_d1():
    s = Stream()
    rng = random.Random(31000)
    toks = [rng.choice(LITS12) for _ in range(32768)] + [(258, 32768, True)] * 2600
    s.dynamic(toks, A1_LIT, A1_DIST, True)
    return s


def make_d2():
    s = Stream()
    lit = table([(97, 2), (256, 2), (285, 1)], 286)
    s.dynamic([97] + [(258, 1)] * 66000, lit, [1], True)
    return s


def make_d3():
    s = Stream()
    s.dynamic([97] * (LONG_BYTES * 8), table([(97, 1), (256, 1)], 257), [0], True)
    return s


def make_d4():
    s = Stream()
    rng = random.Random(34000)
    s.dynamic(_prime(s, 32768, rng) + _wide_tokens(rng, 3600), A1_LIT, A1_DIST, True)
    return s


def make_d5():
    s = Stream()
    i = 0
    while s.nbytes < LONG_BYTES:
        f_a2(s, False, i)
        s.fixed([200 + i % 8] * (i % 8), False)  # ends on bit phase (10 + 9 j) mod 8
        s.sync_point()
        if i % 5 == 0:
            s.sync_point()                       # two sync points back to back
        i += 1
    f_a2(s, False, i)
    s.sync_point()                               # a sync point directly before the final block
    s.fixed([33], True)
    return s


_add("d1_chain_long", "d1", "long", "valid", "deep (258, 32768) match chain in 48-bit tokens", make_d1)
_add("d2_ratio_long", "d2", "long", "valid", "(258, 1) matches in 2-bit tokens: about 1000:1", make_d2)
_add("d3_density_long", "d3", "long", "valid", "8 tokens per byte: two 1-bit codes", make_d3)
_add("d4_resync_long", "d4", "long", "valid", "48-bit tokens with random extra bits: slow resynchronisation", make_d4)
_add("d5_syncs_framed", "d5", "framed", "valid", "sync points back to back, before the final block, after each phase",
     make_d5)


def dict_stream(dist, length=5):
    """A stream whose first token reaches `dist` bytes back into a preset dictionary."""
    s = Stream()
    s.fixed([(length, dist), 90, (3, 1)], True)
    return s


def short_valid():
    return [c for c in CASES.values() if c.cls == "valid" and c.variant == "short"]


def zlib_inflate(stream, zdict=None):
    """(output, bytes consumed) by zlib's raw inflate; zlib.error on a stream it
    rejects, ValueError on one it does not see the end of."""
    import zlib

    d = zlib.decompressobj(-15, zdict=zdict) if zdict is not None else zlib.decompressobj(-15)
    out = d.decompress(stream)
    if not d.eof:
        raise ValueError("stream incomplete")
    return out, len(stream) - len(d.unused_data)


def reference_records():
    """tests/golden/inflate_constructed.json (tools/gen_golden_constructed.mjs) by case name."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inflate_constructed.json")
    with open(path) as f:
        return {r["name"]: r for r in json.load(f)["records"]}


def main(argv):
    if len(argv) >= 2 and argv[0] == "--dump":
        os.makedirs(argv[1], exist_ok=True)
        index = []
        for c in CASES.values():
            data = c.stream
            with open(os.path.join(argv[1], c.name + ".bin"), "wb") as f:
                f.write(data)
            index.append({"name": c.name, "len": len(data), "sha256": hashlib.sha256(data).hexdigest()})
        with open(os.path.join(argv[1], "index.json"), "w") as f:
            json.dump(index, f, indent=1)
        print("%d cases written to %s" % (len(index), argv[1]))
        return 0
    for c in CASES.values():
        print("%-28s %-7s %-7s %7d B  %s" % (c.name, c.variant, c.cls, len(c.stream), c.feature))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
