"""The match audit's inputs (tests/test_gpu_match_audit.py; test_lz77_ref.py
checks them on the CPU): random filler with planted copies at the places where
the match kernel can go wrong, and a low-multiplicity vocabulary text.

The filler is random bytes over a 64-symbol alphabet: 6 bits of order-0
entropy keep every block below classify_kernel's stored verdict, and an 8-byte
key is 48 random bits, unique among a million positions except where planted.
A copy (src, dst = src + D, L) repeats L bytes; the bytes just before and just
after it are forced to differ from the source's neighbours, so the copy's
extent is exactly L and does not depend on chance.

Everything is a function of a lz77_ref.Geom and a few sizes read from the
library (sub-chunk, restart segment): nothing here states the kernel's
constants.
"""
from collections import namedtuple

import numpy as np

Copy = namedtuple("Copy", "src dst dist length tag")

ALPHA0, ALPHA_N = 0x30, 64
DISTANCES = lambda g: [1, 2, 5, 8, 16, 17, 255, 1024, 1025, 4096, 4097, 16384, g.maxdist - 1, g.maxdist,  # noqa: E731
                       g.maxdist + 1, 32768]
LENGTHS = [3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 128, 257, 258, 259, 600]


class Planter:
    """n bytes of filler and the copies planted into it.  `used` marks every
    byte a copy fixed -- its source, its destination and the byte on either
    side of both: a later copy never touches those."""

    def __init__(self, n, seed):
        self.rng = np.random.RandomState(seed)
        self.buf = (self.rng.randint(0, ALPHA_N, size=n) + ALPHA0).astype(np.uint8)
        self.used = np.zeros(n, dtype=bool)
        self.copies = []

    @property
    def n(self):
        return self.buf.size

    def free(self, dst, dist, length):
        src = dst - dist
        if src < 1 or dst + length > self.n:
            return False
        return not (self.used[src - 1:src + length + 1].any() or self.used[dst - 1:min(dst + length + 1, self.n)].any())

    def _differ(self, at, other):
        """buf[at] := a symbol that differs from buf[other] (and from itself)."""
        b = self.buf
        v = int(b[at])
        while v == b[other] or v == b[at]:
            v = ALPHA0 + (v - ALPHA0 + 1 + int(self.rng.randint(0, ALPHA_N - 1))) % ALPHA_N
        b[at] = v

    def plant(self, dst, dist, length, tag):
        """The copy src = dst - dist -> dst of `length` bytes (overlapping when
        length > dist); dst + length may be the data's end."""
        assert self.free(dst, dist, length), (dst, dist, length, tag)
        b, src = self.buf, dst - dist
        if 1 < dist < length and dist <= ALPHA_N:
            # an overlapping copy repeats its first `dist` bytes: all different,
            # so that no shorter period hides in them
            b[src:dst] = ALPHA0 + self.rng.permutation(ALPHA_N)[:dist]
        # the byte before: the source's is changed (it lies before both ranges)
        if b[src - 1] == b[dst - 1]:
            self._differ(src - 1, dst - 1)
        for k in range(length):
            b[dst + k] = b[src + k]
        # the byte after: the destination's is changed (no source byte lies there)
        if dst + length < self.n and b[dst + length] == b[src + length]:
            self._differ(dst + length, src + length)
        assert b[src - 1] != b[dst - 1] and (dst + length == self.n or b[dst + length] != b[src + length])
        self.used[src - 1:src + length + 1] = True
        self.used[dst - 1:min(dst + length + 1, self.n)] = True
        self.copies.append(Copy(src, dst, dist, length, tag))

    def place(self, dist, length, candidates, tag, required=True):
        """Plant at the first free destination among `candidates`; returns it
        (None when there is none and the copy is not required)."""
        for dst in candidates:
            if self.free(dst, dist, length):
                self.plant(dst, dist, length, tag)
                return dst
        assert not required, "no room for %s (D %d, L %d)" % (tag, dist, length)
        return None

    def data(self):
        return self.buf.tobytes()


def _tail(p, e, dist, length, tag):
    """a copy whose last byte is the data's e-th from the end (e = 1: the last)"""
    p.plant(p.n - (e - 1) - length, dist, length, tag)


def matrix(g, sub, seed=20):
    """The whole matrix in one input of a segment + 40 KiB + 37 bytes:
    (data, copies).  Destinations lie from the third block on, so that every
    distance has a source."""
    B, S, M = g.block, sub, g.maxdist
    n = g.segment + 40 * 1024 + 37
    p = Planter(n, seed)
    dists = DISTANCES(g)
    # -- fixed places first (the sweep below takes what is left) --
    # the restart point: sources before it and destinations after it (must
    # not be found), and a source that straddles it (only its part inside the
    # segment counts: one source, since only one range can hold the point)
    R = g.segment
    p.plant(R + 300, 1025, 33, "across-restart")
    p.plant(R + 1400, 4097, 258, "across-restart")
    p.plant(R + 5000, M, 128, "across-restart")
    p.plant(R - 100 + 1024, 1024, 259, "source-straddles-restart")
    # the data's ragged end
    _tail(p, 1, 4097, 33, "tail")
    # a source in the previous super-chunk (one block per workgroup: the
    # previous block), destinations in a block's first sub-chunk
    for j, (d, ln) in enumerate([(255, 33), (4097, 128), (16384, 258), (M, 259), (M - 1, 17), (1025, 9)]):
        p.place(d, ln, range((4 + j) * B + 4 * j + (0, 1, 2, 3, 64, 255)[j], (5 + j) * B, 1), "previous-super-chunk")
    # starts 1 .. 321 bytes before a sub-chunk end (not a block end)
    k = 0
    for off in (1, 3, 8, 257, 258, 319, 320, 321):
        for d, ln in ((8, 17), (4097, 259), (M - 1, 600), (1024, 33)):
            # (every other sub-chunk end: the sources, a sub-chunk or nearly a
            # block back, fall between the destinations)
            sub_end = (10 + k // 3) * B + (2 + 2 * (k % 3)) * S
            k += 1
            p.plant(sub_end - off, d, ln, "sub-chunk-end")
    # copies that straddle a block end: the length must be clipped there
    k = 0
    for off in (1, 3, 8, 100, 257):
        for d, ln in ((5, 16), (1025, 258), (M, 600), (16, 300)):
            if ln > off:
                p.plant((11 + k) * B - off, d, ln, "block-end")
                k += 1
    # 64-lane exchanges and 256-position super-steps
    at = 36 * S * 2
    for m, rs in ((64, (63, 64, 65)), (256, (255, 256, 257))):
        for r in rs:
            for d, ln in ((5, 9), (1025, 33), (M, 258), (17, 31)):
                at = p.place(d, ln, range(at + (r - at) % m, n, m), "mod-%d" % m) + 700
    # -- the sweep: every distance x every length x every residue mod 4 --
    at = 2 * B + 16
    runs = 0
    for d in dists:
        for ln in LENGTHS:
            for r in range(4):
                at = p.place(d, ln, range(at + (r - at) % 4, n, 4), "sweep")
                if d == 1:
                    # a run of one symbol, a different one per run: the runs'
                    # keys do not add up in one window (at most ALPHA_N runs)
                    p.buf[at - 1:at + ln] = ALPHA0 + runs % ALPHA_N
                    p.buf[at - 2] = ALPHA0 + (runs + 1) % ALPHA_N
                    p.buf[at + ln] = ALPHA0 + (runs + 1) % ALPHA_N
                    runs += 1
                at += ln + 40 + int(p.rng.randint(0, 400))
    assert at < g.segment - B, "the sweep stays inside the first segment"
    return p.data(), p.copies


def small(g, sub, n, e, seed, super_chunks=False):
    """A ragged input of n bytes: copies around its sub-chunk and block ends,
    one that ends e bytes before the data's end, and -- super_chunks: for runs
    with several blocks per workgroup -- copies whose sources lie in the
    previous super-chunk of four blocks."""
    B, S, M = g.block, sub, g.maxdist
    p = Planter(n, seed)
    _tail(p, e, 17 if e & 1 else 1025, 33 if n < 3 * S else 258, "tail")
    p.plant(S - 3, 255, 33, "sub-chunk-end")
    p.plant(2 * S - 258, 8, 200 if n < 3 * S else 600, "sub-chunk-end")
    if n > B:
        p.plant(B - 8, 1025, 258, "block-end")
    if super_chunks:
        for j, (d, ln) in enumerate([(255, 33), (4097, 128), (16384, 258), (M, 259), (M - 1, 17), (M + 1, 64)]):
            p.place(d, ln, range(4 * B + 300 * j + j, n, 1), "previous-super-chunk")
    at = S + 100
    for d in (1, 2, 5, 16, 17, 255, 1024):
        for ln in (3, 4, 7, 8, 9, 16, 31, 258):
            got = p.place(d, ln, range(at, n), "sweep", required=False)
            if got is not None:
                at = got + ln + 30 + int(p.rng.randint(0, 4))
    return p.data(), p.copies


def vocabulary_text(n, seed=5, words=192):
    """n bytes of words drawn evenly from a random vocabulary of lower-case
    words of 3..12 letters, single spaces between them: chains with many real
    candidates of differing lengths.  With 192 words a window of 28 KiB holds
    a word about 20 times (test_lz77_ref.py asserts the key multiplicity the
    reference reports)."""
    rng = np.random.RandomState(seed)
    vocab = [bytes(rng.randint(97, 123, size=rng.randint(3, 13)).astype(np.uint8)) for _ in range(words)]
    out = bytearray()
    while len(out) < n:
        out += vocab[rng.randint(0, words)] + b" "
    return bytes(out[:n])


def dictionary_case(g, sub, seed=9):
    """A preset dictionary shorter than a sub-chunk and two items whose copies
    have their sources in it: (dictionary, items, copies per item); a copy's
    src is negative, counted back from the item's start."""
    rng = np.random.RandomState(seed)
    dn = sub - 1000 - 3
    d = (rng.randint(0, ALPHA_N, size=dn) + ALPHA0).astype(np.uint8)
    items, copies = [], []
    for n, plan in ((40 * 1024 + 3, [(0, 50, 64), (700, 300, 258), (5000, 1000, 33), (20000, 1500, 128)]),
                    (sub + 904, [(100, 20, 258), (1500, 2000, 32)])):
        buf = (rng.randint(0, ALPHA_N, size=n) + ALPHA0).astype(np.uint8)
        cs = []
        for dst, s, ln in plan:
            buf[dst:dst + ln] = d[s:s + ln]
            if dst and buf[dst - 1] == d[s - 1]:
                buf[dst - 1] = ALPHA0 + (buf[dst - 1] - ALPHA0 + 1) % ALPHA_N
            if buf[dst + ln] == d[s + ln]:
                buf[dst + ln] = ALPHA0 + (buf[dst + ln] - ALPHA0 + 1) % ALPHA_N
            cs.append(Copy(s - dn, dst, dst + dn - s, ln, "dictionary"))
        items.append(buf.tobytes())
        copies.append(cs)
    return d.tobytes(), items, copies


def coverable(copies, g):
    """The copies a parse must cover at their own distance: 32 bytes or more,
    inside the window, destination inside one block, source inside the
    destination's segment."""
    return [c for c in copies
            if c.length >= 32 and c.dist <= g.maxdist and c.dst // g.block == (c.dst + c.length - 1) // g.block
            and (c.src < 0 or c.src >= c.dst // g.segment * g.segment)]


def forbidden(copies, g):
    """The copies no match may cover at their own distance: beyond the window,
    or with the whole source before the destination's segment."""
    return [c for c in copies
            if c.dist > g.maxdist or (c.src >= 0 and c.src + c.length <= c.dst // g.segment * g.segment)]


def covered(cover, c):
    """bytes of copy c that `cover` (the distance of the match over each
    position, 0: a literal) holds at the copy's own distance"""
    return int((cover[c.dst:c.dst + c.length] == c.dist).sum())
