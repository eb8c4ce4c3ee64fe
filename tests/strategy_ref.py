"""The deflate strategies' per-position words, restated in numpy.

What strategy_kernel (csrc/deflate_strategy.hip) must write for a stream, with
none of its chunks, break bits or LDS: the definition of include/zt_strategy.h.

`data` holds `halo` bytes of history in front of the stream, so position i is
data[halo + i].  The geometry is lz77_ref's Geom (block, segment; maxdist is
not used): the GPU tests take it from the library (ztamd.debug_match_strategy),
the CPU tests also run reduced ones.

  lo(i)      the first byte position i may reference: the stream's first byte;
             the halo's first byte for segment 0 with halo > 0; the start of
             i's segment for later segments
  run_end(i) the smallest j > i with byte[j] != byte[i], or n
  cap(i)     min(258, (i // block + 1) * block - i, n - i)
  L(i)       min(cap(i), run_end(i) - i) if i - 1 >= lo(i) and byte[i] ==
             byte[i - 1], else 0; L < 3 becomes 0
  word(i)    byte << 24 | L << 15 | (1 if L else 0)       (RLE)
             byte << 24                                   (Huffman-only)

A batch item is a stream of its own (halo 0): its bounds are the item's.
"""
import numpy as np

MAX_MATCH = 258
HUFFMAN_ONLY, RLE = 2, 3  # zlib's Z_HUFFMAN_ONLY, Z_RLE


def _array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data


def rle_lengths(data, g, halo=0):
    """L(i) for every position of the stream, int64[n]."""
    d = _array(data)
    s = d[halo:].astype(np.int64)
    n = s.size
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    i = np.arange(n, dtype=np.int64)
    # byte[i] == byte[i - 1], where i - 1 >= lo(i)
    same = np.zeros(n, dtype=bool)
    same[1:] = s[1:] == s[:-1]
    same[(i % g.segment == 0) & (i > 0)] = False
    same[0] = halo > 0 and int(d[halo - 1]) == int(s[0])
    # run_end: the next position whose byte differs from the one in front of it
    brk = np.full(n + 1, n, dtype=np.int64)
    brk[1:n][s[1:] != s[:-1]] = i[1:][s[1:] != s[:-1]]
    nxt = np.minimum.accumulate(brk[::-1])[::-1]  # nxt[j] = the first break at or after j
    run = nxt[1:] - i
    cap = np.minimum(np.minimum(MAX_MATCH, (i // g.block + 1) * g.block - i), n - i)
    length = np.where(same, np.minimum(cap, run), 0)
    length[length < 3] = 0
    return length


def rle_words(data, g, halo=0):
    """The RLE strategy's res words, uint32[n]."""
    d = _array(data)
    length = rle_lengths(d, g, halo).astype(np.uint32)
    return (d[halo:].astype(np.uint32) << 24) | (length << 15) | (length > 0).astype(np.uint32)


def huffman_words(data, halo=0):
    """The Huffman-only strategy's res words, uint32[n]."""
    return _array(data)[halo:].astype(np.uint32) << 24


def words(strategy, data, g, halo=0):
    return rle_words(data, g, halo) if strategy == RLE else huffman_words(data, halo)


def token_positions(blocks):
    """[(position, token)] of the blocks deflate_audit.parse returned: a literal
    token is an int, a match (length, distance[, True])."""
    out, p = [], 0
    for b in blocks:
        for t in b.tokens:
            out.append((p, t))
            p += t[0] if isinstance(t, tuple) else 1
    return out


def check_tokens(strategy, blocks, data, g, halo=0):
    """The token rules of a strategy's stream: Huffman-only holds no match;
    every RLE match at p is (l, 1) with 3 <= l <= L(p).  Returns the number of
    matches."""
    length = rle_lengths(data, g, halo) if strategy == RLE else None
    matches = 0
    for p, t in token_positions(blocks):
        if not isinstance(t, tuple):
            continue
        matches += 1
        assert strategy == RLE, "match token %r at %d of a Huffman-only stream" % (t, p)
        assert t[1] == 1 and 3 <= t[0] <= length[p], "token %r at %d, L = %d" % (t, p, length[p])
    return matches


# ---- inputs ---------------------------------------------------------------------
RUN_LENGTHS = (1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517)


def no_repeats(n, seed):
    """n bytes, no two adjacent ones equal."""
    rng = np.random.default_rng(seed)
    step = rng.integers(1, 256, size=n, dtype=np.int64)  # never 0: every byte differs from the one before
    return (np.cumsum(step) % 256).astype(np.uint8)


def run_structured(n, seed, alphabet=4, mean=6):
    """Runs of random lengths (many below 3, some beyond 258) over a small alphabet."""
    rng = np.random.default_rng(seed)
    out = []
    total = 0
    while total < n:
        k = int(rng.geometric(1.0 / mean))
        if rng.integers(0, 40) == 0:
            k += int(rng.integers(200, 700))
        out.append(np.full(k, rng.integers(0, alphabet), dtype=np.uint8))
        total += k
    return np.concatenate(out)[:n]


class Planter:
    """Runs planted into a background without adjacent equal bytes: a run of
    `length` at p takes a value that differs from both of its neighbours, so
    it is exactly that long.  Runs keep a byte of background between them."""

    def __init__(self, n, seed):
        self.d = no_repeats(n, seed)
        self.used = np.zeros(n + 2, dtype=bool)  # index p + 1
        self.runs = []

    def plant(self, p, length):
        n = self.d.size
        if p < 0 or p + length > n or self.used[p:p + length + 2].any():
            return False
        before = int(self.d[p - 1]) if p > 0 else -1
        after = int(self.d[p + length]) if p + length < n else -1
        v = next(x for x in range(256) if x != before and x != after)
        self.d[p:p + length] = v
        self.used[p + 1:p + length + 1] = True
        self.runs.append((p, length))
        return True

    def must(self, p, length):
        assert self.plant(p, length), "no room for a run of %d at %d" % (length, p)


def straddles(length):
    """How many bytes of a run of `length` lie in front of a boundary it straddles."""
    mid = (length // 2,) if length in (258, 517) else ()
    return sorted({j for j in (1, length - 1) + mid if 0 < j < length})


def matrix(block, seed=7):
    """One buffer with every RUN_LENGTHS run (a) starting -- and so ending -- on
    every offset of a 16-byte chunk, (b) straddling a multiple of 1024 inside
    a block, (c) straddling a block end.  Returns (bytes, runs)."""
    cases = [(ln, j) for ln in RUN_LENGTHS for j in straddles(ln)]
    nblocks = len(cases) + 3
    p = Planter(nblocks * block, seed)
    for k, (ln, j) in enumerate(cases):  # (c) block end k + 1
        p.must((k + 1) * block - j, ln)
    for k, (ln, j) in enumerate(cases):  # (b) 1024-byte spans well inside block k
        p.must(k * block + 1024 * (4 + 2 * (k % 8)) - j, ln)
    at = len(cases) * block + 1024  # (a) behind them
    for ln in RUN_LENGTHS:
        for off in range(16):
            q = at + 2
            q += (off - q) % 16
            p.must(q, ln)
            at = q + ln
    assert at <= p.d.size
    return p.d, p.runs
