"""Plain-Python reference for the deflate block stage's Huffman decisions.

`package_merge` is the textbook algorithm (Larmore and Hirschberg) on lists
of (weight, symbols): nothing of the kernel's layout -- no sort key, no
bitmaps, no prefix counts -- so the two agree only if both are optimal.
`huffman_depth` is the depth of the unrestricted Huffman tree, which tells a
test whether a length limit binds at all.  canonical_codes, kraft and
rle_greedy come from deflate_builder.
"""
import heapq

from deflate_builder import canonical_codes, kraft, rle_greedy  # noqa: F401  (re-exported)


def two_symbol_rule(freq):
    """Lengths when fewer than two symbols are used, else None: a complete
    code needs two, so the used symbol and symbol 0 (symbol 1 when the used
    one is 0) get one bit each, symbols 0 and 1 when none is used."""
    used = [i for i, f in enumerate(freq) if f]
    if len(used) >= 2:
        return None
    lens = [0] * len(freq)
    if not used:
        lens[0] = lens[1] = 1
    else:
        lens[used[0]] = 1
        lens[1 if used[0] == 0 else 0] = 1
    return lens


def package_merge(freq, limit):
    """Optimal code lengths of at most `limit` bits for `freq` (0: unused)."""
    forced = two_symbol_rule(freq)
    if forced is not None:
        return forced
    used = [i for i, f in enumerate(freq) if f]
    m = len(used)
    if m > (1 << limit):
        raise ValueError("%d symbols do not fit %d bits" % (m, limit))
    items = sorted(((freq[i], (i,)) for i in used), key=lambda t: (t[0], t[1]))
    level = list(items)
    for _ in range(limit - 1):
        packages = [(level[k][0] + level[k + 1][0], level[k][1] + level[k + 1][1])
                    for k in range(0, len(level) - 1, 2)]
        # stable: an item goes before a package of the same weight
        level = sorted(items + packages, key=lambda t: t[0])
    lens = [0] * len(freq)
    for _, syms in level[:2 * m - 2]:
        for s in syms:
            lens[s] += 1
    return lens


def cost(freq, lens):
    return sum(f * l for f, l in zip(freq, lens))


def huffman_depth(freq):
    """Longest code of the unrestricted Huffman tree over the used symbols."""
    heap = [(f, 0) for f in freq if f]
    if len(heap) < 2:
        return 1
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def kraft_at(lens, limit):
    """Sum of 2^(limit - l) over the used symbols: 2^limit is a complete code."""
    return sum(1 << (limit - l) for l in lens if l)
