"""A brute-force LZ77 reference for the deflate match stage.

What the match kernel (csrc/deflate.hip) should find at a position, stated
without its hash tables, chains or work split: the candidate window, the
longest length a match may have there, and the longest match among the
candidates.  Pure Python and numpy.

Positions count from the stream's first byte.  `data` holds `halo` bytes of
history in front of the stream (the multi-GPU shard case), so position i is
data[halo + i].  The geometry -- block, segment and window sizes -- is a
parameter: the GPU tests take it from the library (ztamd.debug_match), the CPU
tests also run reduced ones.

The candidates q of a position i are the positions with
  * q < i,
  * i - q <= maxdist,
  * q not before the start of i's segment; the stream's first segment starts
    at data[0]: at the stream's start with halo = 0, else at the halo's first
    byte (the window reaches into the halo),
and a match at i is at most max_len(i) = min(258, end of i's block - i, end of
the data - i) long.
"""
from collections import namedtuple

import numpy as np

Geom = namedtuple("Geom", "block segment maxdist")
MAX_MATCH = 258
KEY = 8  # longest_keyed joins on this many bytes (the chains' key length)


def _array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data


def window_start(i, g, halo=0):
    """The first candidate of position i, as an index into data."""
    a = halo + i
    seg = i // g.segment
    seg_lo = 0 if seg == 0 else halo + seg * g.segment
    return max(a - g.maxdist, seg_lo)


def max_len(i, n, g):
    """The longest match position i of an n-byte stream may hold."""
    return min(MAX_MATCH, (i // g.block + 1) * g.block - i, n - i)


def longest_naive(data, i, g, halo=0):
    """(length, distance) of the longest match at position i, the nearest of
    equal length; (0, 0) when no candidate shares a byte.  The obvious double
    loop: for tiny inputs."""
    d = _array(data)
    n = d.size - halo
    a, ml = halo + i, max_len(i, n, g)
    best, dist = 0, 0
    for q in range(a - 1, window_start(i, g, halo) - 1, -1):
        eq = d[q:q + ml] == d[a:a + ml]
        k = ml if eq.all() else int(eq.argmin())  # (the first unequal byte)
        if k > best:
            best, dist = k, a - q
    return best, dist


def _keys(d):
    """key[a] = the KEY bytes at a as one integer, for every a (zero past the end)."""
    p = np.concatenate([d, np.zeros(KEY, dtype=np.uint8)]).astype(np.uint64)
    k = np.zeros(d.size, dtype=np.uint64)
    for b in range(KEY):
        k |= p[b:b + d.size] << np.uint64(8 * b)
    return k


def longest_keyed(data, g, halo=0):
    """For every position i: L*(i), the longest common prefix, at most
    max_len(i), over the candidates that share their first KEY bytes with i
    (0 when none does or max_len(i) < KEY), and the distance of the nearest
    candidate of that length.  Returns (length uint16[n], distance
    uint32[n], mult): mult is the largest number of occurrences of one key
    inside any window -- a position and its candidates of the same key.

    A join on the key: the positions sorted by (key, position); candidates of
    a position are its predecessors in its key's run, nearest first."""
    d = _array(data)
    n = d.size - halo
    key = _keys(d)
    # bytes past the end compare unequal to everything before them
    pad = np.concatenate([d.astype(np.int16), np.full(MAX_MATCH + KEY, -1, dtype=np.int16)])
    order = np.argsort(key, kind="stable")  # (stable: positions ascend inside a key's run)
    skey = key[order]
    pos = np.arange(n, dtype=np.int64)
    ml = np.minimum(np.minimum(MAX_MATCH, (pos // g.block + 1) * g.block - pos), n - pos)
    seg = pos // g.segment
    lo = np.maximum(halo + pos - g.maxdist, np.where(seg == 0, 0, halo + seg * g.segment))
    best = np.zeros(n, dtype=np.uint16)
    dist = np.zeros(n, dtype=np.uint32)
    count = np.ones(n, dtype=np.int64)
    # pairs (order[j - k], order[j]) of one key, k = 1, 2, ...: the k-th nearest
    # earlier occurrence; a run's distances grow with k, so the loop ends when
    # no pair is left inside its window
    # (j: the sorted indices whose k - 1 nearest predecessors were all of
    # their key and inside their window; only those can have a k-th)
    j = np.nonzero(order >= halo)[0]  # (the halo's bytes are candidates, not positions)
    k = 0
    while j.size:
        k += 1
        j = j[j >= k]
        j = j[skey[j] == skey[j - k]]
        j = j[order[j - k] >= lo[order[j] - halo]]
        a, q = order[j], order[j - k]
        count[a - halo] += 1
        ok = ml[a - halo] >= KEY
        a, q = a[ok], q[ok]
        i = a - halo
        ln = np.full(a.size, KEY, dtype=np.int64)
        # (whole keys while KEY more bytes fit below max_len, then single bytes)
        live = np.arange(a.size)
        while live.size:
            lv = ln[live]
            live = live[lv + KEY <= ml[i[live]]]
            lv = ln[live]
            live = live[key[a[live] + lv] == key[q[live] + lv]]
            ln[live] += KEY
        live = np.arange(a.size)
        while live.size:
            lv = ln[live]
            go = (lv < ml[i[live]]) & (pad[a[live] + lv] == pad[q[live] + lv])
            live = live[go]
            ln[live] += 1
        better = ln > best[i]  # (nearest first: an equal length keeps the nearer)
        best[i[better]] = ln[better]
        dist[i[better]] = (a - q)[better]
    return best, dist, int(count.max()) if n else 0


def nearest_same_prefix(data, k=4):
    """For every index a of data: the distance to the nearest earlier index
    whose first k <= KEY bytes equal a's (0: none, or fewer than k bytes left)."""
    d = _array(data)
    key = _keys(d) & np.uint64((1 << (8 * k)) - 1)
    order = np.argsort(key, kind="stable")
    same = key[order[1:]] == key[order[:-1]]
    near = np.zeros(d.size, dtype=np.int64)
    near[order[1:][same]] = (order[1:] - order[:-1])[same]
    near[max(d.size - k + 1, 0):] = 0
    return near


def greedy_cover(best, dist):
    """A greedy parse over longest_keyed's matches: at a position with a match
    take it whole, else step one byte.  Returns dist_at int64[n]: the distance
    of the match that covers each position, 0 for a literal."""
    n = best.size
    cover = np.zeros(n, dtype=np.int64)
    i = 0
    while i < n:
        if best[i]:
            cover[i:i + int(best[i])] = int(dist[i])
            i += int(best[i])
        else:
            i += 1
    return cover
