"""block_kernel's code construction (huff_lengths: package-merge, huff_codes:
canonical codes) on histograms handed in through zt_debug_huffman, against
the plain package-merge of tests/huffman_ref.py.

A wrong code never shows from outside: block_kernel compares the dynamic
form's size with the fixed form's and emits the smaller, so the stream stays
valid and only the ratio suffers.  Here the lengths must be a complete code
within the limit whose cost is the optimum, exactly; on ties the lengths
themselves may differ from the reference's.

The hook rejects a frequency of 2^23 or more (the kernel's sort key is
freq << 9 | symbol in 32 bits) and a histogram summing to 2^27 or more."""
import random

import numpy as np
import pytest

import huffman_ref as hr

pytestmark = pytest.mark.gpu

PAIRS = [(286, 15), (30, 15), (19, 7)]
MANY = [272, 273, 274, 275, 285, 286]  # used symbols around 2m - 2 = 544: the 17-word bitmap rows' last bit


def fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def spread(values, n, rng=None):
    """`values` as the first frequencies of an n-symbol histogram, or at
    random positions."""
    h = [0] * n
    pos = list(range(n))
    if rng:
        rng.shuffle(pos)
    for p, v in zip(pos, values):
        h[p] = v
    return h


def histograms(n, limit):
    """[(name, histogram)] for one (n, limit) pair."""
    rng = random.Random(1000 * n + limit)
    out = [("none", [0] * n)]
    for p in (0, 1, n - 1):
        out.append(("one@%d" % p, spread([0] * p + [5], n)))
    out.append(("two", spread([3, 9], n, rng)))
    out.append(("two@ends", [7] + [0] * (n - 2) + [1]))
    out.append(("three", spread([3, 9, 4], n, rng)))
    k = 1
    while (1 << k) - 1 <= n:
        for m in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            if 2 <= m <= n and m <= (1 << limit):
                out.append(("equal%d" % m, spread([6] * m, n)))
                out.append(("equal%d/shuffled" % m, spread([6] * m, n, rng)))
        k += 1
    out.append(("equal%d" % n, [11] * n))
    for m in range(8, 31):
        if m <= n:
            out.append(("fib%d" % m, spread(fib(m), n)))
            out.append(("fib%d/shuffled" % m, spread(fib(m), n, rng)))
            out.append(("fib%d/descending" % m, spread(fib(m)[::-1], n)))
    out.append(("pow2", spread([1 << i for i in range(min(n, 22))], n)))
    out.append(("pow2/shuffled", spread([1 << i for i in range(min(n, 22))], n, rng)))
    out.append(("pow2+ones", [1 << (i % 16) if i % 3 == 0 else 1 for i in range(n)]))
    out.append(("ties2", [1 + (i % 2) for i in range(n)]))
    out.append(("ties3", [(1, 2, 4)[i % 3] for i in range(n)]))
    out.append(("ties/blocks", [1 + 3 * (i * 5 // n) for i in range(n)]))
    out.append(("big", [1 << 22] + [1] * (n - 1)))
    out.append(("big/last", [1] * (n - 1) + [1 << 22]))
    out.append(("big/sparse", spread([1 << 22, 1, 1, 2, (1 << 22) - 1], n, rng)))
    if n == 286:
        for m in MANY:
            tail = fib(24)
            out.append(("many%d/flat" % m, spread([40] * m, n, rng)))
            out.append(("many%d/pareto" % m, spread([1 + 200000 // (1 + i) ** 2 for i in range(m)], n, rng)))
            out.append(("many%d/fibtail" % m, spread([3] * (m - 24) + tail, n, rng)))
            out.append(("many%d/ordered" % m, spread([1 + 200000 // (1 + i) ** 2 for i in range(m)], n)))
    for i in range(200):
        kind = i % 4
        m = rng.randint(2, n)
        if kind == 0:
            v = [rng.randint(1, 1000) for _ in range(m)]
        elif kind == 1:
            v = [max(1, int(rng.paretovariate(0.7))) for _ in range(m)]
            v = [min(x, 1 << 18) for x in v]
        elif kind == 2:
            v = [rng.choice((1, 1, 2, 3, 50)) for _ in range(m)]
        else:
            v = [1 + int(30000 * rng.random() ** 6) for _ in range(n)]
        out.append(("random%d" % i, spread(v, n, rng)))
    return out


def bit_reverse(c, l):
    return int(format(c, "0%db" % l)[::-1], 2) if l else 0


@pytest.fixture(scope="module")
def zt():
    import ztamd

    return ztamd


@pytest.fixture(scope="module", params=PAIRS, ids=lambda p: "n%d-limit%d" % p)
def run(request, zt):
    """Every histogram of the pair through the hook in one call."""
    n, limit = request.param
    hs = histograms(n, limit)
    lens, codes = zt.debug_huffman(np.array([h for _, h in hs], dtype=np.uint32), n, limit)
    return n, limit, hs, lens.tolist(), codes.tolist()


def test_lengths(run):
    n, limit, hs, lens, _ = run
    bad = []
    for (name, f), l in zip(hs, lens):
        want = hr.package_merge(f, limit)
        forced = hr.two_symbol_rule(f)
        why = None
        if forced is not None:
            if l != forced:
                why = "two-symbol rule: %r" % ([i for i, x in enumerate(l) if x],)
        elif [x != 0 for x in l] != [x != 0 for x in f]:
            why = "lengths are not nonzero exactly where the frequencies are"
        elif max(l) > limit:
            why = "longest code %d" % max(l)
        elif hr.kraft_at(l, limit) != 1 << limit:
            why = "Kraft sum %d of %d" % (hr.kraft_at(l, limit), 1 << limit)
        elif hr.cost(f, l) != hr.cost(f, want):
            why = "cost %d, optimum %d" % (hr.cost(f, l), hr.cost(f, want))
        else:
            # a more frequent symbol never has the longer code
            # (per frequency, ascending: its shortest code is no shorter than
            # the longest code of any larger frequency)
            span = {}
            for x, y in zip(f, l):
                if x:
                    lo, hi = span.get(x, (y, y))
                    span[x] = (min(lo, y), max(hi, y))
            by_f = sorted(span.items())
            longest_above = 0
            for fa, (lo, hi) in reversed(by_f):
                if lo < longest_above:
                    why = "frequency %d has a %d-bit code, a larger one %d bits" % (fa, lo, longest_above)
                longest_above = max(longest_above, hi)
        if why:
            bad.append("%s (%d used): %s" % (name, sum(1 for x in f if x), why))
    assert not bad, "\n".join(bad)


def test_codes(run):
    n, limit, hs, lens, codes = run
    bad = []
    for (name, _), l, c in zip(hs, lens, codes):
        if hr.kraft_at(l, limit) > 1 << limit:
            bad.append("%s: over-subscribed lengths" % name)
            continue
        want = [(x << 16) | bit_reverse(cc, x) if x else 0 for x, cc in zip(l, hr.canonical_codes(l))]
        if c != want:
            bad.append("%s: codes differ from the canonical codes of the lengths" % name)
    assert not bad, "\n".join(bad)


def test_limit_binds():
    """The histograms do exceed the limit without it (else package-merge is
    never asked for more than Huffman), and the many-symbol set is there."""
    for n, limit in PAIRS:
        hs = histograms(n, limit)
        deep = [name for name, f in hs if name.startswith("fib") and hr.huffman_depth(f) > limit]
        assert any("/" not in name for name in deep), (n, limit)  # in symbol order
        assert any(name.endswith("/shuffled") for name in deep), (n, limit)
    used = {sum(1 for x in f if x) for name, f in histograms(286, 15) if name.startswith("many")}
    assert used == set(MANY)


def test_arguments(zt):
    ok = np.ones(19, dtype=np.uint32)
    zt.debug_huffman(ok, 19, 7)
    for f, n, limit in ((ok, 19, 8), (ok, 19, 0), (np.ones(287, dtype=np.uint32), 287, 15), (ok[:1], 1, 15),
                        (np.ones(200, dtype=np.uint32), 200, 7)):
        with pytest.raises(zt.ZtError) as e:
            zt.debug_huffman(f, n, limit)
        assert e.value.code == -103  # ZT_E_ARG
    # a frequency of 2^23; 17 (2^23 - 1) + 2 > 2^27
    for big in ([1 << 23] + [1] * 18, [(1 << 23) - 1] * 17 + [1] * 2):
        with pytest.raises(zt.ZtError) as e:
            zt.debug_huffman(np.array(big, dtype=np.uint32), 19, 15)
        assert e.value.code == -103  # ZT_E_ARG
