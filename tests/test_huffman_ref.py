"""The Huffman reference (tests/huffman_ref.py) checked against brute force
and against zlib, so that the GPU tests compare the kernels with something
that is itself known to be optimal."""
import itertools
import zlib

import numpy as np
import pytest

import deflate_audit
import huffman_ref as hr
from audit_inputs import dense_input, oracle_input


def complete_assignments(m, limit):
    """Every ordered assignment of lengths 1..limit to m symbols whose Kraft
    sum is exactly one."""
    rows = [a for a in itertools.product(range(1, limit + 1), repeat=m)
            if sum(1 << (limit - l) for l in a) == (1 << limit)]
    return np.array(rows, dtype=np.int64).reshape(len(rows), m)


@pytest.mark.parametrize("limit", [2, 3, 4])
def test_package_merge_is_optimal_on_every_small_alphabet(limit):
    """Alphabets of up to 7 symbols, frequencies 0..4.  A zero frequency only
    removes the symbol (checked on the full 0..4 grid up to 5 symbols, where
    the two-symbol rule is checked too); the used symbols, in order, run over
    every tuple of 1..4."""
    for m in range(2, 8):
        freqs = list(itertools.product(range(1, 5), repeat=m))
        if m > (1 << limit):
            with pytest.raises(ValueError):
                hr.package_merge(freqs[0], limit)
            continue
        A = complete_assignments(m, limit)
        assert len(A)
        best = (np.array(freqs, dtype=np.int64) @ A.T).min(axis=1)
        for f, want in zip(freqs, best):
            lens = hr.package_merge(f, limit)
            assert max(lens) <= limit and min(lens) >= 1, (f, lens)
            assert hr.kraft_at(lens, limit) == 1 << limit, (f, lens)
            assert hr.cost(f, lens) == want, (f, lens, int(want))


@pytest.mark.parametrize("limit", [2, 3, 4])
def test_package_merge_with_unused_symbols(limit):
    for n in range(2, 6):
        for f in itertools.product(range(5), repeat=n):
            used = [i for i in range(n) if f[i]]
            if len(used) > (1 << limit):
                continue
            lens = hr.package_merge(f, limit)
            if len(used) >= 2:
                compact = hr.package_merge([f[i] for i in used], limit)
                assert [lens[i] for i in used] == compact, f
                assert all(lens[i] == 0 for i in range(n) if not f[i]), f
            elif len(used) == 1:
                other = 1 if used[0] == 0 else 0
                assert lens == [1 if i in (used[0], other) else 0 for i in range(n)], f
            else:
                assert lens == [1, 1] + [0] * (n - 2), f


def test_huffman_depth():
    assert hr.huffman_depth([1, 1]) == 1
    assert hr.huffman_depth([1, 1, 1, 1]) == 2
    assert hr.huffman_depth([0, 5, 0]) == 1
    fib = [1, 1, 2, 3, 5, 8, 13, 21]
    assert hr.huffman_depth(fib) == 7
    # where no limit binds, package-merge is Huffman: same cost, same depth
    for f in ([3, 1, 4, 1, 5, 9, 2, 6], fib, list(range(1, 40))):
        lens = hr.package_merge(f, 15)
        assert max(lens) == hr.huffman_depth(f)


@pytest.mark.parametrize("name", ["dense", "wordsalad"])
def test_package_merge_matches_zlib_cost(name):
    """zlib builds a Huffman tree and repairs it when it exceeds the limit
    (not optimal then); where its longest code stayed below the limit, its
    tree is an unrestricted optimum and the costs must agree."""
    data = dense_input() if name == "dense" else oracle_input("wordsalad")
    checked = 0
    for level in (1, 6, 9):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        stream = c.compress(data) + c.flush()
        for b in deflate_audit.parse(stream):
            if b.btype != 2:
                continue
            for hist, lens, limit in ((b.lit_hist, b.lit_lens, 15), (b.dist_hist, b.dist_lens, 15),
                                      (b.cl_hist, b.cl_lens, 7)):
                lens = list(lens) + [0] * (len(hist) - len(lens))
                if max(lens) >= limit or sum(1 for f in hist if f) < 2:
                    continue  # zlib may have hit its limit / coded an unused symbol
                if any(l and not f for l, f in zip(lens, hist)):
                    continue
                assert hr.cost(hist, hr.package_merge(hist, limit)) == hr.cost(hist, lens), (name, level, limit)
                checked += 1
    assert checked >= 6
