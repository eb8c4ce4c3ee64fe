"""tests/lz77_ref.py against itself and by hand, and the match audit's inputs
(tests/match_audit_inputs.py) against the reference -- all on the CPU: the
join on the 8-byte key equals the obvious double loop, the window and max_len
rules hold at their edges, every planted copy measures exactly its length, and
a greedy parse over the reference's matches covers every planted copy whole
(the ground truth of test_gpu_match_audit.py's stream-level check)."""
import numpy as np
import pytest

import lz77_ref as ref
import match_audit_inputs as inputs
from lz77_ref import Geom

# The geometry of the shipped build, for inputs shaped as the GPU audit's are;
# the GPU audit reads its own from the library (ztamd.debug_match).
NOMINAL, NOMINAL_SUB = Geom(block=32768, segment=1 << 20, maxdist=28352), 4096
SMALL = Geom(block=256, segment=1024, maxdist=200)


def text():
    rng = np.random.RandomState(1)
    words = [b"compress", b"compression", b"press", b"window", b"windowed", b"the", b"chain of", b"hash chain"]
    return b" ".join(words[rng.randint(0, len(words))] for _ in range(400))


CASES = {
    "text": (text()[:2000], Geom(4096, 1 << 20, 500), 0),
    "period5": ((b"\x01\x7fab\xf0" * 500)[:1003], Geom(4096, 1 << 20, 150), 0),
    "zeros": (bytes(800), Geom(4096, 1 << 20, 100), 0),
    # block ends every 256 bytes clip lengths, segment starts every 1024 cut windows
    "block-and-segment-ends": (text()[:2500], SMALL, 0),
    "halo": (text()[:2000], SMALL, 300),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_keyed_equals_naive_from_eight_bytes(name):
    data, g, halo = CASES[name]
    best, dist, mult = ref.longest_keyed(data, g, halo)
    n = len(data) - halo
    assert best.size == n
    checked = 0
    for i in range(n):
        ln, d = ref.longest_naive(data, i, g, halo)
        if ln >= ref.KEY:
            assert (int(best[i]), int(dist[i])) == (ln, d), "position %d" % i
            checked += 1
        else:
            assert best[i] == 0 and dist[i] == 0, "position %d" % i
    assert checked > n // 4
    assert mult >= 2


def test_multiplicity_counts_one_key_inside_a_window():
    g = Geom(4096, 1 << 20, 100)
    # zeros: a position and its 100 candidates share one key
    assert ref.longest_keyed(bytes(1000), g)[2] == 101
    rng = np.random.RandomState(2)
    assert ref.longest_keyed(rng.randint(0, 256, 5000).astype(np.uint8).tobytes(), g)[2] == 1


def planted(n, src, dst, length, seed=3):
    b = np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8)
    b[dst:dst + length] = b[src:src + length]
    b[src - 1], b[dst - 1] = 1, 2
    if dst + length < n:
        b[src + length], b[dst + length] = 3, 4
    return b.tobytes()


def test_window_edge_by_hand():
    g = Geom(4096, 1 << 20, 1000)
    for d, found in ((1000, True), (1001, False)):
        data = planted(3000, 500, 500 + d, 40)
        best, dist, _ = ref.longest_keyed(data, g)
        if found:
            assert ref.longest_naive(data, 500 + d, g) == (40, d)
        else:
            assert ref.longest_naive(data, 500 + d, g)[0] < ref.KEY
        assert (int(best[500 + d]), int(dist[500 + d])) == ((40, d) if found else (0, 0))
        # (the next position's source is as far: in the window only where the first one's is)
        assert int(best[500 + d + 1]) == (39 if found else 0)
    assert ref.window_start(2000, g) == 1000 and ref.window_start(999, g) == 0


def test_source_straddles_the_segment_start_by_hand():
    g = Geom(1024, 1024, 900)
    # source 1014 .. 1054, destination 1514 ..: the first 10 source bytes lie before segment 1
    data = planted(2500, 1014, 1514, 40)
    best, dist, _ = ref.longest_keyed(data, g)
    for k in range(40):
        want = (40 - k, 500) if k >= 10 and 40 - k >= ref.KEY else (0, 0)
        assert (int(best[1514 + k]), int(dist[1514 + k])) == want, k
        if 40 - k >= ref.KEY:
            ln, d = ref.longest_naive(data, 1514 + k, g)
            assert (ln, d) == (40 - k, 500) if k >= 10 else ln < ref.KEY
    assert ref.window_start(1514, g) == 1024 and ref.window_start(1023, g) == 123
    # with a halo the first segment's window reaches into the halo, later ones start at their own first byte
    assert ref.window_start(5, g, halo=300) == 0 and ref.window_start(1030, g, halo=300) == 1324


def test_max_len_is_clipped_by_the_block_end_and_the_data_end_by_hand():
    g = Geom(256, 1024, 900)
    assert ref.max_len(0, 10000, Geom(4096, 1 << 20, 900)) == 258
    assert ref.max_len(250, 10000, g) == 6 and ref.max_len(256, 10000, g) == 256
    assert ref.max_len(256, 300, g) == 44
    # a 100-byte copy whose destination starts 30 bytes before a block end
    data = planted(2000, 100, 482, 100)
    best, dist, _ = ref.longest_keyed(data, g)
    assert (int(best[482]), int(dist[482])) == (30, 382)
    assert int(best[482 + 23]) == 0  # (7 bytes to the block end: below the key)
    assert (int(best[512]), int(dist[512])) == (70, 382)


# ---- the audit's inputs ----
@pytest.fixture(scope="module")
def matrix():
    data, copies = inputs.matrix(NOMINAL, NOMINAL_SUB)
    best, dist, mult = ref.longest_keyed(data, NOMINAL)
    return data, copies, best, dist, mult


def exact(data, copies, best, dist, g):
    """every copy inside the window and its segment measures exactly its length"""
    n, checked = len(data), 0
    for c in copies:
        if c.dist > g.maxdist or c.src < c.dst // g.segment * g.segment:
            continue
        want = min(c.length, ref.max_len(c.dst, n, g))
        if want >= ref.KEY:
            assert int(best[c.dst]) == want, c
            # (an overlapping copy repeats at every multiple of its distance: the nearest wins)
            assert int(dist[c.dst]) == c.dist, c
            checked += 1
        else:
            assert best[c.dst] == 0, c
    return checked


def test_matrix_holds_every_case(matrix):
    data, copies, best, dist, mult = matrix
    g = NOMINAL
    assert len(data) == g.segment + 40 * 1024 + 37
    sweep = {(c.dist, c.length, c.dst % 4) for c in copies if c.tag == "sweep"}
    assert sweep == {(d, ln, r) for d in inputs.DISTANCES(g) for ln in inputs.LENGTHS for r in range(4)}
    assert any(c.length > c.dist for c in copies)
    for m, rs in ((64, (63, 0, 1)), (256, (255, 0, 1))):
        assert {c.dst % m for c in copies if c.tag == "mod-%d" % m} == set(rs)
    ends = {(-c.dst) % NOMINAL_SUB for c in copies if c.tag == "sub-chunk-end"}
    assert ends == {1, 3, 8, 257, 258, 319, 320, 321}
    assert all(c.dst // g.block != (c.dst + c.length - 1) // g.block for c in copies if c.tag == "block-end")
    assert all(c.src // g.block == c.dst // g.block - 1 and c.dst % g.block < NOMINAL_SUB
               for c in copies if c.tag == "previous-super-chunk")
    assert all(c.src + c.length <= g.segment < c.dst for c in copies if c.tag == "across-restart")
    assert all(c.src < g.segment < c.src + c.length for c in copies if c.tag == "source-straddles-restart")
    assert any(c.dst + c.length == len(data) for c in copies if c.tag == "tail")
    assert exact(data, copies, best, dist, g) > 800
    # nothing is found across the restart point, and of the straddling source only its part inside
    for c in copies:
        if c.tag == "across-restart":
            assert not best[c.dst:c.dst + c.length].any()
        if c.tag == "source-straddles-restart":
            k = g.segment - c.src
            assert not best[c.dst:c.dst + k].any() and int(best[c.dst + k]) == c.length - k


def test_filler_blocks_stay_searched_and_keys_unique(matrix):
    data, copies, best, dist, mult = matrix
    b = np.frombuffer(data, dtype=np.uint8)
    for lo in range(0, b.size, NOMINAL.block):
        f = np.bincount(b[lo:lo + NOMINAL.block], minlength=256).astype(float)
        f = f[f > 0] / f.sum()
        assert -(f * np.log2(f)).sum() < 6.05
    # outside the planted copies no position has a candidate
    planted_at = np.zeros(b.size, dtype=bool)
    for c in copies:
        planted_at[c.dst:c.dst + c.length] = True
    assert not best[~planted_at].any()


def test_greedy_parse_over_the_reference_covers_every_copy(matrix):
    data, copies, best, dist, mult = matrix
    cover = ref.greedy_cover(best, dist)
    must = inputs.coverable(copies, NOMINAL)
    assert len(must) > 300
    for c in must:
        # (matches end at 258 bytes: a last piece shorter than the key is left to literals)
        rest = c.length % ref.MAX_MATCH
        assert inputs.covered(cover, c) == c.length - (rest if rest < ref.KEY else 0), c
    never = inputs.forbidden(copies, NOMINAL)
    assert len(never) >= 2 * 16 * 4 + 3
    for c in never:
        assert inputs.covered(cover, c) == 0, c


@pytest.mark.parametrize("n,e,seed,sup", [(160 * 1024 + 511, 2, 21, True), (8192 + 1, 3, 22, False),
                                          (8192 + 63, 5, 23, False), (8192 + 513, 8, 24, False)])
def test_small_inputs(n, e, seed, sup):
    data, copies = inputs.small(NOMINAL, NOMINAL_SUB, n, e, seed, sup)
    assert len(data) == n
    best, dist, mult = ref.longest_keyed(data, NOMINAL)
    assert exact(data, copies, best, dist, NOMINAL) >= 20
    assert any(c.dst + c.length == n - (e - 1) for c in copies if c.tag == "tail")
    if sup:
        assert sum(1 for c in copies if c.tag == "previous-super-chunk" and c.src < 4 * NOMINAL.block <= c.dst) == 6


def test_vocabulary_text_has_low_multiplicity():
    data = inputs.vocabulary_text(96 * 1024 + 13)
    best, dist, mult = ref.longest_keyed(data, NOMINAL)
    assert 8 <= mult <= 64
    assert (best >= ref.KEY).mean() > 0.3
    assert len(set(best.tolist())) > 8  # (candidates of differing lengths)


def test_dictionary_case():
    d, items, copies = inputs.dictionary_case(NOMINAL, NOMINAL_SUB)
    assert len(d) < NOMINAL_SUB
    for item, cs in zip(items, copies):
        best, dist, _ = ref.longest_keyed(d + item, NOMINAL, halo=len(d))
        for c in cs:
            assert (int(best[c.dst]), int(dist[c.dst])) == (c.length, c.dist), c
        assert len(inputs.coverable(cs, NOMINAL)) == len(cs)


def test_nearest_same_prefix_by_hand():
    near = ref.nearest_same_prefix(b"abcdXabcdYabcZabcdabc", 4)
    assert near.tolist() == [0, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 9, 0, 0, 0, 0, 0, 0]
    assert ref.nearest_same_prefix(bytes(6), 4).tolist() == [0, 1, 1, 0, 0, 0]
