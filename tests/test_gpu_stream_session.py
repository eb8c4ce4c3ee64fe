"""Inflate sessions (include/zt_stream.h; ztamd.InflateSession,
ztamd.inflate_sessions_feed): raw inflate fed piece by piece -- only the new
bytes each time -- that resumes at a token and keeps its state on the device.

The yardstick for what a prefix can yield is CPU zlib:
``zlib.decompressobj(-15).decompress(prefix)`` returns every byte decodable
from ``prefix``.  After a feed history ending at cut ``c``, with ``acc`` the
concatenation of the outputs so far, every test asserts

    len(zlib_prefix(s[:max(0, c - 8)])) <= len(acc) and data.startswith(acc)

(8 bytes: the repository's convention for "may still be running out of
input"; it also covers the widest token, 48 bits)."""
import random
import zlib

import pytest

from deflate_builder import Stream

pytestmark = pytest.mark.gpu

ZT_E_INPUT_BROKEN, ZT_E_UNKNOWN_BTYPE, ZT_E_INVALID_DISTANCE, ZT_E_ARG = -10, -12, -15, -103
KINDS = ["zlib6", "zlib1", "stored", "fixed", "huffman_only", "reference", "engine"]


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8, zdict=None):
    if zdict is None:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    else:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy, zdict)
    return c.compress(data) + c.flush()


def zlib_prefix(prefix):
    return zlib.decompressobj(-15).decompress(prefix)


def make_stream(oracle, kind, data):
    import ztamd

    if kind == "zlib6":
        return raw(data, 6)
    if kind == "zlib1":
        return raw(data, 1, mem=1)  # small blocks (128-symbol buffer)
    if kind == "stored":
        return raw(data, 0)
    if kind == "fixed":
        return raw(data, 6, zlib.Z_FIXED)
    if kind == "huffman_only":
        return raw(data, 6, zlib.Z_HUFFMAN_ONLY)
    if kind == "reference":
        return oracle.raw_deflate(data)[0]  # one block for the whole input
    assert kind == "engine"
    return ztamd.deflate_raw(data, level=6)


@pytest.fixture(scope="module")
def mixed(oracle):
    text = oracle.gen("wordsalad", 11, 400_000)
    return text[:150_000] + oracle.gen("xorshift32", 11, 70_000) + oracle.gen("structured", 11, 120_000)


def check_bound(s, data, cut, acc):
    assert data.startswith(acc), cut
    need = len(zlib_prefix(s[:max(0, cut - 8)]))
    assert need <= len(acc), (cut, need, len(acc))


def work_is_linear(info):
    """Every launch reads what it decodes plus at most one partial header (below
    1 KiB): the work is linear in the input, by a counter and not by a clock."""
    assert info["decoded_bits"] <= info["end_bits"] + info["launches"] * 8 * 1024, info


@pytest.mark.parametrize("kind", KINDS)
def test_pieces_equal_whole(oracle, mixed, kind):
    import ztamd

    data = mixed[:200_000] if kind == "reference" else mixed
    s = make_stream(oracle, kind, data)
    rng = random.Random(zlib.crc32(kind.encode()))
    cuts = sorted(set(rng.randrange(1, len(s)) for _ in range(16))) + [len(s)]
    acc, prev, nonempty = b"", 0, 0
    with ztamd.InflateSession() as ses:
        for k, cut in enumerate(cuts):
            part = ses.feed(s[prev:cut], last=cut == len(s))
            prev = cut
            acc += part
            nonempty += bool(part)
            check_bound(s, data, cut, acc)
            if k == 7:
                assert ses.crc32 == zlib.crc32(acc) and ses.adler32 == zlib.adler32(acc)
        info = ses.info()
        assert acc == data
        assert ses.finished and ses.unused == 0
        assert ses.crc32 == zlib.crc32(data) and ses.adler32 == zlib.adler32(data)
        assert info["total_in"] == len(s) and info["total_out"] == len(data) and info["pending"] == 0
        assert (info["end_bits"] + 7) // 8 == len(s)
    if kind == "reference":
        # one block: a decoder that resumes at block boundaries returns nothing before the end
        assert nonempty >= len(cuts) - 2
    work_is_linear(info)


def test_one_byte_per_feed(oracle):
    """Dynamic headers that arrive over dozens of feeds: a partial header stays
    pending (it is read again from its start), and the pending tail stays
    below 1 KiB."""
    import ztamd

    head = oracle.gen("wordsalad", 6, 6000)
    data = oracle.gen("wordsalad", 5, 3000) + oracle.gen("xorshift32", 5, 500)
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    s = c.compress(head) + c.flush(zlib.Z_FULL_FLUSH)  # one dynamic block of level 9 in front
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    # many small blocks: a block boundary every 400 input bytes
    s += b"".join(c.compress(data[i:i + 400]) + c.flush(zlib.Z_FULL_FLUSH if i % 800 else zlib.Z_SYNC_FLUSH)
                  for i in range(0, len(data), 400)) + c.flush()
    data = head + data
    assert zlib.decompress(s, -15) == data
    acc = b""
    with ztamd.InflateSession() as ses:
        for i in range(len(s)):
            acc += ses.feed(s[i:i + 1], last=i == len(s) - 1)
            assert ses.info()["pending"] <= 1024
            if i % 97 == 0:
                check_bound(s, data, i + 1, acc)
        assert acc == data and ses.finished and ses.unused == 0
        assert ses.crc32 == zlib.crc32(data)


def far_match_stream():
    rng = random.Random(7)
    r = [rng.randrange(256) for _ in range(32768)]
    s = Stream()
    s.fixed(r)
    p0 = s.nbytes
    s.fixed([(258, 32768)] * 40 + [(3, 32768), (4, 1), (258, 32767)] * 10, final=True)
    return s.getvalue(), p0


def test_far_matches_across_cuts():
    """Distance-32768 matches read the oldest bytes of the history ring, the
    bytes a match copy overwrites: a token decoded from the zero bits past the
    end of a feed must not have written the ring.  One session per cut, all
    fed in one batch call."""
    import ztamd

    st, p0 = far_match_stream()
    data = zlib.decompress(st, -15)
    assert len(st) == 34766 and len(data) == 45738
    cuts = list(range(p0 - 2, len(st)))
    assert len(cuts) == 213
    sessions = [ztamd.InflateSession() for _ in cuts]
    try:
        first = ztamd.inflate_sessions_feed(sessions, [st[:c] for c in cuts])
        for (status, out), c in zip(first, cuts):
            assert status == 0
            check_bound(st, data, c, out)
        second = ztamd.inflate_sessions_feed(sessions, [st[c:] for c in cuts], last=True)
        for (s1, o1), (s2, o2), ses, c in zip(first, second, sessions, cuts):
            assert s2 == 0 and o1 + o2 == data, c
            assert ses.finished and ses.unused == 0 and ses.crc32 == zlib.crc32(data)
    finally:
        for ses in sessions:
            ses.close()


@pytest.mark.parametrize("feeds", [1, 3])
def test_output_full_stop(feeds):
    """A ratio above 1000:1: the output slot fills, the kernel stops at a
    token, and the host launches again on the input it has already uploaded --
    no size is guessed and nothing is decoded twice."""
    import ztamd

    data = bytes(4 << 20)
    s = raw(data, 9)
    assert len(s) < 4200
    step = (len(s) + feeds - 1) // feeds
    acc = b""
    with ztamd.InflateSession() as ses:
        for k in range(feeds):
            acc += ses.feed(s[k * step:(k + 1) * step], last=k == feeds - 1)
        info = ses.info()
        assert acc == data and ses.finished and ses.crc32 == zlib.crc32(data)
    assert info["launches"] > feeds
    work_is_linear(info)


def test_preset_window(oracle):
    import ztamd

    d = oracle.gen("wordsalad", 13, 40_000)
    s = raw(d[10_000:40_000], 6, zdict=d[:20_000])
    step = (len(s) + 4) // 5
    with ztamd.InflateSession(window=d[:20_000]) as ses:
        out = b"".join(ses.feed(s[k * step:(k + 1) * step], last=k == 4) for k in range(5))
        assert out == d[10_000:40_000]
        assert ses.info()["total_out"] == 30_000 and ses.finished
        assert ses.adler32 == zlib.adler32(out)


def one_shot_error(stream):
    import ztamd

    with pytest.raises(ztamd.ZtError) as e:
        ztamd.inflate_raw(stream)
    return e.value.code, e.value.msg


def test_errors(oracle):
    """Codes and texts are those of the one-shot decode of the whole bytes.
    (The truncated stream is cut inside a stored block, where the one-shot
    decoder reports the end of the input as the sessions do everywhere:
    'input buffer is broken'.)"""
    import ztamd

    # BTYPE 3 in the first header, far from the end of the feed: fails at once, and stays failed
    bad = b"\x07" + bytes(64)
    with ztamd.InflateSession() as ses:
        with pytest.raises(ztamd.ZtError) as e:
            ses.feed(bad)
        assert (e.value.code, e.value.msg) == (ZT_E_UNKNOWN_BTYPE, "unknown BTYPE: 3") == one_shot_error(bad)
        with pytest.raises(ztamd.ZtError) as e2:
            ses.feed(b"\x00" * 16)
        assert (e2.value.code, e2.value.msg) == (e.value.code, e.value.msg)
        info = ses.info()
        assert info["status"] == ZT_E_UNKNOWN_BTYPE and info["message"] == "unknown BTYPE: 3"
        assert info["total_out"] == 0
        res = ztamd.inflate_sessions_feed([ses], [b"\x00"])
        assert res[0][0] == ZT_E_UNKNOWN_BTYPE and res[0][0].message == "unknown BTYPE: 3" and res[0][1] == b""

    # the same two bytes as the last bytes of the input: they may still be running out of input
    data = oracle.gen("wordsalad", 21, 50_000)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    tail_bad = c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH) + b"\x07\x00"
    with ztamd.InflateSession() as ses:
        out = ses.feed(tail_bad)
        assert data.startswith(out) and not ses.finished and ses.info()["status"] == 0
        with pytest.raises(ztamd.ZtError) as e:
            ses.feed(b"", last=True)
        assert (e.value.code, e.value.msg) == (ZT_E_UNKNOWN_BTYPE, "unknown BTYPE: 3") == one_shot_error(tail_bad)

    # a valid stream truncated in the middle (inside a stored block)
    mixed = data + oracle.gen("xorshift32", 21, 60_000) + data
    s = raw(mixed, 6)
    cut = len(s) // 2
    assert len(zlib_prefix(s[:cut])) > len(data) + 1000 and len(zlib_prefix(s[:cut])) < len(data) + 59_000
    with ztamd.InflateSession() as ses:
        out = ses.feed(s[:cut // 2])
        out += ses.feed(s[cut // 2:cut])
        assert mixed.startswith(out) and len(out) >= len(zlib_prefix(s[:cut - 8]))
        with pytest.raises(ztamd.ZtError) as e:
            ses.feed(b"", last=True)
        assert (e.value.code, e.value.msg) == (ZT_E_INPUT_BROKEN, "input buffer is broken") == one_shot_error(s[:cut])

    # a fixed block whose first token is a match
    st = Stream()
    st.fixed([(3, 1)] + [65] * 40, final=True)
    far = st.getvalue()
    with ztamd.InflateSession() as ses:
        with pytest.raises(ztamd.ZtError) as e:
            ses.feed(far, last=True)
        assert e.value.code == ZT_E_INVALID_DISTANCE
        assert (e.value.code, e.value.msg) == one_shot_error(far)
    # with a preset window the same match is valid: the distance is judged against the window too
    with ztamd.InflateSession(window=b"xyz") as ses:
        assert ses.feed(far, last=True) == b"zzz" + b"A" * 40


def mixed_batch_plan(oracle):
    """64 small streams of every kind with their own cut schedules over 6 rounds."""
    rng = random.Random(64)
    plan = []
    for i in range(64):
        kind = KINDS[i % len(KINDS)]
        n = rng.randrange(2_000, 80_000)
        gen = ("wordsalad", "structured", "xorshift32")[i % 3]
        data = oracle.gen(gen, 100 + i, n)
        s = make_stream(oracle, kind, data)
        trailing = b""
        if i in (5, 40):
            trailing = bytes(rng.randrange(256) for _ in range(11 + i))
        if i == 17:  # corrupt: an unknown block type behind a sync flush, in the middle
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            s = c.compress(data[:n // 2]) + c.flush(zlib.Z_SYNC_FLUSH) + b"\x07" + bytes(200)
        if i % 8 == 3:  # finishes in round 2
            cuts = sorted([rng.randrange(1, len(s)), len(s)]) + [len(s)] * 4
        else:
            cuts = sorted(rng.randrange(0, len(s) + 1) for _ in range(5)) + [len(s)]
            if i % 5 == 0:
                cuts[2] = cuts[1]  # an empty feed
        full = s + trailing
        pieces, prev = [], 0
        for r, cut in enumerate(cuts):
            end = len(full) if (r == 5 and trailing) else cut
            pieces.append(full[prev:end])
            prev = end
        plan.append({"data": data, "stream": s, "trailing": trailing, "pieces": pieces, "corrupt": i == 17})
    return plan


def test_mixed_batch(oracle):
    import ztamd

    plan = mixed_batch_plan(oracle)
    assert any(not p for item in plan for p in item["pieces"][:5])
    batch = [ztamd.InflateSession() for _ in plan]
    single = [ztamd.InflateSession() for _ in plan]
    try:
        got = [[] for _ in plan]
        for r in range(6):
            rc, res = ztamd.inflate_sessions_feed(batch, [item["pieces"][r] for item in plan], last=r == 5,
                                                  return_code=True)
            for i, (status, out) in enumerate(res):
                got[i].append((int(status), status.message, out))
            if any(int(st) for st, _ in res):
                assert rc == next(int(st) for st, _ in res if int(st))
            else:
                assert rc == 0
        for i, item in enumerate(plan):
            want = []
            for r in range(6):
                try:
                    want.append((0, "", single[i].feed(item["pieces"][r], last=r == 5)))
                except ztamd.ZtError as e:
                    want.append((e.code, e.msg, b""))
            assert got[i] == want, i
            assert batch[i].info() == single[i].info(), i
            failed = [st for st, _, _ in got[i] if st]
            if item["corrupt"]:
                assert failed and set(failed) == {ZT_E_UNKNOWN_BTYPE}
                assert item["data"].startswith(b"".join(o for _, _, o in got[i]))
            else:
                assert not failed, i
                assert b"".join(o for _, _, o in got[i]) == item["data"], i
                assert batch[i].finished and batch[i].unused == len(item["trailing"])
                assert batch[i].crc32 == zlib.crc32(item["data"])
        with pytest.raises(ztamd.ZtError) as e:  # (no item carries a status: the call's code is raised)
            ztamd.inflate_sessions_feed([batch[0], batch[1], batch[0]], [b"", b"", b""])
        assert e.value.code == ZT_E_ARG
    finally:
        for ses in batch + single:
            ses.close()
