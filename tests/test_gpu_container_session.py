"""Container sessions (include/zt_stream_container.h; ztamd.GunzipSession,
ztamd.ZlibInflateSession, ztamd.container_sessions_feed): gzip files and zlib
streams fed piece by piece -- only the new bytes each time, many sessions per
call -- over the inflate sessions' kernel.

The yardstick for bytes is Python's gzip and zlib on the CPU; for error codes
and texts it is this library's own one-shot calls on the same bytes.  The
progress bound is test_gpu_stream_session.py's: after the feeds up to cut
``c`` the outputs so far hold at least what a CPU decode of ``file[:c - 8]``
yields, and are a prefix of the whole decode.

The files are small on purpose: the slots of a launch hold eight times their
input, and no body here expands more than that, so no launch stops on a full
slot and a session takes part in at most one launch per member it starts plus
one per feed."""
import gzip
import struct
import zlib

import pytest

from deflate_builder import Stream

pytestmark = pytest.mark.gpu

ZT_E_INPUT_BROKEN, ZT_E_INVALID_DISTANCE, ZT_E_ARG = -10, -15, -103
ZT_E_GZIP_SIGNATURE, ZT_E_GZIP_METHOD, ZT_E_GZIP_HCRC, ZT_E_GZIP_CRC32, ZT_E_GZIP_ISIZE = -30, -31, -32, -33, -34
ZT_E_ZLIB_FDICT, ZT_E_ZLIB_ADLER, ZT_E_ZLIB_DICTID = -42, -43, -44


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def gz_member(body, data, extra=None, name=None, comment=None, hcrc=False, mtime=0):
    """(header, member) of one RFC 1952 member built by hand; FHCRC over this member's own header."""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (
        2 if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + struct.pack("<I", mtime) + b"\x02\x03"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\x00"
    if comment is not None:
        h += comment + b"\x00"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h, h + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def cpu_prefix(prefix):
    """Every byte a CPU gzip decoder yields from a prefix of a multi-member file."""
    out = b""
    while prefix:
        d = zlib.decompressobj(31)
        out += d.decompress(prefix)
        if not d.eof:
            break
        prefix = d.unused_data
    return out


def work_is_linear(info):
    assert info["decoded_bits"] <= info["end_bits"] + info["launches"] * 8 * 1024, info


def open_sessions(make, count):
    return [make() for _ in range(count)]


def close_all(sessions):
    for s in sessions:
        s.close()


@pytest.fixture(scope="module")
def four_members(oracle):
    """(file, whole decode, expected member records)"""
    text = oracle.gen("wordsalad", 3, 2048)
    stored = oracle.gen("xorshift32", 3, 300)
    tail = b"the last member, the last member, the last member."
    parts = [
        (raw(text, 9), text, dict(extra=b"EX\x04\x00abcd", name=b"a.txt", comment=b"first", hcrc=True, mtime=77)),
        (raw(b""), b"", dict()),
        (raw(stored, 0), stored, dict(name=b"")),
        (raw(tail, 6, zlib.Z_FIXED), tail, dict(hcrc=True, comment=b"d")),
    ]
    assert parts[0][0][0] & 6 == 4 and parts[2][0][0] & 6 == 0  # a dynamic and a stored first block
    file, want, off = b"", [], 0
    for body, data, kw in parts:
        h, m = gz_member(body, data, **kw)
        want.append({"flg": h[3], "mtime": kw.get("mtime", 0), "xfl": 2, "os": 3, "xlen": len(kw.get("extra", b"")),
                     "has_crc16": int(kw.get("hcrc", False)), "crc32": zlib.crc32(data), "isize": len(data),
                     "name": kw.get("name"), "comment": kw.get("comment"), "data_off": off, "data_len": len(data),
                     "in_off": len(file)})
        if kw.get("hcrc"):
            want[-1]["crc16"] = zlib.crc32(h[:-2]) & 0xFFFF
        file += m
        off += len(data)
    data = b"".join(d for _, d, _ in parts)
    assert gzip.decompress(file) == data
    return file, data, want


def check_members(ses, want):
    got = ses.members()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k, v in w.items():
            assert g[k] == v, (k, g[k], v)


def test_every_cut(four_members):
    """One session per cut position of a four-member file, two batch calls."""
    import ztamd

    file, data, want = four_members
    cuts = list(range(len(file) + 1))
    sessions = open_sessions(ztamd.GunzipSession, len(cuts))
    try:
        first = ztamd.container_sessions_feed(sessions, [file[:c] for c in cuts])
        for (st, out), c in zip(first, cuts):
            assert st == 0, (c, st.message)
            assert data.startswith(out) and len(cpu_prefix(file[:max(0, c - 8)])) <= len(out), c
        second = ztamd.container_sessions_feed(sessions, [file[c:] for c in cuts], last=True)
        for (s1, o1), (s2, o2), ses, c in zip(first, second, sessions, cuts):
            assert s2 == 0 and o1 + o2 == data, c
            info = ses.info()
            assert info["finished"] and info["at_member_end"] and info["members_done"] == 4 and info["unused"] == 0
            assert info["total_in"] == len(file) and info["total_out"] == len(data)
            assert info["end_bits"] == 8 * len(file) and info["pending"] == 0
            assert info["crc32"] == want[3]["crc32"]
            assert info["launches"] <= 4 + 2, (c, info)
            work_is_linear(info)
        for ses in sessions:  # (a header cut by the feeds is read from the bytes held back and the new ones)
            check_members(ses, want)
    finally:
        close_all(sessions)


def test_all_pairs_of_cuts():
    """Every pair of cuts of a short two-member file, three batch calls."""
    import ztamd

    a, b = b"pairs of cuts, pairs of cuts", b"0123456789"
    file = gz_member(raw(a, 6, zlib.Z_FIXED), a)[1] + gz_member(raw(b, 0), b, name=b"n")[1]
    data = a + b
    assert gzip.decompress(file) == data
    pairs = [(i, j) for i in range(len(file) + 1) for j in range(i, len(file) + 1)]
    assert 2000 < len(pairs) < 4096
    sessions = open_sessions(ztamd.GunzipSession, len(pairs))
    try:
        r1 = ztamd.container_sessions_feed(sessions, [file[:i] for i, _ in pairs])
        r2 = ztamd.container_sessions_feed(sessions, [file[i:j] for i, j in pairs])
        for (s1, o1), (s2, o2), (i, j) in zip(r1, r2, pairs):
            assert s1 == 0 and s2 == 0
            acc = o1 + o2
            assert data.startswith(acc) and len(cpu_prefix(file[:max(0, j - 8)])) <= len(acc), (i, j)
        r3 = ztamd.container_sessions_feed(sessions, [file[j:] for _, j in pairs], last=True)
        for (s1, o1), (s2, o2), (s3, o3), ses, p in zip(r1, r2, r3, sessions, pairs):
            assert s3 == 0 and o1 + o2 + o3 == data, p
        for ses in sessions[::211]:
            info = ses.info()
            assert info["finished"] and info["members_done"] == 2 and info["launches"] <= 2 + 3
            assert [m["name"] for m in ses.members()] == [None, b"n"]
    finally:
        close_all(sessions)


def test_one_byte_per_feed(oracle):
    import ztamd

    a = oracle.gen("wordsalad", 9, 150)
    b = b"stored bytes"
    file = (gz_member(raw(a, 9), a, name=b"one", hcrc=True)[1] + gz_member(raw(b""), b"")[1]
            + gz_member(raw(b, 0), b, comment=b"c")[1])
    data = a + b
    assert gzip.decompress(file) == data and 150 < len(file) < 260
    acc = b""
    with ztamd.GunzipSession() as ses:
        for i in range(len(file)):
            acc += ses.feed(file[i:i + 1], last=i == len(file) - 1)
            assert data.startswith(acc)
            assert len(cpu_prefix(file[:max(0, i + 1 - 8)])) <= len(acc), i
            assert ses.info()["pending"] <= 1024
        info = ses.info()
        assert acc == data and info["finished"] and info["members_done"] == 3 and info["at_member_end"]
        work_is_linear(info)


def one_shot_zlib(stream, verify, dictionary):
    import ztamd

    try:
        return 0, "", ztamd.zlib_decompress(stream, verify=verify, dictionary=dictionary)[0]
    except ztamd.ZtError as e:
        return e.code, e.msg, b""


def run_session(ses, pieces):
    """(status, message, output) of the pieces fed in turn, last on the final one."""
    import ztamd

    out = b""
    for k, p in enumerate(pieces):
        try:
            out += ses.feed(p, last=k == len(pieces) - 1)
        except ztamd.ZtError as e:
            return e.code, e.msg, out + e.output
    return 0, "", out


def test_zlib_every_cut(oracle):
    import ztamd

    dic = oracle.gen("wordsalad", 5, 3000)
    data = oracle.gen("wordsalad", 5, 5000)[2000:]
    plain = zlib.compress(data, 6)
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, dic)
    fdict = c.compress(data) + c.flush()
    assert fdict[1] & 0x20 and not plain[1] & 0x20 and len(fdict) < len(plain)
    for stream, d in ((plain, None), (fdict, dic), (plain, dic)):
        stream += b"TRAIL"
        zd = [d] if d and stream[1] & 0x20 else []
        cuts = list(range(len(stream) + 1))
        sessions = open_sessions(lambda: ztamd.ZlibInflateSession(dictionary=d, auto=d is None), len(cuts))
        try:
            r1 = ztamd.container_sessions_feed(sessions, [stream[:k] for k in cuts])
            r2 = ztamd.container_sessions_feed(sessions, [stream[k:] for k in cuts], last=True)
            for (s1, o1), (s2, o2), ses, k in zip(r1, r2, sessions, cuts):
                assert s1 == 0 and s2 == 0 and o1 + o2 == data, k
                assert len(zlib.decompressobj(15, *zd).decompress(stream[:max(0, k - 8)])) <= len(o1), k
            for ses in sessions[::53] + sessions[-1:]:
                info = ses.info()
                assert info["finished"] and info["unused"] == 5 and info["members_done"] == 1
                assert info["adler32"] == zlib.adler32(data) and info["format"] == ztamd.SESSION_ZLIB
                assert info["launches"] <= 1 + 2
                work_is_linear(info)
        finally:
            close_all(sessions)
    # AUTO picks gzip too
    g = gzip.compress(data, 6)
    with ztamd.GunzipSession(auto=True) as ses:
        assert ses.feed(g[:1]) + ses.feed(g[1:], last=True) == data and ses.info()["format"] == ztamd.SESSION_GZIP
    # the dictionary cases are the one-shot call's
    for d, code in ((dic[:-1], ZT_E_ZLIB_DICTID), (None, ZT_E_ZLIB_FDICT)):
        want = one_shot_zlib(fdict, True, d if d is not None else b"")
        assert want[0] == code
        with ztamd.ZlibInflateSession(dictionary=d) as ses:
            with pytest.raises(ztamd.ZtError) as e:  # decided by the header alone, before `last`
                ses.feed(fdict[:6])
            assert (e.value.code, e.value.msg, e.value.output) == want
        with ztamd.ZlibInflateSession(dictionary=d) as ses:
            assert run_session(ses, [fdict[:3], fdict[3:]]) == want
    # a flipped Adler-32
    for stream, d in ((plain, None), (fdict, dic)):
        bad = stream[:-2] + bytes([stream[-2] ^ 4]) + stream[-1:]
        want = one_shot_zlib(bad, True, d)
        assert want[0] == ZT_E_ZLIB_ADLER
        with ztamd.ZlibInflateSession(dictionary=d) as ses:
            st, msg, out = run_session(ses, [bad[:100], bad[100:]])
            assert (st, msg) == want[:2] and out == data
            with pytest.raises(ztamd.ZtError) as e:  # sticky
                ses.feed(b"more")
            assert (e.value.code, e.value.msg) == want[:2]
        with ztamd.ZlibInflateSession(dictionary=d, verify=False) as ses:
            assert run_session(ses, [bad[:100], bad[100:]]) == (0, "", data)
            assert one_shot_zlib(bad, False, d) == (0, "", data)


def test_fdict_distance_bound():
    """With FDICT the history is the dictionary: distance dict_len is its first byte, dict_len + 1 is invalid."""
    import ztamd

    dic = b"abcdef" * 5
    head = b"\x78\xbb" + struct.pack(">I", zlib.adler32(dic))
    assert (head[0] * 256 + head[1]) % 31 == 0 and head[1] & 0x20
    for dist, ok in ((len(dic), True), (len(dic) + 1, False)):
        s = Stream()
        s.fixed([(3, dist), 65, 66], final=True)
        out = dic[:3] + b"AB"
        stream = head + s.getvalue() + struct.pack(">I", zlib.adler32(out))
        want = one_shot_zlib(stream, True, dic)
        assert want == ((0, "", out) if ok else (ZT_E_INVALID_DISTANCE, want[1], b""))
        for pieces in ([stream], [stream[:4], stream[4:7], stream[7:]]):
            with ztamd.ZlibInflateSession(dictionary=dic) as ses:
                assert run_session(ses, pieces) == want


def test_history_is_per_member():
    """The ring is not cleared at a member's end: the kernel's distance test
    alone keeps the second member from reading the first one's bytes."""
    import ztamd

    first = b"member one's bytes " * 8
    s = Stream()
    s.fixed([(3, 1)] + [65] * 40, final=True)
    file = gz_member(raw(first, 6), first)[1]
    n1 = len(file)
    file += gz_member(s.getvalue(), b"???" + b"A" * 40)[1]
    with pytest.raises(ztamd.ZtError) as ref:
        ztamd.inflate_raw(s.getvalue())
    assert ref.value.code == ZT_E_INVALID_DISTANCE
    for pieces in ([file], [file[:n1], file[n1:]], [file[:n1 + 12], file[n1 + 12:]]):
        with ztamd.GunzipSession() as ses:
            st, msg, out = run_session(ses, pieces)
            assert (st, msg) == (ZT_E_INVALID_DISTANCE, ref.value.msg)
            assert out == first  # no byte of member one is copied
            info = ses.info()
            assert info["members_done"] == 1 and not info["at_member_end"] and info["status"] == st
            assert info["total_out"] == len(first)


def one_shot_gunzip(data):
    import ztamd

    try:
        return 0, "", ztamd.gunzip(data)[0]
    except ztamd.ZtError as e:
        return e.code, e.msg, b""


@pytest.fixture(scope="module")
def stored_member(oracle):
    data = oracle.gen("xorshift32", 8, 40)
    head, file = gz_member(raw(data, 0), data, name=b"f", hcrc=True)
    assert one_shot_gunzip(file) == (0, "", data)
    return data, head, file


def test_errors_equal_the_one_shot_call(stored_member):
    import ztamd

    data, head, file = stored_member
    t = len(file) - 8
    cases = {
        "magic": (bytes([file[0] ^ 1]) + file[1:], ZT_E_GZIP_SIGNATURE, 2),
        "method": (file[:2] + b"\x07" + file[3:], ZT_E_GZIP_METHOD, 3),
        "fhcrc": (file[:len(head) - 1] + bytes([file[len(head) - 1] ^ 1]) + file[len(head):], ZT_E_GZIP_HCRC, len(head)),
        "crc": (file[:t] + bytes([file[t] ^ 1]) + file[t + 1:], ZT_E_GZIP_CRC32, len(file)),
        "isize": (file[:t + 4] + bytes([file[t + 4] ^ 1]) + file[t + 5:], ZT_E_GZIP_ISIZE, len(file)),
        "garbage": (file + b"\x00\x01\x02", ZT_E_GZIP_SIGNATURE, len(file) + 2),
    }
    for name, (bad, code, decided) in cases.items():
        want = one_shot_gunzip(bad)
        assert want[0] == code, name
        # in one feed without `last`: the first feed that can decide reports it
        with ztamd.GunzipSession() as ses:
            with pytest.raises(ztamd.ZtError) as e:
                ses.feed(bad)
            assert (e.value.code, e.value.msg) == want[:2], name
            assert data.startswith(e.value.output)
            with pytest.raises(ztamd.ZtError) as e2:  # sticky
                ses.feed(b"", last=True)
            assert (e2.value.code, e2.value.msg) == want[:2] and e2.value.output == b""
        # cut one byte before the deciding byte: the first feed passes, the second reports
        with ztamd.GunzipSession() as ses:
            out = ses.feed(bad[:decided - 1])
            assert data.startswith(out) and ses.info()["status"] == 0, name
            with pytest.raises(ztamd.ZtError) as e:
                ses.feed(bad[decided - 1:decided])
            assert (e.value.code, e.value.msg) == want[:2], name


def test_truncation_at_every_length(stored_member):
    """`last` on a file cut at every length: the status and text of gunzip on the same bytes."""
    import ztamd

    data, head, file = stored_member
    lens = list(range(len(file)))
    sessions = open_sessions(ztamd.GunzipSession, len(lens))
    try:
        res = ztamd.container_sessions_feed(sessions, [file[:n] for n in lens], last=True)
        got = [(int(st), st.message) for st, _ in res]
        want = [one_shot_gunzip(file[:n])[:2] for n in lens]
        differ = [(n, g, w) for n, g, w in zip(lens, got, want) if g != w]
        print("truncation: session / one-shot differ at", differ)
        assert not differ
        assert all(data.startswith(out) for _, out in res)
    finally:
        close_all(sessions)


def test_truncated_stored_header_behind_other_blocks(oracle):
    """The end of the input inside a stored block's LEN / NLEN is reported as the
    one-shot call reports it also when Huffman blocks precede the stored block
    in the same feed or in an earlier one (the host walks the final feed's
    tokens from the session's state).  Elsewhere a cut body reports the
    one-shot status, or 'input buffer is broken' inside a Huffman code."""
    import ztamd

    text = oracle.gen("wordsalad", 14, 600)
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    body = c.compress(text) + c.flush(zlib.Z_SYNC_FLUSH)  # a dynamic block, an empty stored block
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    body += c.compress(b"fixed fixed fixed") + c.flush(zlib.Z_SYNC_FLUSH) + raw(b"tail bytes", 0)
    data = text + b"fixed fixed fixed" + b"tail bytes"
    head, file = gz_member(body, data)
    assert one_shot_gunzip(file) == (0, "", data)
    lens = list(range(48, len(file) - 8))
    want = [one_shot_gunzip(file[:n])[:2] for n in lens]
    stored = [n for n, w in zip(lens, want) if w[0] in (-13, -14)]
    assert len(stored) == 12 and {w[0] for w in want} >= {-13, -14, ZT_E_INPUT_BROKEN}
    for first in (0, 40):  # the whole cut file in the final feed, and after an earlier feed
        sessions = open_sessions(ztamd.GunzipSession, len(lens))
        try:
            if first:
                ztamd.container_sessions_feed(sessions, [file[:first]] * len(lens))
            res = ztamd.container_sessions_feed(sessions, [file[first:n] for n in lens], last=True)
            for (st, out), n, w in zip(res, lens, want):
                got = (int(st), st.message)
                if n in stored:
                    assert got == w, (n, got, w)
                else:
                    assert got in (w, (ZT_E_INPUT_BROKEN, "input buffer is broken")), (n, got, w)
        finally:
            close_all(sessions)


def test_mixed_batch(oracle, four_members):
    """gzip and zlib sessions, finished and failing ones in one call: a failed item leaves the others untouched."""
    import ztamd

    file, data, _ = four_members
    z = oracle.gen("wordsalad", 12, 3000)
    zs = zlib.compress(z, 9)
    bad = file[:700] + bytes([file[700] ^ 0x55]) + file[701:]  # inside the first body
    ses = [ztamd.GunzipSession(), ztamd.ZlibInflateSession(), ztamd.GunzipSession(), ztamd.GunzipSession(),
           ztamd.ZlibInflateSession(auto=True), ztamd.GunzipSession()]
    inputs = [file, zs, bad, file, zs + b"xx", b""]
    try:
        third = len(file) // 3
        assert data.startswith(ses[3].feed(file[:third]))  # (already under way)
        assert ses[5].feed(file, last=True) == data and ses[5].finished
        halves = [(x[:len(x) // 2], x[len(x) // 2:]) for x in inputs]
        halves[3] = (file[third:len(file) // 2], file[len(file) // 2:])
        rc1, r1 = ztamd.container_sessions_feed(ses, [h[0] for h in halves], return_code=True)
        rc2, r2 = ztamd.container_sessions_feed(ses, [h[1] for h in halves], last=True, return_code=True)
        got = [(int(s2), o1 + o2) for (s1, o1), (s2, o2) in zip(r1, r2)]
        assert got[0] == (0, data) and got[1] == (0, z) and got[4] == (0, z) and got[5] == (0, b"")
        assert got[3][0] == 0 and ses[3].info()["total_out"] == len(data)
        assert got[2][0] != 0 and got[2][1] != data
        failing = [int(s) for s, _ in r1 + r2 if int(s)]
        assert failing and set(failing) == {got[2][0]}
        assert rc2 == got[2][0] and rc1 in (0, got[2][0])
        assert ses[4].unused == 2 and ses[4].info()["format"] == ztamd.SESSION_ZLIB
        assert all(s.finished for k, s in enumerate(ses) if k != 2)
        # a finished session counts what follows, a failed one repeats its error
        again = ztamd.container_sessions_feed([ses[0], ses[2]], [b"zz", b"zz"])
        assert int(again[0][0]) == 0 and again[0][1] == b"" and int(again[1][0]) == got[2][0]
        assert again[1][0].message == r2[2][0].message != ""
        with pytest.raises(ztamd.ZtError) as e:  # (no item carries a status: the call's code is raised)
            ztamd.container_sessions_feed([ses[0], ses[1], ses[0]], [b"", b"", b""])
        assert e.value.code == ZT_E_ARG
    finally:
        close_all(ses)
