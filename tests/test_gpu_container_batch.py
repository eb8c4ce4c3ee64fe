"""Batch GUnzip and zlib Inflate (include/zt_container_batch.h) on the GPU:
many gzip files / zlib streams decoded and verified per call.  Per item the
output, the members, the status and the message are what the single call on
that item alone gives (zt_gunzip, zt_zlib_decompress, zt_zlib_decompress_dict),
and what the reference recorded (tests/golden/containers.json)."""
import gzip
import json
import os
import subprocess
import sys
import zlib

import pytest

import dict_corpus
from container_batch_corpus import alias_items, data_of, frame, gzip_member, results_digest
from golden_util import blob_bytes, blob_matches, load

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = load("containers.json")["records"]
SIZES = [0, 1, 100, 4 << 10, 64 << 10, 300 << 10]


@pytest.fixture(scope="module")
def zt():
    import ztamd

    assert ztamd.device_count() > 0, "no GPU visible"
    return ztamd


def single_gunzip(zt, item):
    """(status, message, output, members) of zt.gunzip(item) alone."""
    try:
        out, members = zt.gunzip(item)
    except zt.ZtError as e:
        return e.code, e.msg, None, []
    return 0, "", out, members


def same_as_single(zt, items, results):
    for item, (st, out, members) in zip(items, results):
        code, msg, sout, smembers = single_gunzip(zt, item)
        assert (int(st), st.message) == (code, msg)
        assert out == sout
        assert members == smembers


def test_golden_gunzip_one_batch(zt):
    recs = [r for r in REC if r["kind"] in ("gzip", "gunzip")]
    items = [blob_bytes(r.get("stream") or r["output"]) for r in recs]
    rc, res = zt.gunzip_batch(items, return_code=True)
    assert len(res) == len(recs)
    first = 0
    for r, (st, out, members) in zip(recs, res):
        want = r["gunzip"]
        if not want["ok"]:
            assert st != 0 and out is None and members == []
            assert st.message == want["error"]["message"]
            first = first or int(st)
            continue
        # (as check_gunzip of tests/test_gpu_containers.py compares them)
        assert st == 0 and st.message == ""
        assert blob_matches(want["out"], out)
        assert len(members) == len(want["members"])
        for m, w in zip(members, want["members"]):
            assert (m["flg"], m["xfl"], m["os"], m["mtime"]) == (w["flg"], w["xfl"], w["os"], w["mtime"])
            for k in ("name", "comment"):
                assert (None if m[k] is None else m[k].decode("latin1")) == w[k]
            assert blob_matches(w["data"], m["data"])
        assert members[-1]["crc32"] == want["crc32"]
    assert first != 0 and rc == first  # the batch holds failing records; the call returns the first one's code


@pytest.mark.parametrize("verify", [False, True])
def test_golden_zlib_one_batch(zt, verify):
    recs, items, index = [], [], []
    for r in REC:
        if r["kind"] == "zlib" and "output" in r:
            recs.append((r, r[f"inflate_{str(verify).lower()}"], r["compressionType"] != 0))
            items.append(blob_bytes(r["output"]))
            index.append(0)
        elif r["kind"] == "inflate" and bool(r["opts"].get("verify", False)) == verify:
            recs.append((r, r["inflate"], True))
            items.append(blob_bytes(r["stream"]))
            index.append(r["opts"].get("index", 0))
    rc, res = zt.zlib_decompress_batch(items, verify=verify, index=index, return_code=True)
    first = 0
    for (r, want, exact_msg), (st, out, ip, adler) in zip(recs, res):
        if not want["ok"]:
            assert st != 0 and out is None
            # (compressionType 0: the reference's 32 KiB NONE buffer; its decoder ignores NLEN
            # and the engine reports it -- tests/test_gpu_containers.py)
            if exact_msg:
                assert st.message == want["error"]["message"]
            first = first or int(st)
            continue
        assert st == 0 and blob_matches(want["out"], out) and ip == want["ip"]
        assert adler == (zlib.adler32(out) if verify else 1)
    assert rc == first


def test_python_writers(zt, oracle):
    datas, items = [], []
    for k in range(64):
        d = data_of(oracle, k, SIZES[k % len(SIZES)])
        datas.append(d)
        how = (k // len(SIZES)) % 4
        if how < 3:
            items.append(gzip.compress(d, (1, 6, 9)[how], mtime=k))
        else:
            items.append(frame(d, extra=bytes(range(k % 40)), name=b"n%d" % k))
    own = zt.gzip_compress_batch(datas[:12], name=b"file.bin", comment=b"a comment", hcrc=True, mtime=77)
    items += own
    datas += datas[:12]
    res = zt.gunzip_batch(items)
    for d, (st, out, members) in zip(datas, res):
        assert st == 0 and out == d
    same_as_single(zt, items, res)
    st = zt.gunzip_batch_stats()
    assert st["items"] == len(items) and st["members"] == len(items)


def test_multi_member(zt, oracle):
    passes = {}
    for M in (1, 2, 4, 64):
        items, datas = [], []
        for i in range(8):
            parts = [data_of(oracle, 100 * i + j, 1024 + (977 * (i + 3 * j)) % (7 << 10)) for j in range(M)]
            ms = [gzip_member(p, 1 + j % 9) if j % 3 else frame(p, name=b"m%d" % j, comment=b"c") for j, p in
                  enumerate(parts)]
            items.append(b"".join(ms))
            datas.append(b"".join(parts))
        res = zt.gunzip_batch(items)
        st = zt.gunzip_batch_stats()
        for d, (s, out, members) in zip(datas, res):
            assert s == 0 and out == d and len(members) == M
        same_as_single(zt, items, res)
        assert st["members"] == 8 * M and st["items"] == 8
        passes[M] = st["decode_passes"]
    assert passes[4] == passes[64] <= 2, passes


def test_dense_members_truncated_list(zt):
    """Members of about 21 bytes: 12 per 256 bytes of input, more than the
    candidate list holds (one per item and per 256 packed bytes), so the list
    is truncated and the chain asks for the starts it misses; the host scan
    behind each adds 32, 64, 128 ... candidates to the next pass, so the 3000
    members take at most 1 + 7 passes (32 * (2^7 - 1) >= 3000)."""
    parts = [bytes([65 + k % 26]) * (k % 4) for k in range(3000)]
    item = b"".join(gzip_member(p, 6) for p in parts)
    good = gzip_member(b"beside it " * 100)
    res = zt.gunzip_batch([good, item])
    st = zt.gunzip_batch_stats()
    assert res[0][0] == 0 and res[0][1] == b"beside it " * 100
    s, out, members = res[1]
    assert s == 0 and out == b"".join(parts) and len(members) == 3000
    assert [m["data"] for m in members] == parts
    assert st["members"] == 3001 and st["candidates"] >= 3001
    assert 2 <= st["decode_passes"] <= 8 and st["redecoded"] >= 1, st
    same_as_single(zt, [item], res[1:])


def test_false_candidates(zt, oracle):
    inner = gzip_member(b"an inner member " * 40)
    c = zlib.compressobj(0, zlib.DEFLATED, 31)
    payload = inner + oracle.gen("xorshift32", 5, 200 << 10)
    outer = c.compress(payload) + c.flush()
    assert outer[15:15 + len(inner)] == inner  # the inner header survives intact in the stored block
    text = oracle.gen("wordsalad", 6, 5000)
    in_comment = frame(text, comment=b"abc\x1f\x8b\x08\x01xyz")
    in_extra = frame(text, extra=gzip_member(b"hidden in FEXTRA"))
    items = [outer, in_comment, in_extra]
    for it in items:
        assert gzip.decompress(it) in (payload, text)
    res = zt.gunzip_batch([outer])
    st = zt.gunzip_batch_stats()
    assert res[0][0] == 0 and res[0][1] == payload
    assert st["candidates"] > st["members"] == 1 and st["redecoded"] >= 1, st
    res = zt.gunzip_batch(items)
    st = zt.gunzip_batch_stats()
    for it, (s, out, members) in zip(items, res):
        assert s == 0 and out == gzip.decompress(it) and len(members) == 1
    same_as_single(zt, items, res)
    assert st["candidates"] > st["members"] == 3 and st["redecoded"] >= 1, st


def test_per_item_errors(zt, oracle):
    good = [gzip_member(data_of(oracle, k, 3000 + 500 * k)) for k in range(9)]
    base = gzip_member(oracle.gen("wordsalad", 9, 20000))

    def flip(b, at):
        return b[:at] + bytes([b[at] ^ 0x55]) + b[at + 1:]

    bad = {
        "signature": b"\x1f\x8c" + base[2:],
        "garbage after a member": base + b"garbage!",
        "crc32": flip(base, len(base) - 8),
        "isize": flip(base, len(base) - 1),
        "truncated body": base[:len(base) // 2],
        "trailer cut off": base[:-6],
        "corrupt body": flip(base, len(base) // 2),
        "method": base[:2] + b"\x07" + base[3:],
    }
    reference_defines = ("signature", "garbage after a member", "crc32", "isize", "trailer cut off", "method")
    items, names = [], []
    for g, (name, b) in zip(good, bad.items()):
        items += [g, b]
        names += [None, name]
    items.append(good[8])
    names.append(None)
    rc, res = zt.gunzip_batch(items, return_code=True)
    same_as_single(zt, items, res)
    for name, item, (st, out, members) in zip(names, items, res):
        if name is None:
            assert st == 0 and out == gzip.decompress(item)
            continue
        assert st != 0 and out is None and members == [], name
        if name in reference_defines:
            import zt_oracle

            with pytest.raises(zt_oracle.OracleError) as ei:
                oracle.gunzip(item)
            assert (int(st), st.message) == (ei.value.code, ei.value.msg), name
    assert rc == int(res[1][0])


def test_signature_flood(zt, oracle):
    flood = b"\x1f\x8b\x08" * 131072
    good = [gzip_member(data_of(oracle, k, 10000 + k)) for k in range(8)]
    items = good[:4] + [flood] + good[4:]
    zt.release_scratch()
    res = zt.gunzip_batch(items)
    dev_bytes, _ = zt.scratch_bytes()
    st = zt.gunzip_batch_stats()
    code, msg, _, _ = single_gunzip(zt, flood)
    assert code != 0 and (int(res[4][0]), res[4][0].message) == (code, msg)
    for k in (0, 1, 2, 3, 5, 6, 7, 8):
        assert res[k][0] == 0 and res[k][1] == gzip.decompress(items[k])
    assert st["candidates"] >= 131072
    # unbounded, 131 072 candidates x 256 KiB of token slots ask for ~32 GiB;
    # with the candidate list's capacity the call asks for tens of MiB
    assert dev_bytes < 1 << 30, dev_bytes


def test_zlib_batch(zt, oracle):
    datas, items, index = [], [], []
    for k in range(24):
        d = data_of(oracle, 50 + k, SIZES[k % len(SIZES)])
        pre = b"\xAA" * (k % 5)
        datas.append(d)
        items.append(pre + zlib.compress(d, (0, 1, 6, 9)[(k // len(SIZES)) % 4]))
        index.append(len(pre))
    ok = zlib.compress(b"hello hello hello hello")
    bad_adler = ok[:-1] + bytes([ok[-1] ^ 1])
    bad_fcheck = bytes([ok[0], ok[1] ^ 1]) + ok[2:]
    bad_method = bytes([0x77]) + ok[1:]
    d0 = dict_corpus.dictionary()
    c = zlib.compressobj(zdict=d0)
    with_fdict = c.compress(b"needs a dictionary") + c.flush()
    extra = [bad_adler, bad_fcheck, bad_method, with_fdict, b""]
    allitems = items + extra
    allindex = index + [0] * len(extra)
    for verify in (False, True):
        rc, res = zt.zlib_decompress_batch(allitems, verify=verify, index=allindex, return_code=True)
        first = 0
        for k, (item, idx, (st, out, ip, adler)) in enumerate(zip(allitems, allindex, res)):
            try:
                sout, sip = zt.zlib_decompress(item, index=idx, verify=verify)
                assert st == 0 and out == sout and ip == sip
                assert adler == (zlib.adler32(out) if verify else 1)
            except zt.ZtError as e:
                assert (int(st), st.message) == (e.code, e.msg) and out is None
                first = first or e.code
        assert rc == first
        for d, (st, out, ip, adler) in zip(datas, res):
            assert st == 0 and out == d
        n = len(items)
        assert (res[n][0] == -43) == verify and (verify or res[n][1] == b"hello hello hello hello")  # ZT_E_ZLIB_ADLER
        assert res[n + 1][0] == -41 and res[n + 2][0] == -40  # ZT_E_ZLIB_FCHECK, ZT_E_ZLIB_METHOD
        assert res[n + 3][0] == -42 and res[n + 3][0].message == "fdict flag is not supported"
        assert res[n + 4][0] == -40


def test_dictionary_batch(zt):
    D = dict_corpus.dictionary()
    recs = dict_corpus.messages(256)
    msgs = recs[:24] + [b"".join(recs[24 + 16 * k:24 + 16 * (k + 1)])[:4096] for k in range(12)]
    assert min(map(len, msgs)) < 600 and max(map(len, msgs)) == 4096
    own = zt.zlib_compress_batch(msgs[0::3], dictionary=D)
    py = []
    for m in msgs[1::3]:
        c = zlib.compressobj(zdict=D)
        py.append(c.compress(m) + c.flush())
    plain = [zlib.compress(m) for m in msgs[2::3]]
    items = own + py + plain
    want = msgs[0::3] + msgs[1::3] + msgs[2::3]
    nfd = len(own) + len(py)
    assert all(it[1] & 0x20 for it in items[:nfd]) and not any(it[1] & 0x20 for it in plain)
    for verify in (False, True):
        res = zt.zlib_decompress_batch(items, verify=verify, dictionary=D)
        for item, w, (st, out, ip, adler) in zip(items, want, res):
            assert st == 0 and out == w and ip == len(item) - 4
            assert adler == (zlib.adler32(w) if verify else 1)
            assert (out, ip) == zt.zlib_decompress(item, verify=verify, dictionary=D)
    other = D[:-1] + b"!"
    rc, res = zt.zlib_decompress_batch(items, verify=True, dictionary=other, return_code=True)
    assert rc == -44
    for k, (item, w, (st, out, ip, adler)) in enumerate(zip(items, want, res)):
        if k < nfd:
            assert st == -44 and out is None  # ZT_E_ZLIB_DICTID
            with pytest.raises(zt.ZtError) as ei:
                zt.zlib_decompress(item, verify=True, dictionary=other)
            assert st.message == ei.value.msg
        else:
            assert st == 0 and out == w


def test_alias_devices(zt, oracle):
    """The same batches over 8 logical devices (LPT split, one host thread per
    device): the digests of outputs and members are those of one device."""
    gz, zl, datas = alias_items(oracle)
    g = zt.gunzip_batch(gz)
    st = zt.gunzip_batch_stats()
    z = zt.zlib_decompress_batch(zl, verify=True)
    assert [r[1] for r in g] == datas and [r[1] for r in z] == datas
    env = dict(os.environ, ZT_ALIAS_DEVICES="8")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "container_batch_alias_child.py")], env=env,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res == {"logical_devices": 8, "gzip": results_digest(g), "zlib": results_digest(z), "items": 256,
                   "members": st["members"]}, res
