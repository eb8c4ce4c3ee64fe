"""ZipCrypto on the GPU (csrc/zipcrypto.hip, include/zt_zipcrypto.h): the raw
cipher batches against the pure-Python cipher of tests/zipcrypto_py.py (pinned
to the reference by tests/test_zipcrypto_ref.py), password archives against
the fixtures the reference's own Zip / Unzip wrote
(tests/golden/zipcrypto.json) and against Python's zipfile."""
import ctypes
import io
import zipfile
import zlib

import numpy as np
import pytest

import zipcrypto_py as zc
from golden_util import blob_bytes, load
from test_zip_fixtures import DATE, gen_spec, parse_zip

pytestmark = pytest.mark.gpu

FIX = load("zipcrypto.json")
RECORDS = FIX["records"]
PASSWORDS = [b"", b"k", b"password", bytes([0x80, 0xFF, 0x41, 0xC3, 0xA9, 0x00, 0x7F])]


@pytest.fixture(scope="module")
def zt():
    import ztamd

    assert ztamd.device_count() > 0, "no GPU visible"
    return ztamd


def rnd(seed, n):
    return np.random.RandomState(seed).bytes(n)


@pytest.fixture(scope="module")
def edge_batch(zt):
    """(plaintexts, passwords, helper ciphertexts) at every length where the
    encrypt kernels take another path; computed once (about 1.2 MiB through
    the helper)."""
    t, c = zt.zipcrypto_geometry()
    lens = [0, 1, 11, 12, 13, c - 1, c, c + 1, 64 * c - 1, 64 * c + 1, t - 1, t, t + 1, 2 * t + 1, 3 * t + c + 5,
            65 * t + 7]
    assert sum(lens) < (3 << 19)
    items = [rnd(100 + i, n) for i, n in enumerate(lens)]
    pws = [PASSWORDS[i % 4] for i in range(len(lens))]
    return items, pws, [zc.crypt(p, d) for p, d in zip(pws, items)]


def test_raw_encrypt_matches_helper(zt, edge_batch):
    items, pws, want = edge_batch
    got = zt.zipcrypto_encrypt(items, pws)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, len(w))


def test_raw_decrypt_matches_helper(zt, edge_batch):
    items, pws, cts = edge_batch
    got = zt.zipcrypto_decrypt(cts, pws)
    for i, (g, w) in enumerate(zip(got, items)):
        assert g == w, (i, len(w))
    # 130 streams of differing lengths: lanes diverge, more than two waves
    many = [rnd(300 + i, (i * 37) % 1000 + i) for i in range(130)]
    mpw = [PASSWORDS[i % 4] for i in range(130)]
    mct = [zc.crypt(p, d) for p, d in zip(mpw, many)]
    assert zt.zipcrypto_decrypt(mct, mpw) == many
    assert zt.zipcrypto_encrypt(many, mpw) == mct


def test_large_item_beside_small_ones(zt):
    big = rnd(7, (8 << 20) + 5)
    items = [rnd(1000 + i, (i * 53) % 700) for i in range(150)] + [big] + \
            [rnd(2000 + i, (i * 31) % 900) for i in range(150)]
    pws = [PASSWORDS[i % 4] for i in range(len(items))]
    ct = zt.zipcrypto_encrypt(items, pws)
    assert [len(x) for x in ct] == [len(x) for x in items]
    # a prefix of the ciphertext depends only on the same prefix of the input
    assert ct[150][:256 << 10] == zc.crypt(pws[150], big[:256 << 10])
    for i in (0, 1, 149, 151, 300):
        assert ct[i] == zc.crypt(pws[i], items[i])
    # the serial decrypt kernel undoes the scan-parallel encrypt
    assert zt.zipcrypto_decrypt(ct, pws) == items


def _files(zt, oracle, rec, header="reference", lead=None):
    mt = zt.dos_mtime(DATE[0], DATE[1] + 1, DATE[2], DATE[3], DATE[4], DATE[5])
    out = []
    for f, pw in zip(rec["archive"]["files"], rec["passwords"]):
        o = f["opts"]
        d = dict(data=gen_spec(oracle, f["spec"]), name=f["fn"].encode("latin1"), mtime=mt,
                 method=o.get("compressionMethod", 8), os=o.get("os", 0))
        if "comment" in o:
            d["comment"] = o["comment"].encode("latin1")
        ct = o.get("deflateOptions", {}).get("compressionType")
        if ct is not None:
            d["compression_type"] = ct
        if pw is not None:
            d["password"] = bytes(pw)
            d["crypt_header"] = header
            if lead is not None:
                d["crypt_lead"] = lead
        out.append(d)
    return out


@pytest.mark.parametrize("rec", RECORDS, ids=lambda r: r["name"])
def test_reference_mode_matches_fixture(zt, oracle, rec):
    files = _files(zt, oracle, rec)
    ours = zt.zip_compress(files, comment=bytes(rec["archive"]["comment"]))
    ref = blob_bytes(rec["output"])
    if all(f["method"] == 0 for f in files):
        assert ours == ref
        return
    a, b = parse_zip(ours), parse_zip(ref)
    assert len(a["entries"]) == len(b["entries"]) == len(files)
    assert a["comment"] == b["comment"]
    for ea, eb, f in zip(a["entries"], b["entries"], files):
        for k in ("name", "comment", "method", "crc32", "plain_size", "mtime", "os", "version", "flags"):
            assert ea[k] == eb[k], k
        pw = f.get("password")
        assert ea["flags"] == (0 if pw is None else 1)
        lflags = int.from_bytes(ours[ea["local_offset"] + 6:ea["local_offset"] + 8], "little")
        lcsize = int.from_bytes(ours[ea["local_offset"] + 18:ea["local_offset"] + 22], "little")
        assert lflags == ea["flags"] and lcsize == ea["compressed_size"]
        body = ours[ea["data_off"]:ea["data_off"] + ea["compressed_size"]]
        if pw is not None:
            pt = zc.crypt(pw, body, decrypt=True)
            assert pt[:12] == zc.header(ea["crc32"], 0)
            body = pt[12:]
            assert ea["compressed_size"] == 12 + len(body)
        if f["method"] == 8:
            out, ip = oracle.raw_inflate(body)
            assert out == f["data"] and ip == len(body)
            assert zlib.decompress(body, -15) == f["data"]
        else:
            assert body == f["data"]
            assert body == f["data"] and ea["compressed_size"] == eb["compressed_size"]


def test_pkware_mode_reads_with_zipfile(zt, oracle):
    rec = next(r for r in RECORDS if r["name"] == "mixed methods")
    files = _files(zt, oracle, rec, header="pkware", lead=bytes(range(1, 11)))
    files.append(dict(data=b"", name=b"empty", method=0, password=b"p", crypt_header="pkware"))
    files.append(dict(data=b"x" * 777, name=b"plain", method=8))
    ours = zt.zip_compress(files)
    with zipfile.ZipFile(io.BytesIO(ours)) as zf:
        for f in files:
            assert zf.read(f["name"].decode("latin1"), pwd=b"p") == f["data"]
        zf.setpassword(b"p")
        assert zf.testzip() is None
    with zipfile.ZipFile(io.BytesIO(ours)) as zf:
        with pytest.raises(RuntimeError, match="Bad password"):
            zf.read("m1", pwd=b"not the password")
    # the leading header bytes are the caller's
    e = parse_zip(ours)["entries"][0]
    pt = zc.crypt(b"p", ours[e["data_off"]:e["data_off"] + 12], decrypt=True)
    assert pt == zc.header(e["crc32"], 1, bytes(range(1, 11)))
    # the reference's header form is what zipfile rejects (why there are two)
    ref = zt.zip_compress(_files(zt, oracle, rec))
    with zipfile.ZipFile(io.BytesIO(ref)) as zf:
        with pytest.raises(RuntimeError, match="Bad password"):
            zf.read("m2", pwd=b"p")


@pytest.mark.parametrize("verify", [False, True], ids=["plain", "verify"])
@pytest.mark.parametrize("rec", RECORDS, ids=lambda r: r["name"])
def test_unzip_with_password(zt, oracle, rec, verify):
    arch = blob_bytes(rec["output"])
    want = rec["unzip_verify" if verify else "unzip"]
    datas = [gen_spec(oracle, f["spec"]) for f in rec["archive"]["files"]]
    # one call per distinct password of the archive (zt_unzip_pw takes one)
    for pw in {bytes(p) for p in rec["passwords"] if p is not None}:
        err, ents = zt.unzip(arch, verify=verify, password=pw)
        assert [e["name"].decode("latin1") for e in ents] == want["names"]
        for e, w, p, d in zip(ents, want["files"], rec["passwords"], datas):
            if p is None or bytes(p) == pw:
                assert e["status"] == 0, e["message"]
                assert e["data"] == d and len(d) == w["out"]["len"]
            elif verify:
                assert e["status"] != 0  # another entry's password
        if all(p is None or bytes(p) == pw for p in rec["passwords"]):
            assert err is None
    # no password: only the protected entries fail, with the reference's message
    err, ents = zt.unzip(arch, verify=verify)
    for e, w, d in zip(ents, rec["unzip_no_password"]["files"], datas):
        if w["ok"]:
            assert e["status"] == 0 and e["data"] == d
        else:
            assert e["status"] == -52 and e["message"] == w["error"]["message"]
    assert err is not None and err.msg == "encrypted: please set password"


def test_unzip_wrong_password_and_input_untouched(zt):
    for rec in RECORDS:
        arch = blob_bytes(rec["output"])
        buf = ctypes.create_string_buffer(arch, len(arch))
        out = ctypes.POINTER(ctypes.c_uint8)()
        olen, cnt = ctypes.c_size_t(), ctypes.c_size_t()
        ents = ctypes.POINTER(zt.UnzipEntry)()
        for pw in (b"wrong password", bytes(next(p for p in rec["passwords"] if p is not None))):
            rc = zt.lib.zt_unzip_pw(buf, len(arch), 1, pw, len(pw), ctypes.byref(out), ctypes.byref(olen),
                                    ctypes.byref(ents), ctypes.byref(cnt))
            assert cnt.value == len(rec["passwords"])
            if pw == b"wrong password":
                assert rc != 0
                for i, (p, f) in enumerate(zip(rec["passwords"], rec["archive"]["files"])):
                    # (an empty STORE entry has no data byte a wrong key could change, and like the
                    # reference the engine does not check the header bytes: it alone cannot fail)
                    hollow = f["spec"].get("ascii") == "" and f["opts"].get("compressionMethod", 8) == 0
                    assert (ents[i].status != 0) == (p is not None and not hollow), (rec["name"], i, ents[i].message)
            zt.lib.zt_free(out)
            zt.lib.zt_free(ents)
            assert buf.raw == arch  # the reference decrypts its input in place; the engine does not


def test_round_trip_300_members(zt):
    sizes = [0, 1, 100, 5000, 40000, 200000]
    files = []
    for i in range(300):
        n = sizes[(i * 7 + i // 6) % 6]
        data = (rnd(5000 + i, n) if i % 3 == 0 else (b"member %d of the archive. " % i) * (n // 20 + 1))[:n]
        files.append(dict(data=data, name=b"f%03d" % i, method=8 if i % 2 else 0, password=b"one password",
                          crypt_header="pkware" if i % 5 == 0 else "reference"))
    arch = zt.zip_compress(files)
    err, ents = zt.unzip(arch, verify=True, password=b"one password")
    assert err is None
    assert [e["data"] for e in ents] == [f["data"] for f in files]
    assert all(e["flags"] == 1 for e in ents)


def test_unzip_data_descriptor_and_short_header(zt):
    ents = [dict(name=b"dd-deflate", data=b"streamed member " * 400, method=8, password=b"pw", dd=True),
            dict(name=b"dd-stored", data=rnd(9, 3000), method=0, password=b"pw", dd=True),
            dict(name=b"sized", data=rnd(10, 100), method=0, password=b"pw", mode=1),
            dict(name=b"plain", data=b"not protected", method=8)]
    # (no verify: a data descriptor leaves the local header's CRC 0, which is what verify compares)
    err, got = zt.unzip(zc.build_zip(ents), password=b"pw")
    assert err is None
    assert [g["data"] for g in got] == [e["data"] for e in ents]
    assert [g["data_crc32"] for g in got] == [zlib.crc32(e["data"]) for e in ents]
    # an encrypted entry shorter than its header: the reference reads garbage, the engine says so
    short = bytearray(zc.build_zip([dict(name=b"s", data=b"", method=0, password=b"pw")]))
    p = parse_zip(bytes(short))["entries"][0]
    short[p["local_offset"] + 18:p["local_offset"] + 22] = (5).to_bytes(4, "little")
    err, got = zt.unzip(bytes(short), password=b"pw")
    assert got[0]["status"] == -50 and got[0]["message"] == "invalid encryption header size"
    assert err is not None and err.code == -50


def test_no_crypt_calls_equal_the_old_ones(zt, oracle):
    rec = next(r for r in load("zip.json")["records"] if r["kind"] == "zip" and r["name"] == "mixed methods")
    mt = zt.dos_mtime(DATE[0], DATE[1] + 1, DATE[2], DATE[3], DATE[4], DATE[5])
    files = []
    for f in rec["archive"]["files"]:
        o = f["opts"]
        d = dict(data=gen_spec(oracle, f["spec"]), name=f["fn"].encode("latin1"), mtime=mt,
                 method=o.get("compressionMethod", 8), os=o.get("os", 0))
        ct = o.get("deflateOptions", {}).get("compressionType")
        if ct is not None:
            d["compression_type"] = ct
        files.append(d)
    comment = bytes(rec["archive"]["comment"])
    old = zt.zip_compress(files, comment=comment)
    assert zt.zip_compress(files, comment=comment, pw_call=True) == old
    for verify in (False, True):
        e0, a = zt.unzip(old, verify=verify)
        e1, b = zt.unzip(old, verify=verify, pw_call=True)
        assert e0 is None and e1 is None and a == b
        assert [x["data"] for x in a] == [f["data"] for f in files]
