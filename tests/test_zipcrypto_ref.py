"""The password fixtures the reference wrote (tests/golden/zipcrypto.json,
tools/gen_golden_zipcrypto.mjs) against the pure-Python cipher of
tests/zipcrypto_py.py -- this pins the checker of the GPU tests
(tests/test_gpu_zipcrypto.py) to the reference -- and the C boundary of
include/zt_zipcrypto.h without a GPU."""
import ctypes
import hashlib
import os
import re
import zlib

import pytest

import zipcrypto_py as zc
from golden_util import blob_bytes, load
from test_zip_fixtures import gen_spec, parse_zip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zt_zipcrypto.h")
FIX = load("zipcrypto.json")
RECORDS = FIX["records"]


def declared_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zt_[a-z0-9_]+)\s*\(", text)))


def test_fixture_covers_the_cases():
    names = {r["name"] for r in RECORDS}
    assert {"store only", "deflate", "mixed methods", "per-file password", "empty files",
            "high password bytes"} <= names
    assert any(b >= 0x80 for r in RECORDS for p in r["passwords"] if p for b in p)


@pytest.mark.parametrize("rec", RECORDS, ids=lambda r: r["name"])
def test_helper_decrypts_reference_archives(oracle, rec):
    arch = blob_bytes(rec["output"])
    p = parse_zip(arch)
    files = rec["archive"]["files"]
    assert [e["name"].decode("latin1") for e in p["entries"]] == rec["unzip"]["names"]
    for e, f, pw, want, want_v in zip(p["entries"], files, rec["passwords"], rec["unzip"]["files"],
                                      rec["unzip_verify"]["files"]):
        data = gen_spec(oracle, f["spec"])
        ct = arch[e["data_off"]:e["data_off"] + e["compressed_size"]]
        assert e["flags"] == (0 if pw is None else 1)
        if pw is None:
            body = ct
        else:
            pt = zc.crypt(bytes(pw), ct, decrypt=True)
            assert pt[:12] == zc.header(e["crc32"], 0)  # src/Zip.ts:169-174
            body = pt[12:]
            # and the helper's encode gives the reference's exact bytes back
            assert zc.crypt(bytes(pw), pt) == ct
            if e["method"] == 0:
                assert zc.crypt(bytes(pw), zc.header(zlib.crc32(data), 0) + data) == ct
        out = zlib.decompress(body, -15) if e["method"] == 8 else body
        assert out == data and e["crc32"] == zlib.crc32(data)
        for w in (want, want_v):
            assert w["ok"] and w["out"]["len"] == len(out)
            assert w["out"]["sha256"] == hashlib.sha256(out).hexdigest()


@pytest.mark.parametrize("rec", RECORDS, ids=lambda r: r["name"])
def test_no_password_record(rec):
    for pw, w in zip(rec["passwords"], rec["unzip_no_password"]["files"]):
        if pw is None:
            assert w["ok"]
        else:
            assert not w["ok"] and w["error"]["message"] == "encrypted: please set password"


def test_builder_makes_archives_zipfile_reads():
    import io
    import zipfile

    ents = [dict(name=b"s", data=b"stored " * 50, method=0, password=b"pw", mode=1, lead=bytes(range(10))),
            dict(name=b"d", data=b"deflated " * 500, method=8, password=b"pw", mode=1),
            dict(name=b"plain", data=b"open", method=0)]
    with zipfile.ZipFile(io.BytesIO(zc.build_zip(ents))) as zf:
        for e in ents:
            assert zf.read(e["name"].decode(), pwd=b"pw") == e["data"]


def test_library_exports_every_declared_symbol():
    import ztamd

    lib = ctypes.CDLL(ztamd.LIBPATH)
    names = declared_functions()
    for want in ("zt_zipcrypto_encrypt_batch", "zt_zipcrypto_decrypt_batch", "zt_zipcrypto_tile_bytes",
                 "zt_zipcrypto_chunk_bytes", "zt_zip_compress_pw", "zt_unzip_pw"):
        assert want in names
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert sorted(ztamd.ZIPCRYPTO_SYMBOLS) == names
    assert not set(ztamd.ZIPCRYPTO_SYMBOLS) & set(ztamd.SYMBOLS)
    t, c = ztamd.zipcrypto_geometry()
    assert 0 < c < t <= 16 << 10 and t % c == 0


def test_no_cpu_fallback_without_gpu():
    import torch
    import ztamd

    if torch.cuda.is_available():
        return  # the GPU suite covers the compute path
    stored = blob_bytes(RECORDS[0]["output"])
    for call in (lambda: ztamd.zipcrypto_encrypt([b"abc"], b"pw"), lambda: ztamd.zipcrypto_decrypt([b"abc"], b"pw"),
                 lambda: ztamd.zip_compress([dict(data=b"abc", name=b"a", method=0, password=b"pw")])):
        with pytest.raises(ztamd.ZtError) as ei:
            call()
        assert ei.value.code == -100  # ZT_E_NO_DEVICE
    err, ents = ztamd.unzip(stored, password=b"secret")
    assert err is not None and err.code == -100 and ents == []
