"""The password paths of the Node facade (zlib.ts_amd/lib Zip / Unzip over
zt.node), driven as the reference's callers would drive them, against the
fixtures the reference wrote (tests/golden/zipcrypto.json)."""
import json
import os
import shutil
import subprocess
import tempfile

import pytest

from golden_util import blob_bytes, load
from test_zip_fixtures import DATE, gen_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "zlib.ts_amd", "zt.node")
pytestmark = pytest.mark.skipif(not NODE or not os.path.exists(ADDON), reason="node or zt.node missing")
RECORDS = {r["name"]: r for r in load("zipcrypto.json")["records"]}


def run_cases(cases):
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(cases, f)
        path = f.name
    try:
        p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "zipcrypto_check.mjs"), path],
                           capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(path)
    assert p.returncode == 0, p.stderr
    return {r["id"]: r for r in json.loads(p.stdout.strip().splitlines()[-1])}


def hx(p):
    return None if p is None else {"hex": bytes(p).hex()}


def zip_case(oracle, rec, cid):
    files = []
    for f in rec["archive"]["files"]:
        opts = {k: v for k, v in f["opts"].items() if k != "password"}
        files.append({"fn": f["fn"], "in": gen_spec(oracle, f["spec"]).hex(), "opts": opts,
                      "password": hx(f["opts"].get("password"))})
    return {"id": cid, "op": "zip", "files": files, "date": DATE, "comment": rec["archive"]["comment"],
            "password": hx(rec["archive"]["password"])}


def test_password_refused_without_gpu(oracle):
    import torch

    if torch.cuda.is_available():
        return  # the GPU test covers the compute path
    rec = RECORDS["store only"]
    res = run_cases([zip_case(oracle, rec, "z"),
                     {"id": "u", "op": "unzip", "in": blob_bytes(rec["output"]).hex(), "ctor": {"str": "secret"}}])
    assert res["z"]["error"]["status"] == -100  # no JS cipher behind the facade
    assert res["u"]["error"]["status"] == -100


@pytest.mark.gpu
def test_facade_passwords(oracle):
    store, per_file, mixed = RECORDS["store only"], RECORDS["per-file password"], RECORDS["mixed methods"]
    datas = {n: [gen_spec(oracle, f["spec"]) for f in r["archive"]["files"]] for n, r in RECORDS.items()}
    cases = [zip_case(oracle, store, "zs"), zip_case(oracle, per_file, "zp"), zip_case(oracle, mixed, "zm")]
    # a string password is the same key as its bytes
    zstr = zip_case(oracle, store, "zstr")
    zstr["password"] = {"str": "secret"}
    cases.append(zstr)
    # the pkware header: random lead unless given
    zk = zip_case(oracle, store, "zk")
    for f in zk["files"]:
        f["opts"]["cryptHeader"] = "pkware"
    zk["files"][0]["cryptLead"] = bytes(range(10)).hex()
    cases.append(zk)
    for name, rec in RECORDS.items():
        arch = blob_bytes(rec["output"]).hex()
        # every entry with its own password through getFileData(i, {password})
        cases.append({"id": "each:" + name, "op": "unzip", "in": arch, "verify": True,
                      "each": [hx(p) for p in rec["passwords"]]})
        cases.append({"id": "none:" + name, "op": "unzip", "in": arch, "byName": True})
    arch = blob_bytes(store["output"]).hex()
    cases.append({"id": "ctor", "op": "unzip", "in": arch, "verify": True, "ctor": {"str": "secret"}, "byName": True})
    cases.append({"id": "set", "op": "unzip", "in": arch, "verify": True, "set": hx(b"secret")})
    # the call's password overrides the archive's (src/Unzip.ts:265)
    cases.append({"id": "override", "op": "unzip", "in": blob_bytes(per_file["output"]).hex(), "verify": True,
                  "ctor": hx(per_file["archive"]["password"]),
                  "each": [hx(per_file["passwords"][0]), None, hx(per_file["passwords"][2])]})
    cases.append({"id": "wrong", "op": "unzip", "in": arch, "verify": True, "ctor": {"str": "not it"}})
    res = run_cases(cases)
    for r in res.values():
        assert "error" not in r, r
    # reference-mode STORE archives are the reference's bytes
    assert res["zs"]["out"] == blob_bytes(store["output"]).hex()
    assert res["zstr"]["out"] == res["zs"]["out"]
    assert res["zp"]["out"][:200] == blob_bytes(per_file["output"]).hex()[:200]  # (its first, stored entry)
    for name, rec in RECORDS.items():
        r = res["each:" + name]
        assert r["names"] == rec["unzip"]["names"] and r["inputSame"]
        assert [f["ok"] and bytes.fromhex(f["out"]) for f in r["files"]] == datas[name], name
        for f, w in zip(res["none:" + name]["files"], rec["unzip_no_password"]["files"]):
            assert f["ok"] == w["ok"]
            if not w["ok"]:
                assert f["message"] == w["error"]["message"] == "encrypted: please set password"
    for cid in ("ctor", "set"):
        assert [bytes.fromhex(f["out"]) for f in res[cid]["files"]] == datas["store only"]
    assert [f["ok"] and bytes.fromhex(f["out"]) for f in res["override"]["files"]] == datas["per-file password"]
    assert [f["ok"] for f in res["wrong"]["files"]] == [False] * 3
    assert all(f["message"].startswith("Incorrect crc") for f in res["wrong"]["files"])
    # round trips through the facade itself
    back = run_cases([
        {"id": "m", "op": "unzip", "in": res["zm"]["out"], "verify": True, "ctor": hx(mixed["archive"]["password"])},
        {"id": "p", "op": "unzip", "in": res["zp"]["out"], "verify": True, "each": [hx(p) for p in per_file["passwords"]]},
        {"id": "k", "op": "unzip", "in": res["zk"]["out"], "verify": True, "set": {"str": "secret"}}])
    assert [bytes.fromhex(f["out"]) for f in back["m"]["files"]] == datas["mixed methods"]
    assert [bytes.fromhex(f["out"]) for f in back["p"]["files"]] == datas["per-file password"]
    assert [bytes.fromhex(f["out"]) for f in back["k"]["files"]] == datas["store only"]
    # pkware archives are read by zipfile; the given lead is used, the others are random
    import io
    import zipfile

    import zipcrypto_py as zc
    from test_zip_fixtures import parse_zip

    zk_bytes = bytes.fromhex(res["zk"]["out"])
    with zipfile.ZipFile(io.BytesIO(zk_bytes)) as zf:
        for f, d in zip(store["archive"]["files"], datas["store only"]):
            assert zf.read(f["fn"], pwd=b"secret") == d
    ents = parse_zip(zk_bytes)["entries"]
    heads = [zc.crypt(b"secret", zk_bytes[e["data_off"]:e["data_off"] + 12], decrypt=True) for e in ents]
    assert heads[0] == zc.header(ents[0]["crc32"], 1, bytes(range(10)))
    assert heads[1][:10] != bytes(10) and heads[1][10:] == zc.header(ents[1]["crc32"], 1)[10:]
