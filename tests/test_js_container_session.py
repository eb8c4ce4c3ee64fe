"""GUnzipSession and ZlibInflateSession of the Node facade
(zlib.ts_amd/lib/ContainerSession.js over zt.node's container-session
bindings): a gzip file of three members and a zlib stream pushed in pieces,
only the new bytes each time, against the data they were made from; the
member records; a reference error; and pushMany over both kinds."""
import gzip
import json
import os
import random
import shutil
import subprocess
import tempfile
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "zlib.ts_amd", "zt.node")
pytestmark = pytest.mark.skipif(not NODE or not os.path.exists(ADDON), reason="node or zt.node missing")


def run_cases(cases):
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(cases, f)
        path = f.name
    try:
        p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "container_session_check.mjs"), path],
                           capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(path)
    assert p.returncode == 0, p.stderr
    return {r["id"]: r for r in json.loads(p.stdout.strip().splitlines()[-1])}


def test_facade_exports_the_classes():
    p = subprocess.run([NODE, "--input-type=module", "-e",
                        "import * as m from '%s'; console.log(typeof m.GUnzipSession, typeof m.ZlibInflateSession, "
                        "typeof m.GUnzipSession.pushMany)" % os.path.join(ROOT, "zlib.ts_amd", "lib", "index.js")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.split() == ["function"] * 3


@pytest.mark.gpu
def test_container_session_pieces(oracle):
    import ztamd

    rng = random.Random(10)
    parts = [oracle.gen("wordsalad", 4, 60_000), b"", oracle.gen("xorshift32", 4, 9_000)]
    data = b"".join(parts)
    gz = (gzip.compress(parts[0], 6, mtime=5) + gzip.compress(parts[1], 6, mtime=6)
          + gzip.compress(parts[2], 1, mtime=7))
    assert gzip.decompress(gz) == data
    dic = oracle.gen("wordsalad", 4, 2000)
    zc = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, dic)
    zs = zc.compress(parts[0]) + zc.flush() + b"tail"
    plain = zlib.compress(parts[2], 6)
    cases = []
    for name, kind, s, extra in [("gz", "gzip", gz, {}), ("zl", "zlib", zs, {"dict": dic.hex()})]:
        cuts = sorted(rng.sample(range(1, len(s)), 8)) + [len(s)]
        cases.append(dict({"id": name, "op": "session", "kind": kind, "in": s.hex(), "cuts": cuts}, **extra))
    cases.append({"id": "many", "op": "many", "in": gz.hex(), "in2": plain.hex(), "rounds": 3})
    bad_gz = gz[:-5] + bytes([gz[-5] ^ 1]) + gz[-4:]  # the last member's CRC-32
    bad_zl = plain[:-1] + bytes([plain[-1] ^ 1])
    cases.append({"id": "bad_gz", "op": "bad", "kind": "gzip", "in": bad_gz.hex()})
    cases.append({"id": "bad_zl", "op": "bad", "kind": "zlib", "in": bad_zl.hex()})
    cases.append({"id": "fdict", "op": "bad", "kind": "zlib", "in": zs.hex()})
    res = run_cases(cases)

    r = res["gz"]
    assert "error" not in r, r.get("error")
    assert bytes.fromhex(r["out"]) == data and r["finished"] and r["unused"] == 0 and r["closed"]
    assert len(r["calls"]) == 9 and sum(1 for n in r["calls"] if n) >= 8
    _, ref_members = ztamd.gunzip(gz)
    assert len(r["members"]) == 3
    for m, w in zip(r["members"], ref_members):
        assert (m["flg"], m["mtime"], m["crc32"], m["isize"], m["dataOff"], m["dataLen"]) == (
            w["flg"], w["mtime"], w["crc32"], w["isize"], w["data_off"], w["data_len"])
        assert m["name"] is None and m["comment"] is None
    assert [m["inOff"] for m in r["members"]] == [0, len(gzip.compress(parts[0], 6, mtime=5)),
                                                   len(gz) - len(gzip.compress(parts[2], 1, mtime=7))]
    r = res["zl"]
    assert "error" not in r, r.get("error")
    assert bytes.fromhex(r["out"]) == parts[0] and r["finished"] and r["unused"] == 4 and r["closed"]
    assert len(r["members"]) == 1 and r["members"][0]["crc32"] == zlib.adler32(parts[0])

    assert "error" not in res["many"], res["many"].get("error")
    assert [bytes.fromhex(x) for x in res["many"]["outs"]] == [data, parts[2]]
    assert res["many"]["finished"] and res["many"]["statuses"] == [0, 0]

    # the thrown errors are the one-shot calls'
    for name, call in (("bad_gz", lambda: ztamd.gunzip(bad_gz)),
                       ("bad_zl", lambda: ztamd.zlib_decompress(bad_zl, verify=True)),
                       ("fdict", lambda: ztamd.zlib_decompress(zs, verify=True))):
        with pytest.raises(ztamd.ZtError) as e:
            call()
        assert res[name]["error"] == {"message": e.value.msg, "status": e.value.code}, name
    # push()'s error carries what the call decoded before it: here every member's bytes (the last CRC-32 is wrong)
    assert bytes.fromhex(res["bad_gz"]["errorOutput"]) == data
    assert bytes.fromhex(res["bad_zl"]["errorOutput"]) == parts[2] and res["fdict"]["errorOutput"] == ""
