"""GUnzip.decompressBatch and Inflate.decompressBatch of the Node facade
(zlib.ts_amd/lib over zt.node: zt_gunzip_batch, zt_zlib_decompress_batch),
against the Python binding's results for the same batches."""
import json
import os
import shutil
import subprocess
import tempfile
import zlib

import pytest

import dict_corpus
from container_batch_corpus import data_of, frame, gzip_member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "zlib.ts_amd", "zt.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not NODE or not os.path.exists(ADDON),
                                                  reason="node or zt.node missing")]


def run_batches(batches):
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(batches, f)
        path = f.name
    try:
        p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "container_batch_check.mjs"), path],
                           capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(path)
    assert p.returncode == 0, p.stderr
    return {r["id"]: r for r in json.loads(p.stdout.strip().splitlines()[-1])}


def test_facade_container_batches(oracle):
    import ztamd as zt

    assert zt.device_count() > 0, "no GPU visible"
    d = [data_of(oracle, 300 + k, (1, 900, 5000, 70000)[k % 4]) for k in range(8)]
    multi = b"".join(frame(d[k], name=b"part%d" % k, comment=b"c%d" % k, extra=b"xy", mtime=5 + k) for k in range(4))
    g = gzip_member(d[5])
    hcrc = zt.gzip_compress(d[2], name=b"h", hcrc=True, mtime=9)[0]
    gz = [gzip_member(d[0]), multi, g[:-8] + bytes([g[-8] ^ 1]) + g[-7:], hcrc, g[:len(g) // 2], b"\x1f\x8b\x07" + g[3:],
          gzip_member(d[3], 9), b"", g + b"tail"]
    D = dict_corpus.dictionary()
    msgs = dict_corpus.messages(8)
    c = zlib.compressobj(zdict=D)
    fd = c.compress(msgs[0]) + c.flush()
    ok = zlib.compress(d[1])
    zl = [ok, zt.zlib_compress_batch([msgs[1]], dictionary=D)[0], fd, ok[:-1] + bytes([ok[-1] ^ 1]),
          bytes([ok[0], ok[1] ^ 1]) + ok[2:], zlib.compress(d[3], 1), b"\x77" + ok[1:]]
    wrong = D[:-1] + b"?"
    res = run_batches([
        {"id": "gz", "op": "gunzip", "items": [x.hex() for x in gz]},
        {"id": "zl_plain", "op": "inflate", "items": [x.hex() for x in zl], "opts": {"verify": True}},
        {"id": "zl_dict", "op": "inflate", "items": [x.hex() for x in zl], "opts": {"verify": True},
         "dictionary": D.hex()},
        {"id": "zl_dict_nov", "op": "inflate", "items": [x.hex() for x in zl], "dictionary": D.hex()},
        {"id": "zl_wrong", "op": "inflate", "items": [x.hex() for x in zl], "dictionary": wrong.hex()},
        {"id": "empty", "op": "gunzip", "items": []},
    ])
    for r in res.values():
        assert "error" not in r and r["isArray"], r
    assert res["empty"]["items"] == []
    # gzip: per item what the Python binding gives
    want = zt.gunzip_batch(gz)
    assert len(res["gz"]["items"]) == len(gz)
    seen_error = seen_multi = False
    for js, (st, out, members) in zip(res["gz"]["items"], want):
        if st != 0:
            assert js["error"] == {"message": st.message, "status": int(st)}
            seen_error = True
            continue
        assert bytes.fromhex(js["out"]) == out and len(js["members"]) == len(members)
        seen_multi = seen_multi or len(members) > 1
        for jm, m in zip(js["members"], members):
            assert (jm["flg"], jm["mtime"], jm["xfl"], jm["os"]) == (m["flg"], m["mtime"], m["xfl"], m["os"])
            assert jm.get("name") == (None if m["name"] is None else m["name"].decode("latin1"))
            assert jm.get("comment") == (None if m["comment"] is None else m["comment"].decode("latin1"))
            assert jm.get("xlen") == (m["xlen"] if m["flg"] & 4 else None)
            assert jm.get("crc16") == (m["crc16"] if m["has_crc16"] else None)
            assert bytes.fromhex(jm["data"]) == m["data"]
    assert seen_error and seen_multi
    # zlib: the same
    for key, kw in (("zl_plain", dict(verify=True)), ("zl_dict", dict(verify=True, dictionary=D)),
                    ("zl_dict_nov", dict(dictionary=D)), ("zl_wrong", dict(dictionary=wrong))):
        want = zt.zlib_decompress_batch(zl, **kw)
        oks = 0
        for js, (st, out, ip, adler) in zip(res[key]["items"], want):
            if st != 0:
                assert js["error"] == {"message": st.message, "status": int(st)}, key
                continue
            oks += 1
            assert bytes.fromhex(js["out"]) == out and js["ip"] == ip
            assert js.get("adler32") == (adler if kw.get("verify") else None)
        assert 0 < oks < len(zl), key
    assert [x["error"]["status"] for x in res["zl_wrong"]["items"][1:3]] == [-44, -44]
    assert [x["error"]["status"] for x in res["zl_plain"]["items"][1:3]] == [-42, -42]
    assert bytes.fromhex(res["zl_dict"]["items"][2]["out"]) == msgs[0]
