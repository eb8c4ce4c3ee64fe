"""The checkpoint methods of the Node facade (zlib.ts_amd/lib RawInflate:
buildCheckpoints / decompressRangeAt / decompressRangesAt over zt.node) on
streams without sync points, against slices of the original input."""
import json
import os
import shutil
import subprocess
import zlib

import pytest

import index_corpus
from index_corpus import MIB, TOTAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "zlib.ts_amd", "zt.node")
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not NODE or not os.path.exists(ADDON), reason="node or zt.node missing")]


def test_facade_checkpoints(tmp_path, oracle):
    import ztamd

    data = index_corpus.corpus(oracle)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    zlib6 = co.compress(data) + co.flush()
    reference = oracle.raw_deflate(data)[0]
    ix = ztamd.inflate_index_build(ztamd.deflate_raw(data[:200000], level=6))  # a sync-point index: the wrong blob
    files = {"zlib6": zlib6, "prefixed": b"0123456789" + zlib6, "reference": reference, "ztix": ix,
             "cut": ztamd.inflate_ckpt_build(zlib6, span=256 << 10)[:-1]}
    for name, b in files.items():
        (tmp_path / name).write_bytes(b)
    ranges = [[0, 1], [MIB - 70000, 140000], [TOTAL - 3, 100], [2 * MIB - 1, 2], [0, 1]]
    span = {"span": 256 << 10}
    cases = [
        {"id": "zlib6", "file": str(tmp_path / "zlib6"), "build": span, "range": [3 * MIB // 2, 1000],
         "ranges": ranges},
        {"id": "prefixed", "file": str(tmp_path / "prefixed"), "opts": {"index": 10}, "range": [2 * MIB - 1, 2],
         "ranges": ranges},
        {"id": "reference", "file": str(tmp_path / "reference"), "build": span, "range": [MIB, 70000],
         "ranges": ranges},
        {"id": "wrong-blob", "file": str(tmp_path / "zlib6"), "blobFile": str(tmp_path / "ztix"), "range": [0, 1]},
        {"id": "cut-blob", "file": str(tmp_path / "zlib6"), "blobFile": str(tmp_path / "cut"), "ranges": ranges},
        {"id": "small-span", "file": str(tmp_path / "zlib6"), "build": {"span": 1000}},
    ]
    cfile = tmp_path / "cases.json"
    cfile.write_text(json.dumps(cases))
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "ckpt_check.mjs"), str(cfile)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    doc = json.loads(p.stdout.strip().splitlines()[-1])
    assert doc["codes"] == [-60, -61, -62]
    res = {r["id"]: r for r in doc["results"]}
    for k in ("zlib6", "prefixed", "reference"):
        r = res[k]
        assert "error" not in r, r
        assert r["magic"] == "ZTCK"
        assert r["blobLength"] == 64 + 48 * (r["nunits"] + 1) + 32784 * r["nwin"]
        for (off, length), got in zip(ranges, r["ranges"]):
            assert bytes.fromhex(got) == data[off:off + length], (k, off, length)
    assert res["zlib6"]["nwin"] >= 8 and res["reference"]["nwin"] >= 8
    assert res["prefixed"]["nwin"] == 2, "the default span is 1 MiB"
    assert bytes.fromhex(res["zlib6"]["range"]) == data[3 * MIB // 2:3 * MIB // 2 + 1000]
    assert bytes.fromhex(res["prefixed"]["range"]) == data[2 * MIB - 1:2 * MIB + 1]
    assert bytes.fromhex(res["reference"]["range"]) == data[MIB:MIB + 70000]
    assert res["prefixed"]["ip"] == 10, "the range methods leave ip alone"
    assert res["wrong-blob"]["error"]["status"] == -61
    assert res["cut-blob"]["error"]["status"] == -61
    assert res["small-span"]["error"]["status"] == -103
