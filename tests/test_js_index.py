"""The indexed range methods of the Node facade (zlib.ts_amd/lib RawInflate:
buildIndex / decompressRange / decompressRanges over zt.node), against slices
of the original input."""
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


def test_facade_index(tmp_path, oracle):
    import ztamd

    data = index_corpus.corpus(oracle)
    s = ztamd.deflate_raw(data, level=6)
    flat = zlib.compress(oracle.gen("wordsalad", 5, 256 << 10), 6)[2:-4]  # no sync point
    files = {"plain": s, "prefixed": b"0123456789" + s, "flat": flat}
    for name, b in files.items():
        (tmp_path / name).write_bytes(b)
    ranges = [[0, 1], [MIB - 70000, 140000], [TOTAL - 3, 100]]
    cases = [
        {"id": "plain", "file": str(tmp_path / "plain"), "range": [3 * MIB // 2, 1000], "ranges": ranges},
        {"id": "prefixed", "file": str(tmp_path / "prefixed"), "opts": {"index": 10}, "range": [2 * MIB - 1, 2],
         "ranges": ranges},
        {"id": "flat", "file": str(tmp_path / "flat")},
    ]
    cfile = tmp_path / "cases.json"
    cfile.write_text(json.dumps(cases))
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "index_check.mjs"), str(cfile)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    doc = json.loads(p.stdout.strip().splitlines()[-1])
    assert doc["codes"] == [-60, -61, -62]
    res = {r["id"]: r for r in doc["results"]}
    for k in ("plain", "prefixed"):
        r = res[k]
        assert "error" not in r, r
        assert r["magic"] == "ZTIX" and (r["blobLength"] - 64) % 24 == 0
        for (off, length), got in zip(ranges, r["ranges"]):
            assert bytes.fromhex(got) == data[off:off + length], (k, off, length)
    assert bytes.fromhex(res["plain"]["range"]) == data[3 * MIB // 2:3 * MIB // 2 + 1000]
    assert bytes.fromhex(res["prefixed"]["range"]) == data[2 * MIB - 1:2 * MIB + 1]
    assert res["prefixed"]["ip"] == 10, "the range methods leave ip alone"
    assert res["flat"]["error"] == {"message": "stream has no usable sync points", "status": -60}
