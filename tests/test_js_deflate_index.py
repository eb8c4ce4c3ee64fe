"""The `buildIndex: true` option of the Node facade's writers (zlib.ts_amd/lib
RawDeflate, GZip, Deflate over zt.node): after compress() the stream's range
index is in `.streamIndex`, equal to RawInflate.buildIndex() of the written
bytes, and decompressRange reads slices through it."""
import json
import os
import shutil
import subprocess

import pytest

import index_corpus
from index_corpus import MIB, TOTAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "zlib.ts_amd", "zt.node")
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not NODE or not os.path.exists(ADDON), reason="node or zt.node missing")]


def test_facade_build_index(tmp_path, oracle):
    import ztamd

    data = index_corpus.corpus(oracle)
    (tmp_path / "corpus").write_bytes(data)
    (tmp_path / "empty").write_bytes(b"")
    f = str(tmp_path / "corpus")
    ranges = [[3 * MIB // 2, 1000], [0, 1], [MIB - 70000, 140000], [TOTAL - 3, 100]]
    prefix = bytes(range(1, 11))
    cases = [
        {"id": "raw", "kind": "raw", "file": f, "start": 0, "ranges": ranges},
        {"id": "raw_prefix", "kind": "raw", "file": f, "start": 10, "prefix": prefix.hex(),
         "opts": {"outputIndex": 10, "level": 1}, "ranges": ranges},
        {"id": "gzip", "kind": "gzip", "file": f, "start": 10 + len("corpus.bin") + 1,
         "opts": {"filename": "corpus.bin", "mtime": 1700000000}, "ranges": ranges},
        {"id": "zlib", "kind": "zlib", "file": f, "start": 2, "ranges": ranges},
        {"id": "stored", "kind": "raw", "file": f, "start": 0, "opts": {"compressionType": 0}, "ranges": ranges},
        {"id": "empty", "kind": "zlib", "file": str(tmp_path / "empty"), "start": 2, "ranges": [[0, 0]]},
    ]
    cfile = tmp_path / "cases.json"
    cfile.write_text(json.dumps(cases))
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "deflate_index_check.mjs"), str(cfile)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    res = {r["id"]: r for r in json.loads(p.stdout.strip().splitlines()[-1])["results"]}
    for k in ("raw", "raw_prefix", "gzip", "zlib"):
        r = res[k]
        assert "error" not in r, r
        assert r["sameBytes"] and r["plainHasNoIndex"], k
        assert r["streamIndex"] == r["built"], k
        blob = bytes.fromhex(r["streamIndex"])
        hdr, _ = ztamd.index_entries(blob)
        start = next(c["start"] for c in cases if c["id"] == k)
        assert hdr["stream_start"] == start and hdr["total_out"] == TOTAL
        for (off, length), got in zip(ranges, r["ranges"]):
            assert bytes.fromhex(got) == data[off:off + length], (k, off, length)
        assert bytes.fromhex(r["range"]) == data[3 * MIB // 2:3 * MIB // 2 + 1000]
    # the raw stream's index is the Python binding's too
    s, blob = ztamd.deflate_raw_indexed(data)
    assert bytes.fromhex(res["raw"]["streamIndex"]) == blob and res["raw"]["length"] == len(s)
    # refusals travel as the engine's error
    for k in ("stored", "empty"):
        assert res[k]["error"] == {"message": "stream has no usable sync points", "status": -60}, res[k]
