"""The `strategy` option of the Node facade (RawDeflate, Deflate, GZip's
deflateOptions; include/zt_strategy.h): it reaches the library -- the streams
are the Python facade's, byte for byte -- and their tokens obey the strategy."""
import gzip
import json
import os
import shutil
import subprocess
import tempfile
import zlib

import pytest

import deflate_audit
import lz77_ref
import strategy_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "zlib.ts_amd", "zt.node")
pytestmark = pytest.mark.skipif(not NODE or not os.path.exists(ADDON), reason="node or zt.node missing")


def run_cases(cases):
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(cases, f)
        path = f.name
    try:
        p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "strategy_check.mjs"), path],
                           capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(path)
    assert p.returncode == 0, p.stderr
    return {r["id"]: r for r in json.loads(p.stdout.strip().splitlines()[-1])}


@pytest.mark.gpu
def test_strategy_option(oracle):
    import ztamd

    _, _, info = ztamd.debug_match_strategy(b"\0" * 64, sr.RLE)
    g = lz77_ref.Geom(info["block"], info["segment"], 0)
    data = sr.run_structured(90000, 3).tobytes() + oracle.gen("structured", 4, 50000)
    cases = [{"id": "constants", "op": "constants", "in": ""}]
    for name, st in (("rle", sr.RLE), ("huff", sr.HUFFMAN_ONLY), ("default", 0), ("none", None)):
        opts = {} if st is None else {"strategy": st}
        for op in ("raw", "zlib", "gzip"):
            cases.append({"id": f"{op}-{name}", "op": op, "in": data.hex(), "opts": opts})
    cases.append({"id": "raw-fixed-l1", "op": "raw", "in": data.hex(),
                  "opts": {"strategy": sr.RLE, "compressionType": 1, "level": 1}})
    cases.append({"id": "bad", "op": "raw", "in": data[:100].hex(), "opts": {"strategy": 4}})
    cases.append({"id": "bad-gzip", "op": "gzip", "in": data[:100].hex(), "opts": {"strategy": 1}})
    cases.append({"id": "dict", "op": "raw", "in": data[:100].hex(), "opts": {"strategy": sr.RLE},
                  "dictionary": data[:50].hex()})
    cases.append({"id": "index", "op": "gzip", "in": data[:100].hex(), "opts": {"strategy": sr.RLE},
                  "buildIndex": True})
    res = run_cases(cases)
    assert res["constants"]["constants"] == {"DEFAULT": 0, "HUFFMAN_ONLY": 2, "RLE": 3}
    for name, st in (("rle", sr.RLE), ("huff", sr.HUFFMAN_ONLY), ("default", 0), ("none", None)):
        for op in ("raw", "zlib", "gzip"):
            assert "error" not in res[f"{op}-{name}"], res[f"{op}-{name}"].get("error")
        raw = bytes.fromhex(res[f"raw-{name}"]["out"])
        z = bytes.fromhex(res[f"zlib-{name}"]["out"])
        gz = bytes.fromhex(res[f"gzip-{name}"]["out"])
        assert res[f"raw-{name}"]["strategy"] == st and res[f"zlib-{name}"]["strategy"] == st
        assert zlib.decompress(raw, -15) == data and zlib.decompress(z) == data and gzip.decompress(gz) == data
        assert res[f"zlib-{name}"]["adler32"] == zlib.adler32(data)
        assert res[f"gzip-{name}"]["crc32"] == zlib.crc32(data)
        assert raw == ztamd.deflate_raw(data, strategy=st)
        assert z == ztamd.zlib_compress(data, strategy=st)[0]
        assert gz == ztamd.gzip_compress(data, mtime=7, strategy=st)[0]
        if st in (sr.RLE, sr.HUFFMAN_ONLY):
            for stream in (raw, z[2:], gz[10:]):
                n = sr.check_tokens(st, deflate_audit.parse(stream), data, g)
                assert (n > 100) if st == sr.RLE else (n == 0)
    assert bytes.fromhex(res["raw-default"]["out"]) == bytes.fromhex(res["raw-none"]["out"])
    assert bytes.fromhex(res["raw-fixed-l1"]["out"]) == ztamd.deflate_raw(data, compression_type=1, level=1,
                                                                          strategy=sr.RLE)
    assert res["bad"]["error"] == {"message": "invalid strategy: 4", "status": -103}
    assert res["bad-gzip"]["error"] == {"message": "invalid strategy: 1", "status": -103}
    assert res["dict"]["error"]["status"] == -103 and res["index"]["error"]["status"] == -103
