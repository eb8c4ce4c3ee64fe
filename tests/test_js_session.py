"""RawInflateSession of the Node facade (zlib.ts_amd/lib/InflateSession.js over
zt.node's session bindings): a stream pushed in 9 pieces, only the new bytes
each time, against the data it was made from."""
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
        p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "session_check.mjs"), path],
                           capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(path)
    assert p.returncode == 0, p.stderr
    return {r["id"]: r for r in json.loads(p.stdout.strip().splitlines()[-1])}


@pytest.mark.gpu
def test_session_pieces(oracle):
    rng = random.Random(9)
    data = oracle.gen("wordsalad", 3, 200_000) + oracle.gen("xorshift32", 3, 30_000)
    ref_stream, _ = oracle.raw_deflate(data)  # one block for the whole input
    zc = zlib.compressobj(6, zlib.DEFLATED, -15)
    z_raw = zc.compress(data) + zc.flush()
    cases = []
    for name, s in [("ref", ref_stream), ("zlib", z_raw)]:
        cuts = sorted(rng.sample(range(1, len(s)), 8)) + [len(s)]
        cases.append({"id": name, "op": "session", "in": s.hex(), "cuts": cuts})
    cases.append({"id": "many", "op": "many", "in": z_raw.hex(), "cuts": [len(z_raw) // 3, len(z_raw)]})
    cases.append({"id": "bad", "op": "bad", "in": (b"\x07" + bytes(64)).hex()})
    res = run_cases(cases)
    for name in ("ref", "zlib"):
        r = res[name]
        assert "error" not in r, r.get("error")
        assert bytes.fromhex(r["out"]) == data, name
        assert r["finished"] and r["unused"] == 0 and r["closed"]
        assert r["crc32"] == zlib.crc32(data) and r["adler32"] == zlib.adler32(data)
        assert len(r["calls"]) == 9
    # the one-block stream yields output before its last piece: the session resumes at a token
    assert sum(1 for n in res["ref"]["calls"][:-1] if n) >= 7
    assert "error" not in res["many"], res["many"].get("error")
    assert [bytes.fromhex(x) for x in res["many"]["outs"]] == [data, data] and res["many"]["finished"]
    assert res["bad"]["error"] == {"message": "unknown BTYPE: 3", "status": -12}
