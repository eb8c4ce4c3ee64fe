"""The BGZF classes of the Node facade (zlib.ts_amd/lib BGZF.js: BGZip, BGUnzip
over zt.node): write, read, ranges and virtual-offset chunks on the two range
files of tests/test_gpu_bgzf.py, against the original data and the Python
call's .gzi; one error with the reference-style message."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

import bgzf_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "zlib.ts_amd", "zt.node")
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not NODE or not os.path.exists(ADDON), reason="node or zt.node missing")]


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def test_facade_bgzf(tmp_path, oracle):
    import ztamd

    inputs = {"a": (oracle.gen("structured", 13, 12 * 4096 - 123), 4096),
              "b": (oracle.gen("wordsalad", 11, 4 * 65280 + 1000), 65280)}
    cases, want = [], {}
    for name, (data, bs) in inputs.items():
        f, gzi = ztamd.bgzf_compress(data, block_size=bs, want_index=True)
        blocks = bgzf_py.walk(f)
        (tmp_path / f"{name}.raw").write_bytes(data)
        (tmp_path / f"{name}.bgz").write_bytes(f)
        total = len(data)
        ranges = [[0, 1], [bs - 3, 7], [total - 1, 1], [total, 5], [2 * bs, bs + 1], [0, 1]]
        virtual = [[str(bgzf_py.voffset(blocks[1].offset, 10)), str(bgzf_py.voffset(blocks[1].offset, 900))],
                   [str(bgzf_py.voffset(blocks[1].offset, bs - 100)), str(bgzf_py.voffset(blocks[3].offset, 17))],
                   [str(bgzf_py.voffset(blocks[2].offset, 5)), str(bgzf_py.voffset(blocks[2].offset, 5))]]
        cases.append({"id": f"{name} write", "file": str(tmp_path / f"{name}.raw"),
                      "compress": {"blockSize": bs if bs != 65280 else 0, "level": 6}})
        cases.append({"id": f"{name} read", "file": str(tmp_path / f"{name}.bgz"), "decompress": True,
                      "ranges": ranges, "range": [bs + 5, 300], "virtual": virtual})
        want[name] = (data, f, gzi, ranges, bs)
    # one error: the CRC field of block 2 of file a
    data, f, gzi, ranges, bs = want["a"]
    b2 = bgzf_py.walk(f)[2]
    bad = bytearray(f)
    bad[b2.offset + b2.size - 8] ^= 1
    (tmp_path / "bad.bgz").write_bytes(bytes(bad))
    cases.append({"id": "bad", "file": str(tmp_path / "bad.bgz"), "decompress": True})
    cases.append({"id": "bad ranges", "file": str(tmp_path / "bad.bgz"), "ranges": [[0, 10], [2 * bs + 1, 10]]})
    cases.append({"id": "not bgzf", "file": str(tmp_path / "a.raw"), "decompress": True})
    cfile = tmp_path / "cases.json"
    cfile.write_text(json.dumps(cases))
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "bgzf_check.mjs"), str(cfile)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    doc = json.loads(p.stdout.strip().splitlines()[-1])
    assert doc["codes"] == [-70, -71]
    assert doc["voffset"] == str(bgzf_py.voffset(70000, 123))
    res = {r["id"]: r for r in doc["results"]}
    for name, (data, f, gzi, ranges, bs) in want.items():
        w, r = res[f"{name} write"], res[f"{name} read"]
        assert "error" not in w and "error" not in r, (w, r)
        assert w["file"] == _sha(f) and w["gzi"] == _sha(gzi) and w["roundTrip"] and w["plainHasNoIndex"]
        assert r["output"] == _sha(data) and r["built"] == _sha(gzi)
        for key in ("walked", "indexed"):
            for (off, ln), got in zip(ranges, r[key]):
                assert bytes.fromhex(got) == data[off:off + ln], (name, key, off, ln)
        assert bytes.fromhex(r["range"]) == data[bs + 5:bs + 305]
        v = [data[bs + 10:bs + 900], data[2 * bs - 100:3 * bs + 17], b""]
        assert [bytes.fromhex(x) for x in r["virtual"]] == v and [bytes.fromhex(x) for x in r["chunks"]] == v
    with pytest.raises(ztamd.ZtError) as e:
        ztamd.gunzip(bytes(bad[b2.offset:b2.offset + b2.size]))
    assert res["bad"]["error"] == {"message": e.value.msg, "status": e.value.code} and e.value.code == -33
    assert res["bad ranges"]["error"] == {"message": e.value.msg, "status": e.value.code}
    assert res["not bgzf"]["error"]["status"] == -70
    assert res["not bgzf"]["error"]["message"].startswith("not a BGZF block at offset 0: ")
