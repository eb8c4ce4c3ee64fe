"""The `dictionary` option of the Node facade (zlib.ts_amd/lib RawDeflate /
RawInflate / Deflate / Inflate over zt.node), against Python's zlib with
`zdict`."""
import json
import os
import shutil
import subprocess
import tempfile
import zlib

import pytest

import dict_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "zlib.ts_amd", "zt.node")
pytestmark = pytest.mark.skipif(not NODE or not os.path.exists(ADDON), reason="node or zt.node missing")


def run_cases(cases):
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(cases, f)
        path = f.name
    try:
        p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "dict_check.mjs"), path],
                           capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(path)
    assert p.returncode == 0, p.stderr
    return {r["id"]: r for r in json.loads(p.stdout.strip().splitlines()[-1])}


def fdict_stream(msg, d):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, zdict=d)
    return c.compress(msg) + c.flush()


def test_fdict_error_without_option():
    """no GPU needed: the constructor rejects an FDICT stream as the reference does"""
    d = dict_corpus.dictionary()
    fd = fdict_stream(dict_corpus.messages(4)[1], d)
    res = run_cases([{"id": "none", "op": "inflate", "in": fd.hex()},
                     {"id": "empty", "op": "inflate", "in": fd.hex(), "dictionary": ""}])
    assert res["none"]["error"]["message"] == "fdict flag is not supported"
    assert res["empty"]["error"]["message"] == "fdict flag is not supported"


@pytest.mark.gpu
def test_facade_dictionary():
    d = dict_corpus.dictionary()
    msgs = dict_corpus.messages(6)
    big = b"".join(dict_corpus.records(9, 300))  # several blocks
    m0, m1 = msgs[0], msgs[1]
    co = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=d)
    raw_py = co.compress(m1) + co.flush()
    fd_py = fdict_stream(m1, d)
    wrong = bytes([d[0] ^ 1]) + d[1:]
    res = run_cases([
        {"id": "rd", "op": "rawDeflate", "in": m0.hex(), "dictionary": d.hex()},
        {"id": "rd_plain", "op": "rawDeflate", "in": m0.hex()},
        {"id": "rd_empty", "op": "rawDeflate", "in": m0.hex(), "dictionary": ""},
        {"id": "zd", "op": "deflate", "in": m0.hex(), "dictionary": d.hex()},
        {"id": "zd_big", "op": "deflate", "in": big.hex(), "dictionary": d.hex()},
        {"id": "zd_plain", "op": "deflate", "in": m0.hex()},
        {"id": "ri_py", "op": "rawInflate", "in": raw_py.hex(), "dictionary": d.hex()},
        {"id": "zi_py", "op": "inflate", "in": fd_py.hex(), "dictionary": d.hex(), "opts": {"verify": True}},
        {"id": "zi_wrong", "op": "inflate", "in": fd_py.hex(), "dictionary": wrong.hex()},
        {"id": "zi_none", "op": "inflate", "in": fd_py.hex()},
        {"id": "ri_none", "op": "rawInflate", "in": raw_py.hex()},
        {"id": "zi_nofdict", "op": "inflate", "in": zlib.compress(m1).hex(), "dictionary": d.hex()},
    ])
    for k in ("rd", "rd_plain", "rd_empty", "zd", "zd_big", "zd_plain", "ri_py", "zi_py", "zi_nofdict"):
        assert "error" not in res[k], res[k]
    # written by the facade, read by zlib
    rd = bytes.fromhex(res["rd"]["out"])
    assert zlib.decompressobj(-15, zdict=d).decompress(rd) == m0
    assert len(rd) < len(bytes.fromhex(res["rd_plain"]["out"]))
    assert res["rd_empty"]["out"] == res["rd_plain"]["out"]
    for k, m in (("zd", m0), ("zd_big", big)):
        z = bytes.fromhex(res[k]["out"])
        assert z[1] & 0x20 and z[2:6] == zlib.adler32(d).to_bytes(4, "big")
        assert zlib.decompressobj(zdict=d).decompress(z) == m
        assert res[k]["adler32"] == zlib.adler32(m)
    assert not bytes.fromhex(res["zd_plain"]["out"])[1] & 0x20
    # written by zlib, read by the facade
    assert bytes.fromhex(res["ri_py"]["out"]) == m1 and res["ri_py"]["ip"] == len(raw_py)
    assert bytes.fromhex(res["zi_py"]["out"]) == m1 and res["zi_py"]["ip"] == len(fd_py) - 4
    assert res["zi_py"]["adler32"] == zlib.adler32(m1)
    assert bytes.fromhex(res["zi_nofdict"]["out"]) == m1
    # errors
    assert res["zi_wrong"]["error"]["status"] == -44
    assert res["zi_wrong"]["error"]["message"] == "invalid dictionary id: 0x%x / 0x%x" % (zlib.adler32(d),
                                                                                          zlib.adler32(wrong))
    assert res["zi_none"]["error"]["message"] == "fdict flag is not supported"
    assert "error" in res["ri_none"]
    # the facade's own round trip
    back = run_cases([
        {"id": "a", "op": "rawInflate", "in": res["rd"]["out"], "dictionary": d.hex()},
        {"id": "b", "op": "inflate", "in": res["zd_big"]["out"], "dictionary": d.hex(), "opts": {"verify": True}}])
    assert bytes.fromhex(back["a"]["out"]) == m0
    assert bytes.fromhex(back["b"]["out"]) == big
