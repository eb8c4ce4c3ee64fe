"""Child process of tests/test_gpu_dict.py::test_alias_devices_dict: runs with
ZT_ALIAS_DEVICES=2 (two logical devices on the one GPU, each with its own
context and its own copy of the dictionary), runs a dictionary batch of 256
records on logical device 0 alone and again split over both by
zt_set_devices, and prints a JSON verdict.  Test infrastructure only."""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "zlib.ts_amd", "py"))
import dict_corpus  # noqa: E402
import ztamd as zt  # noqa: E402

ndev = zt.device_count()
d = dict_corpus.dictionary()
msgs = dict_corpus.messages(256)
res = {"logical_devices": ndev}
one_raw = zt.deflate_raw_batch(msgs, dictionary=d)
one_zl = zt.zlib_compress_batch(msgs, dictionary=d)
one_inf = zt.inflate_raw_batch(one_raw, dictionary=d)
zt.set_devices((1 << ndev) - 1)
try:
    two_raw = zt.deflate_raw_batch(msgs, dictionary=d)
    two_zl = zt.zlib_compress_batch(msgs, dictionary=d)
    two_inf = zt.inflate_raw_batch(one_raw, dictionary=d)
finally:
    zt.set_devices(0)
res["deflate_equal"] = two_raw == one_raw
res["zlib_equal"] = two_zl == one_zl
res["inflate_equal"] = two_inf == one_inf and [o for _, o, _ in two_inf] == msgs
ok = True
for m, s, z in zip(msgs, two_raw, two_zl):
    ok &= zlib.decompressobj(-15, zdict=d).decompress(s) == m
    ok &= zlib.decompressobj(zdict=d).decompress(z) == m
res["zlib_ok"] = bool(ok)
print(json.dumps(res), flush=True)
