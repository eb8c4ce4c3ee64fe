"""Child process of tests/test_gpu_host_batch.py::test_fewer_items_than_devices:
runs with ZT_ALIAS_DEVICES=3 (the library then presents three logical devices
on the one GPU), and for batches of fewer items than devices runs every batch
entry point on logical device 0 alone and again under zt_set_devices(0b111)
(host_batch.cpp for_each_device: the device count is clamped to the item
count).  Every output must equal the one-device output and decode with
Python's zlib.  Prints a JSON verdict.  Test infrastructure only."""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "zlib.ts_amd", "py"))
import ztamd as zt  # noqa: E402
import zt_oracle  # noqa: E402

o = zt_oracle.Oracle()
small, large = o.gen("wordsalad", 11, 1 << 10), o.gen("structured", 12, 70000)
dic = o.gen("wordsalad", 13, 4097)
cases = {"two": [small, large], "empty_and_one": [b"", large], "one_empty": [b""]}


def run(items):
    """every batch entry point's outputs for `items`, in a fixed order"""
    gz = zt.gzip_compress_batch(items, mtime=7)
    zl = zt.zlib_compress_batch(items)
    raw = zt.deflate_raw_batch(items)
    zl_d = zt.zlib_compress_batch(items, dictionary=dic)
    raw_d = zt.deflate_raw_batch(items, dictionary=dic)
    inf_d = zt.inflate_raw_batch(raw_d, dictionary=dic)
    gun = [(int(s), out) for s, out, _ in zt.gunzip_batch(gz)]
    unz = [(int(s), out, ip, adler) for s, out, ip, adler in zt.zlib_decompress_batch(zl, verify=True)]
    return {"gz": gz, "zl": zl, "raw": raw, "zl_d": zl_d, "raw_d": raw_d, "inf_d": inf_d, "gun": gun, "unz": unz}


def with_dict(stream, wbits):
    d = zlib.decompressobj(wbits, zdict=dic)
    return d.decompress(stream) + d.flush()


res = {"logical_devices": zt.device_count()}
for name, items in cases.items():
    single = run(items)
    zt.set_devices(0b111)
    try:
        split = run(items)
    finally:
        zt.set_devices(0)
    ok = True
    for i, f in enumerate(items):
        ok &= zlib.decompress(split["gz"][i], 31) == f
        ok &= zlib.decompress(split["zl"][i]) == f
        ok &= zlib.decompress(split["raw"][i], -15) == f
        ok &= with_dict(split["zl_d"][i], 15) == f
        ok &= with_dict(split["raw_d"][i], -15) == f
        ok &= split["inf_d"][i][:2] == (0, f)
        ok &= split["gun"][i] == (0, f)
        ok &= split["unz"][i][:2] == (0, f) and split["unz"][i][3] == zlib.adler32(f)
    res[name] = {"equal": [k for k in single if single[k] != split[k]] == [], "decodes": bool(ok)}
print(json.dumps(res), flush=True)
