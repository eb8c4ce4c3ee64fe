"""Indexed random access against the whole-stream call, in one run: a mixed
corpus (default 256 MiB) deflated at level 6 on the device, then on the host
stream, PCIe included --
  * zt_inflate_raw of the whole stream (the only way to read a range without
    an index),
  * zt_inflate_index_build with and without the decoded output,
  * zt_inflate_range of 64 KiB and of 1 MiB at 200 seeded offsets (median and
    worst of the calls),
  * zt_inflate_ranges of 1024 x 64 KiB (ms, GiB/s of returned bytes),
  * the index blob's size per GiB of output.
Each row: the median of repeated runs after warm-up, a host clock around the
synchronous C calls (zt_free of the outputs included).  Writes
profiles/index_range_time.json.
   usage: python tools/index_time.py [size_bytes] [out.json]"""
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "zlib.ts_amd", "py"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ztamd as zt  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256 << 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "index_range_time.json")
REPS, WARM = 5, 2

d_in = torch.empty(n, dtype=torch.uint8, device="cuda")
zt.synth_dev("mixed", 7, d_in.data_ptr(), n)
d_c = torch.empty(zt.deflate_bound(n), dtype=torch.uint8, device="cuda")
dp = zt.DeflatePlan(n, level=6)
clen = dp.run(d_in.data_ptr(), n, d_c.data_ptr())
dp.close()
data = d_in.cpu().numpy()
stream = d_c[:clen].cpu().numpy()
del d_in, d_c
src = stream.ctypes.data_as(ctypes.c_void_p)
u8p = ctypes.POINTER(ctypes.c_uint8)


def timed(fn, reps=REPS, warm=WARM):
    ts = []
    for r in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if r >= warm:
            ts.append(dt)
    return {"ms_median": round(statistics.median(ts), 3), "ms_all": [round(t, 3) for t in ts]}


def whole():
    back, blen, ip = u8p(), ctypes.c_size_t(), ctypes.c_size_t()
    zt._check(zt.lib.zt_inflate_raw(src, clen, 0, None, ctypes.byref(back), ctypes.byref(blen), ctypes.byref(ip)))
    assert blen.value == n and ip.value == clen
    zt.lib.zt_free(back)


blob_keep = {}


def build(want_output):
    def run():
        idx, ilen = u8p(), ctypes.c_size_t()
        back, blen, ip = u8p(), ctypes.c_size_t(), ctypes.c_size_t()
        zt._check(zt.lib.zt_inflate_index_build(src, clen, 0, ctypes.byref(idx), ctypes.byref(ilen),
                                                ctypes.byref(back) if want_output else None, ctypes.byref(blen),
                                                ctypes.byref(ip)))
        assert blen.value == n and ip.value == clen
        blob_keep["blob"] = ctypes.string_at(idx, ilen.value)
        zt.lib.zt_free(idx)
        if want_output:
            zt.lib.zt_free(back)
    return run


rows = {"inflate_raw_whole": timed(whole)}
rows["inflate_raw_whole"]["GiB_per_s"] = round(n / rows["inflate_raw_whole"]["ms_median"] * 1e3 / 2**30, 3)
rows["index_build_with_output"] = timed(build(True))
rows["index_build_index_only"] = timed(build(False))
blob = blob_keep["blob"]
ib = ctypes.create_string_buffer(blob, len(blob))
hdr, ent = zt.index_entries(blob)
assert hdr["total_out"] == n


def one_range(off, length):
    back, blen = u8p(), ctypes.c_size_t()
    t0 = time.perf_counter()
    zt._check(zt.lib.zt_inflate_range(src, clen, ib, len(blob), off, length, ctypes.byref(back), ctypes.byref(blen)))
    ok = blen.value == length and np.array_equal(np.ctypeslib.as_array(back, shape=(length,)), data[off:off + length])
    zt.lib.zt_free(back)
    dt = (time.perf_counter() - t0) * 1e3  # (the comparison is inside the clock: microseconds for 64 KiB and 1 MiB)
    assert ok, (off, length)
    return dt


for name, length in (("range_64KiB", 64 << 10), ("range_1MiB", 1 << 20)):
    rnd = random.Random(length)
    offs = [rnd.randrange(n - length) for _ in range(200)]
    for o in offs[:8]:
        one_range(o, length)  # warm-up
    ts = [one_range(o, length) for o in offs]
    rows[name] = {"calls": len(ts), "ms_median": round(statistics.median(ts), 3), "ms_worst": round(max(ts), 3),
                  "ms_best": round(min(ts), 3)}

ts = [one_range(0, n) for _ in range(WARM + REPS)][WARM:]  # the whole output through the range call (its comparison with the corpus is inside the clock)
rows["range_whole_output_checked"] = {"ms_median": round(statistics.median(ts), 3), "ms_all": [round(t, 3) for t in ts]}

rnd = random.Random(1024)
k = 1024
offs = (ctypes.c_uint64 * k)(*[rnd.randrange(n - (64 << 10)) for _ in range(k)])
lens = (ctypes.c_uint64 * k)(*([64 << 10] * k))


def many():
    outs, olens, st = (u8p * k)(), (ctypes.c_size_t * k)(), (ctypes.c_int * k)()
    zt._check(zt.lib.zt_inflate_ranges(src, clen, ib, len(blob), offs, lens, k, outs, olens, st))
    if not checked:  # once, outside the timed runs: every range against the corpus
        for i in range(k):
            assert ctypes.string_at(outs[i], olens[i]) == data[offs[i]:offs[i] + lens[i]].tobytes(), i
        checked.append(True)
    for i in range(k):
        zt.lib.zt_free(outs[i])


checked = []
many()
zt.index_stats(reset=True)
rows["ranges_1024x64KiB"] = timed(many)
st = zt.index_stats()
rows["ranges_1024x64KiB"]["GiB_per_s_returned"] = round(k * (64 << 10) / rows["ranges_1024x64KiB"]["ms_median"] * 1e3
                                                        / 2**30, 3)
rows["ranges_1024x64KiB"]["stats_per_call"] = {f: v // (REPS + WARM) for f, v in st.items() if f != "builds"}

res = {
    "tool": "tools/index_time.py",
    "device": torch.cuda.get_device_name(0),
    "corpus": f"mixed, seed 7, {n} bytes, level 6 -> {clen} bytes",
    "timed": f"wall, whole C call(s) incl. zt_free of the outputs, median of {REPS} after {WARM} warm-up rounds "
             "(single ranges: one call per offset, 200 seeded offsets after 8 warm-up calls), one process",
    "index": {"units": hdr["nunits"], "segments": hdr["nseg"], "blob_bytes": len(blob),
              "blob_bytes_per_GiB_of_output": round(len(blob) / n * 2**30)},
    "rows": rows,
    "verdict": {
        "range_64KiB_over_whole": round(rows["inflate_raw_whole"]["ms_median"] / rows["range_64KiB"]["ms_median"], 2),
        "range_64KiB_below_whole": rows["range_64KiB"]["ms_worst"] < rows["inflate_raw_whole"]["ms_median"],
    },
}
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res["rows"], indent=1))
print(json.dumps(res["verdict"]))
