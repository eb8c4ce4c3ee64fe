"""Checkpoint random access against the whole-stream call, in one run, on two
streams without sync points made on the CPU:
  * a mixed corpus (default 256 MiB) deflated by Python's zlib at level 6,
  * a mixed corpus (default 64 MiB) as the reference's RawDeflate writes it
    (the test oracle: one dynamic block for the whole input).
Per stream, on the host stream, PCIe included --
  * zt_inflate_raw of the whole stream (the only way to read a range without
    a blob), median and interquartile range,
  * zt_inflate_ckpt_build with and without the decoded output,
  * zt_inflate_ckpt_range of 64 KiB at 200 seeded offsets (median and worst),
  * zt_inflate_ckpt_ranges of 1024 x 64 KiB (ms, GiB/s of returned bytes),
  * the blob's size per GiB of output.
Each row: repeated runs after warm-up, a host clock around the synchronous C
calls (zt_free of the outputs included).  The one condition: the single-range
median lies below the whole-stream median by more than that decode's
interquartile range.  Writes profiles/checkpoint_range_time.json.
   usage: python tools/checkpoint_range_time.py [zlib_bytes] [reference_bytes] [out.json]"""
import ctypes
import json
import os
import random
import statistics
import sys
import time
import zlib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "zlib.ts_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import zt_oracle  # noqa: E402
import ztamd as zt  # noqa: E402

n_zlib = int(sys.argv[1]) if len(sys.argv) > 1 else 256 << 20
n_ref = int(sys.argv[2]) if len(sys.argv) > 2 else 64 << 20
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "checkpoint_range_time.json")
REPS, WARM = 7, 2
RANGE = 64 << 10
u8p = ctypes.POINTER(ctypes.c_uint8)


def corpus(n, seed):
    d = torch.empty(n, dtype=torch.uint8, device="cuda")
    zt.synth_dev("mixed", seed, d.data_ptr(), n)
    return d.cpu().numpy()


def timed(fn, reps=REPS, warm=WARM):
    ts = []
    for r in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if r >= warm:
            ts.append(dt)
    q = statistics.quantiles(ts, n=4)
    return {"ms_median": round(statistics.median(ts), 3), "ms_iqr": round(q[2] - q[0], 3),
            "ms_all": [round(t, 3) for t in ts]}


def measure(data, stream, how):
    n, clen = len(data), len(stream)
    sbuf = np.frombuffer(stream, dtype=np.uint8)
    src = sbuf.ctypes.data_as(ctypes.c_void_p)

    def whole():
        back, blen, ip = u8p(), ctypes.c_size_t(), ctypes.c_size_t()
        zt._check(zt.lib.zt_inflate_raw(src, clen, 0, None, ctypes.byref(back), ctypes.byref(blen), ctypes.byref(ip)))
        assert blen.value == n and ip.value == clen
        zt.lib.zt_free(back)

    keep = {}

    def build(want_output):
        def run():
            idx, ilen = u8p(), ctypes.c_size_t()
            back, blen, ip = u8p(), ctypes.c_size_t(), ctypes.c_size_t()
            zt._check(zt.lib.zt_inflate_ckpt_build(src, clen, 0, 0, ctypes.byref(idx), ctypes.byref(ilen),
                                                   ctypes.byref(back) if want_output else None, ctypes.byref(blen),
                                                   ctypes.byref(ip)))
            assert blen.value == n and ip.value == clen
            keep["blob"] = ctypes.string_at(idx, ilen.value)
            zt.lib.zt_free(idx)
            if want_output:
                zt.lib.zt_free(back)
        return run

    rows = {"inflate_raw_whole": timed(whole)}
    rows["inflate_raw_whole"]["GiB_per_s"] = round(n / rows["inflate_raw_whole"]["ms_median"] * 1e3 / 2**30, 3)
    rows["ckpt_build_with_output"] = timed(build(True), reps=3, warm=1)
    rows["ckpt_build_blob_only"] = timed(build(False), reps=3, warm=1)
    blob = keep["blob"]
    ib = ctypes.create_string_buffer(blob, len(blob))
    hdr, ent, wins = zt.ckpt_entries(blob)
    assert hdr["total_out"] == n

    def one_range(off, length):
        back, blen = u8p(), ctypes.c_size_t()
        t0 = time.perf_counter()
        zt._check(zt.lib.zt_inflate_ckpt_range(src, clen, ib, len(blob), off, length, ctypes.byref(back),
                                               ctypes.byref(blen)))
        ok = blen.value == length and np.array_equal(np.ctypeslib.as_array(back, shape=(length,)),
                                                     data[off:off + length])
        zt.lib.zt_free(back)
        dt = (time.perf_counter() - t0) * 1e3  # (the comparison is inside the clock: microseconds for 64 KiB)
        assert ok, (off, length)
        return dt

    rnd = random.Random(RANGE)
    offs = [rnd.randrange(n - RANGE) for _ in range(200)]
    for o in offs[:8]:
        one_range(o, RANGE)  # warm-up
    zt.ckpt_stats(reset=True)
    ts = [one_range(o, RANGE) for o in offs]
    st = zt.ckpt_stats()
    rows["range_64KiB"] = {"calls": len(ts), "ms_median": round(statistics.median(ts), 3),
                           "ms_worst": round(max(ts), 3), "ms_best": round(min(ts), 3),
                           "stats_per_call": {f: v // len(ts) for f, v in st.items() if f != "builds"}}

    rnd = random.Random(1024)
    k = 1024
    offs_k = (ctypes.c_uint64 * k)(*[rnd.randrange(n - RANGE) for _ in range(k)])
    lens_k = (ctypes.c_uint64 * k)(*([RANGE] * k))
    checked = []

    def many():
        outs, olens, sts = (u8p * k)(), (ctypes.c_size_t * k)(), (ctypes.c_int * k)()
        zt._check(zt.lib.zt_inflate_ckpt_ranges(src, clen, ib, len(blob), offs_k, lens_k, k, outs, olens, sts))
        if not checked:  # once, outside the timed runs: every range against the corpus
            for i in range(k):
                assert ctypes.string_at(outs[i], olens[i]) == data[offs_k[i]:offs_k[i] + lens_k[i]].tobytes(), i
            checked.append(True)
        for i in range(k):
            zt.lib.zt_free(outs[i])

    many()
    zt.ckpt_stats(reset=True)
    rows["ranges_1024x64KiB"] = timed(many, reps=5, warm=1)
    st = zt.ckpt_stats()
    rows["ranges_1024x64KiB"]["GiB_per_s_returned"] = round(k * RANGE / rows["ranges_1024x64KiB"]["ms_median"] * 1e3
                                                            / 2**30, 3)
    rows["ranges_1024x64KiB"]["stats_per_call"] = {f: v // 6 for f, v in st.items() if f != "builds"}
    w = rows["inflate_raw_whole"]
    return {
        "stream": f"{how}: {n} bytes -> {clen} bytes",
        "blob": {"units": hdr["nunits"], "windows": hdr["nwin"], "span": hdr["span"], "blob_bytes": len(blob),
                 "blob_bytes_per_GiB_of_output": round(len(blob) / n * 2**30),
                 "blob_share_of_output": round(len(blob) / n, 5)},
        "rows": rows,
        "verdict": {
            "range_64KiB_over_whole": round(w["ms_median"] / rows["range_64KiB"]["ms_median"], 2),
            "range_64KiB_median_below_whole_by_more_than_its_iqr":
                rows["range_64KiB"]["ms_median"] < w["ms_median"] - w["ms_iqr"],
        },
    }


streams = {}
data = corpus(n_zlib, 7)
t0 = time.perf_counter()
co = zlib.compressobj(6, zlib.DEFLATED, -15)
s = co.compress(data.tobytes()) + co.flush()
print(f"zlib level 6: {time.perf_counter() - t0:.1f} s on the CPU", flush=True)
streams["zlib6"] = measure(data, s, "mixed, seed 7, Python zlib level 6, wbits -15")
print(json.dumps(streams["zlib6"]["verdict"]), flush=True)
data = corpus(n_ref, 9)
t0 = time.perf_counter()
s = zt_oracle.Oracle().raw_deflate(data.tobytes())[0]
print(f"reference RawDeflate: {time.perf_counter() - t0:.1f} s on the CPU", flush=True)
streams["reference"] = measure(data, s, "mixed, seed 9, the reference's RawDeflate (test oracle), one dynamic block")
print(json.dumps(streams["reference"]["verdict"]), flush=True)

res = {
    "tool": "tools/checkpoint_range_time.py",
    "device": torch.cuda.get_device_name(0),
    "timed": f"wall, whole C call(s) incl. zt_free of the outputs, median and interquartile range of {REPS} after {WARM} "
             "warm-up rounds (builds: 3 after 1; the 1024-range call: 5 after 1; single ranges: one call per offset, "
             "200 seeded offsets after 8 warm-up calls), one process",
    "streams": streams,
}
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res["streams"], indent=1))
