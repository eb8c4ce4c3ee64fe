"""What the deflate-time index costs, in one run: a mixed corpus (default
256 MiB) on the host, level 6, host to host, PCIe included --
  * zt_deflate_raw (plain),
  * zt_deflate_raw_indexed,
  * zt_deflate_raw followed by zt_inflate_index_build of its stream (the only
    way to an index before).
The three are interleaved round by round (plain, indexed, plain + build, ...)
so that drift hits them alike.  Each row: the median of the timed rounds after
warm-up, a host clock around the synchronous C calls (zt_free of the outputs
included), and for the plain call its interquartile range: the run-to-run
spread the indexed call is held against (gate: indexed median <= plain median
+ plain IQR).  The blob is compared with the build's once, outside the clock.
Writes profiles/deflate_index_time.json.
   usage: python tools/deflate_index_time.py [size_bytes] [out.json] [rounds]"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "zlib.ts_amd", "py"))
import torch  # noqa: E402
import ztamd as zt  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256 << 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "deflate_index_time.json")
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 15
WARM = 3

d_in = torch.empty(n, dtype=torch.uint8, device="cuda")
zt.synth_dev("mixed", 7, d_in.data_ptr(), n)
data = d_in.cpu().numpy()
del d_in
src = data.ctypes.data_as(ctypes.c_void_p)
u8p = ctypes.POINTER(ctypes.c_uint8)
opts = zt.DeflateOpts(2, 0, 6)
keep = {}


def plain(free=True):
    out, olen = u8p(), ctypes.c_size_t()
    zt._check(zt.lib.zt_deflate_raw(src, n, ctypes.byref(opts), ctypes.byref(out), ctypes.byref(olen)))
    keep["clen"] = olen.value
    if free:
        zt.lib.zt_free(out)
    return out, olen.value


def indexed():
    out, olen, idx, ilen = u8p(), ctypes.c_size_t(), u8p(), ctypes.c_size_t()
    zt._check(zt.lib.zt_deflate_raw_indexed(src, n, ctypes.byref(opts), 0, ctypes.byref(out), ctypes.byref(olen),
                                            ctypes.byref(idx), ctypes.byref(ilen)))
    if "blob" not in keep:
        keep["blob"] = ctypes.string_at(idx, ilen.value)
        keep["stream"] = ctypes.string_at(out, olen.value)
    zt.lib.zt_free(out)
    zt.lib.zt_free(idx)


def plain_then_build():
    out, clen = plain(free=False)
    idx, ilen, blen = u8p(), ctypes.c_size_t(), ctypes.c_size_t()
    zt._check(zt.lib.zt_inflate_index_build(out, clen, 0, ctypes.byref(idx), ctypes.byref(ilen), None,
                                            ctypes.byref(blen), None))
    if "built" not in keep:
        keep["built"] = ctypes.string_at(idx, ilen.value)
    zt.lib.zt_free(idx)
    zt.lib.zt_free(out)


calls = {"deflate_raw": plain, "deflate_raw_indexed": indexed, "deflate_raw_then_index_build": plain_then_build}
ts = {k: [] for k in calls}
for r in range(WARM + REPS):
    for name, fn in calls.items():
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if r >= WARM:
            ts[name].append(dt)
assert keep["blob"] == keep["built"], "the deflate-time index differs from the build's"
assert len(keep["stream"]) == keep["clen"]


def row(v):
    q = statistics.quantiles(v, n=4)
    return {"ms_median": round(statistics.median(v), 3), "ms_q1": round(q[0], 3), "ms_q3": round(q[2], 3),
            "ms_iqr": round(q[2] - q[0], 3), "ms_all": [round(t, 3) for t in v]}


rows = {k: row(v) for k, v in ts.items()}
p, x, b = rows["deflate_raw"], rows["deflate_raw_indexed"], rows["deflate_raw_then_index_build"]
hdr, _ = zt.index_entries(keep["blob"])
res = {
    "tool": "tools/deflate_index_time.py",
    "device": torch.cuda.get_device_name(0),
    "corpus": f"mixed, seed 7, {n} bytes, level 6 -> {keep['clen']} bytes",
    "timed": f"wall, whole C call(s) incl. zt_free of the outputs, host to host, median of {REPS} rounds after {WARM} "
             "warm-up rounds, the three calls interleaved round by round, one process",
    "index": {"units": hdr["nunits"], "segments": hdr["nseg"], "blob_bytes": len(keep["blob"]),
              "equals_index_build": True},
    "rows": rows,
    "verdict": {
        "indexed_minus_plain_ms": round(x["ms_median"] - p["ms_median"], 3),
        "plain_iqr_ms": p["ms_iqr"],
        "gate_indexed_within_plain_plus_iqr": x["ms_median"] <= p["ms_median"] + p["ms_iqr"],
        "build_minus_plain_ms": round(b["ms_median"] - p["ms_median"], 3),
    },
}
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps({k: {f: v[f] for f in ("ms_median", "ms_q1", "ms_q3", "ms_iqr")} for k, v in rows.items()}, indent=1))
print(json.dumps(res["verdict"]))
