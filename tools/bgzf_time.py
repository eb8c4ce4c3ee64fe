"""What BGZF costs beside the nearest calls a caller had before, in one run: a
mixed corpus (default 256 MiB) on the host, level 6, host to host, PCIe
included --
  * zt_bgzf_compress beside zt_gzip_compress_batch over the same 65280-byte
    slices (members in a slab, not a file: the nearest thing before),
  * zt_bgzf_decompress of the written file beside zt_gunzip_batch of the same
    file read as anonymous multi-member gzip,
  * zt_bgzf_read_ranges of 64 ranges of 4096 bytes spread over the file, with
    the .gzi and without one.
The calls are interleaved round by round so that drift hits them alike.  Each
row: the median of the timed rounds after warm-up, the quartiles and every
sample; a host clock around the synchronous C calls, zt_free of the outputs
included.  The outputs are checked once, outside the clock.  Writes
profiles/bgzf_time.json.
   usage: python tools/bgzf_time.py [size_bytes] [out.json] [rounds]"""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "bgzf_time.json")
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 15
WARM = 3
BS = zt.BGZF_BLOCK_MAX

d_in = torch.empty(n, dtype=torch.uint8, device="cuda")
zt.synth_dev("mixed", 7, d_in.data_ptr(), n)
data = d_in.cpu().numpy()
del d_in
base = data.ctypes.data
src = ctypes.c_void_p(base)
u8p = ctypes.POINTER(ctypes.c_uint8)
sz = ctypes.c_size_t
bopts = zt.BgzfOpts(zt.DeflateOpts(2, 0, 6), 0)
gopts = zt.GzipOpts()
gopts.deflate = zt.DeflateOpts(2, 0, 6)
k = (n + BS - 1) // BS
ptrs = (ctypes.c_void_p * k)(*[base + i * BS for i in range(k)])
lens = (sz * k)(*[min(BS, n - i * BS) for i in range(k)])
keep = {}


def bgzf_compress():
    out, olen, gzi, glen = u8p(), sz(), u8p(), sz()
    zt._check(zt.lib.zt_bgzf_compress(src, n, ctypes.byref(bopts), ctypes.byref(out), ctypes.byref(olen),
                                      ctypes.byref(gzi), ctypes.byref(glen)))
    if "file" not in keep:
        keep["file"] = ctypes.string_at(out, olen.value)
        keep["gzi"] = ctypes.string_at(gzi, glen.value)
    zt.lib.zt_free(out)
    zt.lib.zt_free(gzi)


def gzip_batch():
    outs, olens, st = (u8p * k)(), (sz * k)(), (ctypes.c_int * k)()
    zt._check(zt.lib.zt_gzip_compress_batch(ptrs, lens, k, ctypes.byref(gopts), outs, olens, st))
    keep["gzip_batch_bytes"] = sum(olens)
    for o in outs:
        zt.lib.zt_free(o)


def read_setup():
    f = keep["file"]
    keep["fbuf"] = ctypes.create_string_buffer(f, len(f))
    keep["gbuf"] = ctypes.create_string_buffer(keep["gzi"], len(keep["gzi"]))
    m = 64
    step = (n - 4096) // (m - 1)
    keep["ranges"] = [(i * step + 17 * i, 4096) for i in range(m)]
    keep["offs"] = (ctypes.c_uint64 * m)(*[r[0] for r in keep["ranges"]])
    keep["lens"] = (ctypes.c_uint64 * m)(*[r[1] for r in keep["ranges"]])


def bgzf_decompress():
    out, olen, info = u8p(), sz(), zt.BgzfInfo()
    zt._check(zt.lib.zt_bgzf_decompress(keep["fbuf"], len(keep["file"]), ctypes.byref(out), ctypes.byref(olen),
                                        ctypes.byref(info)))
    if "checked" not in keep:
        keep["checked"] = ctypes.string_at(out, olen.value) == data.tobytes()
    zt.lib.zt_free(out)


def gunzip_batch():
    fp = (ctypes.c_void_p * 1)(ctypes.addressof(keep["fbuf"]))
    fl = (sz * 1)(len(keep["file"]))
    outs, olens, st = (u8p * 1)(), (sz * 1)(), (ctypes.c_int * 1)()
    zt._check(zt.lib.zt_gunzip_batch(fp, fl, 1, outs, olens, None, None, st))
    keep["gunzip_batch_bytes"] = olens[0]
    zt.lib.zt_free(outs[0])


def ranges(with_gzi):
    m = len(keep["ranges"])
    outs, olens, st = (u8p * m)(), (sz * m)(), (ctypes.c_int * m)()
    zt._check(zt.lib.zt_bgzf_read_ranges(keep["fbuf"], len(keep["file"]), keep["gbuf"] if with_gzi else None,
                                         len(keep["gzi"]) if with_gzi else 0, keep["offs"], keep["lens"], m, outs,
                                         olens, st))
    if ("ranges_ok", with_gzi) not in keep:
        keep[("ranges_ok", with_gzi)] = all(
            ctypes.string_at(outs[i], olens[i]) == data[o:o + ln].tobytes() for i, (o, ln) in enumerate(keep["ranges"]))
    for o in outs:
        zt.lib.zt_free(o)


bgzf_compress()
read_setup()
calls = {"bgzf_compress": bgzf_compress, "gzip_compress_batch": gzip_batch, "bgzf_decompress": bgzf_decompress,
         "gunzip_batch": gunzip_batch, "bgzf_read_ranges_gzi": lambda: ranges(True),
         "bgzf_read_ranges_walk": lambda: ranges(False)}
ts = {name: [] for name in calls}
for r in range(WARM + REPS):
    for name, fn in calls.items():
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if r >= WARM:
            ts[name].append(dt)
assert keep["checked"] and keep[("ranges_ok", True)] and keep[("ranges_ok", False)]
assert keep["gunzip_batch_bytes"] == n


def row(v):
    q = statistics.quantiles(v, n=4)
    return {"ms_median": round(statistics.median(v), 3), "ms_q1": round(q[0], 3), "ms_q3": round(q[2], 3),
            "ms_iqr": round(q[2] - q[0], 3), "ms_all": [round(t, 3) for t in v]}


rows = {name: row(v) for name, v in ts.items()}
stats = zt.bgzf_stats()
res = {
    "tool": "tools/bgzf_time.py",
    "device": torch.cuda.get_device_name(0),
    "corpus": f"mixed, seed 7, {n} bytes, level 6 -> {len(keep['file'])} bytes of BGZF in {k} blocks "
              f"(gzip batch members: {keep['gzip_batch_bytes']} bytes)",
    "timed": f"wall, whole C call incl. zt_free of the outputs, host to host, median of {REPS} rounds after {WARM} "
             "warm-up rounds, the calls interleaved round by round, one process",
    "ranges": f"{len(keep['ranges'])} ranges of 4096 bytes spread over the file",
    "rows": rows,
    "verdict": {
        "compress_over_gzip_batch": round(rows["bgzf_compress"]["ms_median"] / rows["gzip_compress_batch"]["ms_median"], 3),
        "decompress_over_gunzip_batch": round(rows["bgzf_decompress"]["ms_median"] / rows["gunzip_batch"]["ms_median"], 3),
        "ranges_gzi_over_decompress": round(rows["bgzf_read_ranges_gzi"]["ms_median"] / rows["bgzf_decompress"]["ms_median"], 4),
        "blocks_decoded_per_range_call": stats["blocks_decoded"] / max(1, stats["range_calls"]),
    },
}
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps({name: {f: v[f] for f in ("ms_median", "ms_q1", "ms_q3", "ms_iqr")} for name, v in rows.items()}, indent=1))
print(json.dumps(res["verdict"]))
