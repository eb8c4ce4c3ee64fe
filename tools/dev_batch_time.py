"""What the device-resident batch calls (include/zt_dev_batch.h) cost beside the
host calls of the same items, in one process and one run:
  * zt_inflate_dev_batch beside zt_inflate_raw_batch on tools/c2_bench.py's
    configuration (the 4096 distinct reference-deflated 64 KiB blocks of
    tests/c2_corpus.py), streams and outputs in device memory for the one and
    in host memory for the other,
  * zt_deflate_dev_batch (gzip) beside zt_gzip_compress_batch on a batch of
    mixed sizes (log-uniform 1 KiB - 1 MiB, "mixed" synthetic data, level 6).
Wall time of the C calls (pointer arrays built once; zt_free of the host
outputs after the clock, as c2_bench does), the calls interleaved round by
round so that drift hits them alike: medians, quartiles and every sample.  Then,
in rounds of their own (the event timing waits for every launch), the HIP-event
time of the gather and scatter launches alone (zt_debug_dev_batch_times) and
their share of the untimed call.  Outputs are checked once, outside the clock.
Writes profiles/dev_batch_time.json.
   usage: python tools/dev_batch_time.py [out.json] [rounds]"""
import ctypes
import json
import math
import os
import random
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "zlib.ts_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import c2_corpus  # noqa: E402
import ztamd as zt  # noqa: E402
import zt_oracle  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dev_batch_time.json")
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
WARM = 3
u8p, sz, vp = ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t, ctypes.c_void_p


def host_ptrs(items):
    bs = [bytes(x) for x in items]
    k = len(bs)
    return bs, (vp * k)(*[ctypes.cast(ctypes.c_char_p(x), vp).value for x in bs]), (sz * k)(*[len(x) for x in bs])


def dev_pack(items, align=1):
    """the items one after the other in one cuda tensor; (tensor, pointer array)"""
    offs, tot = [], 0
    for x in items:
        offs.append(tot)
        tot += (len(x) + align - 1) // align * align
    t = torch.frombuffer(bytearray(b"".join(bytes(x) + b"\0" * (-len(x) % align) for x in items)) or bytearray(1),
                         dtype=torch.uint8).cuda()
    return t, (vp * len(items))(*[t.data_ptr() + o for o in offs])


# ---- C2: inflate ---------------------------------------------------------------------
corpus = c2_corpus.build(zt_oracle.Oracle())
streams = [s for _, s, _ in corpus]
K = len(streams)
keep_h, h_ptrs, h_lens = host_ptrs(streams)
d_streams, d_ptrs = dev_pack(streams)  # back to back: arbitrary alignment
d_out = torch.empty(K * c2_corpus.BLOCK, dtype=torch.uint8, device="cuda")
d_optrs = (vp * K)(*[d_out.data_ptr() + i * c2_corpus.BLOCK for i in range(K)])
d_caps = (sz * K)(*[c2_corpus.BLOCK] * K)
iopts = zt.InflateOpts(1, 0x8000, 0)
state = {}


def inflate_host():
    outs, olens, ips, st = (u8p * K)(), (sz * K)(), (sz * K)(), (ctypes.c_int * K)()
    t0 = time.perf_counter()
    rc = zt.lib.zt_inflate_raw_batch(h_ptrs, h_lens, K, ctypes.byref(iopts), outs, olens, ips, st)
    dt = time.perf_counter() - t0
    assert rc == 0 and not any(st)
    for o in outs:
        zt.lib.zt_free(o)
    return dt


def inflate_dev():
    olens, ips, st = (sz * K)(), (sz * K)(), (ctypes.c_int * K)()
    t0 = time.perf_counter()
    rc = zt.lib.zt_inflate_dev_batch(d_ptrs, h_lens, None, K, d_optrs, d_caps, olens, ips, st, None, None, None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert rc == 0 and not any(st) and all(n == c2_corpus.BLOCK for n in olens)
    if "inflate_checked" not in state:
        state["inflate_checked"] = d_out.cpu().numpy().tobytes() == b"".join(raw for raw, _, _ in corpus)
    return dt


# ---- mixed sizes: gzip ----------------------------------------------------------------
rng = random.Random(11)
sizes = [int(math.exp(rng.uniform(math.log(1 << 10), math.log(1 << 20)))) for _ in range(384)]
total = sum(sizes)
g_src = torch.empty(total, dtype=torch.uint8, device="cuda")
zt.synth_dev("mixed", 7, g_src.data_ptr(), total)
g_host = g_src.cpu().numpy()
M = len(sizes)
offs = [sum(sizes[:i]) for i in range(M)]
g_hptrs = (vp * M)(*[g_host.ctypes.data + o for o in offs])
g_dptrs = (vp * M)(*[g_src.data_ptr() + o for o in offs])  # back to back
g_lens = (sz * M)(*sizes)
caps = [zt.deflate_dev_batch_bound(n, 2, "gzip") for n in sizes]
coffs = [sum(caps[:i]) for i in range(M)]
g_out = torch.empty(sum(caps), dtype=torch.uint8, device="cuda")
g_optrs = (vp * M)(*[g_out.data_ptr() + o for o in coffs])
g_caps = (sz * M)(*caps)
gopts = zt.GzipOpts()
gopts.deflate = zt.DeflateOpts(2, 0, 6)
dopts = zt.DeflateOpts(2, 0, 6)


def gzip_host():
    outs, olens, st = (u8p * M)(), (sz * M)(), (ctypes.c_int * M)()
    t0 = time.perf_counter()
    rc = zt.lib.zt_gzip_compress_batch(g_hptrs, g_lens, M, ctypes.byref(gopts), outs, olens, st)
    dt = time.perf_counter() - t0
    assert rc == 0
    if "members" not in state:
        state["members"] = [ctypes.string_at(outs[i], olens[i]) for i in range(M)]
    for o in outs:
        zt.lib.zt_free(o)
    return dt


def gzip_dev():
    olens, st = (sz * M)(), (ctypes.c_int * M)()
    t0 = time.perf_counter()
    rc = zt.lib.zt_deflate_dev_batch(g_dptrs, g_lens, M, ctypes.byref(dopts), 2, g_optrs, g_caps, olens, st, None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert rc == 0 and not any(st)
    if "gzip_checked" not in state and "members" in state:
        got = g_out.cpu().numpy().tobytes()
        state["gzip_checked"] = all(got[o:o + n] == m for o, n, m in zip(coffs, olens, state["members"]))
        state["gzip_bytes"] = sum(olens)
    return dt


calls = {"inflate_raw_batch_host": inflate_host, "inflate_dev_batch": inflate_dev,
         "gzip_compress_batch_host": gzip_host, "deflate_dev_batch_gzip": gzip_dev}
ts = {name: [] for name in calls}
for r in range(WARM + REPS):
    for name, fn in calls.items():
        dt = fn() * 1e3
        if r >= WARM:
            ts[name].append(dt)
assert state["inflate_checked"] and state["gzip_checked"]

# the gather and scatter launches alone, by HIP events, in rounds of their own
ev = {"inflate_dev_batch": {"gather": [], "scatter": []}, "deflate_dev_batch_gzip": {"gather": [], "scatter": []}}
zt.debug_dev_batch_times(True)
for r in range(WARM + REPS):
    for name in ev:
        calls[name]()
        g, s = zt.debug_dev_batch_times(True)
        if r >= WARM:
            ev[name]["gather"].append(g)
            ev[name]["scatter"].append(s)
zt.debug_dev_batch_times(False)


def row(v):
    q = statistics.quantiles(v, n=4)
    return {"ms_median": round(statistics.median(v), 3), "ms_q1": round(q[0], 3), "ms_q3": round(q[2], 3),
            "ms_iqr": round(q[2] - q[0], 3), "ms_all": [round(t, 3) for t in v]}


rows = {name: row(v) for name, v in ts.items()}
events = {name: {k: row(v) for k, v in d.items()} for name, d in ev.items()}
in_c2, out_c2 = sum(len(s) for s in streams), K * c2_corpus.BLOCK


def gibps(nbytes, name):
    return round(nbytes / (rows[name]["ms_median"] / 1e3) / 2**30, 2)


def share(name):
    return round((events[name]["gather"]["ms_median"] + events[name]["scatter"]["ms_median"])
                 / rows[name]["ms_median"], 4)


res = {
    "tool": "tools/dev_batch_time.py",
    "device": torch.cuda.get_device_name(0),
    "inflate_config": f"C2: {K} distinct reference-deflated 64 KiB blocks, {in_c2} -> {out_c2} bytes",
    "gzip_config": f"{M} items, log-uniform 1 KiB - 1 MiB, mixed synthetic data seed 7, {total} bytes, level 6 -> "
                   f"{state['gzip_bytes']} bytes of gzip members",
    "timed": f"wall of the C call (device calls: until the device is idle), median of {REPS} rounds after {WARM} "
             "warm-up rounds, the four calls interleaved round by round, one process; gather / scatter: HIP events "
             "around their launches in separate rounds",
    "rows": rows,
    "gather_scatter_events": events,
    "verdict": {
        "inflate_dev_over_host": round(rows["inflate_dev_batch"]["ms_median"] / rows["inflate_raw_batch_host"]["ms_median"], 3),
        "gzip_dev_over_host": round(rows["deflate_dev_batch_gzip"]["ms_median"] / rows["gzip_compress_batch_host"]["ms_median"], 3),
        "inflate_host_GiBps_out": gibps(out_c2, "inflate_raw_batch_host"),
        "inflate_dev_GiBps_out": gibps(out_c2, "inflate_dev_batch"),
        "gzip_host_GiBps_in": gibps(total, "gzip_compress_batch_host"),
        "gzip_dev_GiBps_in": gibps(total, "deflate_dev_batch_gzip"),
        "inflate_gather_scatter_share": share("inflate_dev_batch"),
        "gzip_gather_scatter_share": share("deflate_dev_batch_gzip"),
    },
}
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps({name: {f: v[f] for f in ("ms_median", "ms_q1", "ms_q3", "ms_iqr")} for name, v in rows.items()}, indent=1))
print(json.dumps({n: {k: v["ms_median"] for k, v in d.items()} for n, d in events.items()}))
print(json.dumps(res["verdict"]))
