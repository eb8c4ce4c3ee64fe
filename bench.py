#!/usr/bin/env python3
"""bench.py -- the headline metric of BASELINE.json on MI355X:

    "GiB/s RawDeflate L6 + RawInflate on 1 GiB buffer; ratio vs ref"

One step = RawDeflate (level 6) of a 1 GiB device-resident synthetic buffer
followed by RawInflate of the resulting stream back into HBM, both through
libzt's device entry points (zt_deflate_dev / zt_inflate_dev, include/zt.h).
The corpus is SURVEY.md 8(d)'s mixed generator set (wordsalad, xorshift32,
structured int32 deltas, cycling per 4 MiB window), generated on the device.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--size BYTES] [--level L]
                  [--mode weak|c3] [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times the K steps, checks the last step's
round trip and prints the result line.  `--full` adds every leg beside the
headline (below).  `--dump-outputs DIR` writes what the last timed step
returned (stream length and bytes, inflated length and bytes; a fixed seeded
sample of the large arrays) as DIR/<name>.npy; the corpus is seeded, so two
runs with the same arguments dump the outputs of identical inputs.

Processes: one per GPU.  Under torch.distributed.run (WORLD_SIZE set) every
process is one rank.  `--gpus N` without a launcher makes this process a
plain launcher: it starts N rank processes of itself (subprocess, before any
GPU call here) with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, and exits
with their worst status.  Rank r uses device r % device_count (so N ranks can
be rehearsed on a one-GPU box).  Ranks meet over gloo (host TCP): the data
path has no collective at all; gloo carries the barriers
around the timed region, the max-over-ranks of the elapsed time, and the
sums for the ratio.

Modes:
  weak  (default) every rank round-trips its own `--size` buffer (1 GiB):
        value = total bytes of all ranks / max elapsed, "scaling": "weak".
  c3    config C3: ONE `--size` buffer (default 8 GiB) split by
        zt_shard.shard_range into segment-aligned shards, one per rank, each
        generated in place (zt_synth_dev_at), deflated with final only on the
        last rank; the shards' streams concatenate into one valid stream.  A
        step is the deflate of the whole buffer; value = buffer bytes / max
        elapsed, "scaling": "strong".  Each rank checks its shard by inflating
        its stream (closed by an empty final block when not last) on device.

Extra fields: `roofline` for the dominant kernel (deflate's match_kernel,
the LZ77 match finder; algorithmic bytes = N input bytes per launch, SURVEY.md
8(d), timed with HIP events on its launch stream, inside the timed steps);
with `--full` also the round-trip check before the warm-up (a plain weak-mode
run checks the last timed step's output instead), `cpu_baseline` (the oracle
-- the C restatement of the reference's RawDeflate + RawInflate -- on a
bounded sample on 16 threads, one-core figure beside it, rank 0, N = 1
only), the per-generator compression ratio of
this build against the reference on that sample, `api` -- the same round
trip through the host-buffer entry points (zt_deflate_raw / zt_inflate_raw),
PCIe transfers included -- `api_node` -- that round trip from Node through
the JS facade and the N-API addon, the boundary north_star names -- and
`per_generator` -- deflate / inflate rates of each generator alone, the
source-text sample included (all rank 0, N = 1, weak mode only; none of
them inside the timed region).
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "zlib.ts_amd", "py"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md
WINDOW = 4 << 20
KINDS = ["wordsalad", "xorshift32", "structured"]  # mixed corpus order per 4 MiB window
METRIC = "GiB/s RawDeflate L6 + RawInflate on 1 GiB buffer; ratio vs ref"


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, default=None, help="bytes (default 1 GiB; 8 GiB in c3 mode)")
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--mode", choices=["weak", "c3"], default="weak")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beside the headline: the untimed round-trip check before the warm-up, "
                         "cpu_baseline / ratio_vs_ref, api, api_node, per_generator (rank 0, --gpus 1, weak mode)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last step returned as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-api", action="store_true",
                    help="with --full: skip the host-buffer (PCIe-inclusive) round trip")
    ap.add_argument("--no-node", action="store_true", help="with --full: skip the Node (N-API facade) round trip")
    ap.add_argument("--no-per-generator", action="store_true", help="with --full: skip the per-generator rates")
    a = ap.parse_args(argv)
    if a.size is None:
        a.size = (8 << 30) if a.mode == "c3" else (1 << 30)
    return a


# ---------------------------------------------------------------- launcher
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(nproc):
    """Start `nproc` rank processes of this script and wait for them.  Runs
    before anything in this process touches the GPU."""
    port = str(_free_port())
    procs = []
    for r in range(nproc):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(nproc), LOCAL_WORLD_SIZE=str(nproc),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    for p in procs:
        rc = max(rc, p.wait())
    return rc


# ---------------------------------------------------------------- helpers
# the translation unit of the kernel the roofline reports (match_kernel) and
# the headers it includes: a PMC measurement stays tied to that kernel's code
DIGEST_SOURCES = ["deflate.hip", "zt_internal.h", "../../include/zt.h"]


def source_digest():
    """sha256 of the match kernel's sources (DIGEST_SOURCES under
    zlib.ts_amd/csrc): ties a PMC traffic measurement to the kernel it was
    taken on (edits to the inflate or checksum kernels leave it valid)."""
    h = hashlib.sha256()
    d = os.path.join(HERE, "zlib.ts_amd", "csrc")
    for f in DIGEST_SOURCES:
        with open(os.path.join(d, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()


def pmc_traffic(kernel, n):
    """HBM bytes per launch of `kernel` from profiles/pmc_traffic.json
    (tools/pmc_traffic.py over rocprofv3 FETCH_SIZE / WRITE_SIZE passes of
    this workload), or None when the file was measured on other kernel
    sources or another size: a stale measurement is never reported."""
    path = os.path.join(HERE, "profiles", "pmc_traffic.json")
    try:
        with open(path) as f:
            d = json.load(f)
        k = d["kernels"][kernel]
    except (OSError, KeyError, ValueError):
        return None
    if n != 1 << 30 or d.get("source_sha256") != source_digest():
        return None
    return int(k["traffic_bytes"])


def pmc_lds(kernel, n):
    """Where the kernel's cycles go beside HBM (SURVEY 8(d) honesty note: LZ77
    match finding is bound on chip, not by HBM): the LDS array's busy fraction
    of the kernel's CU-cycles and the bank-conflict share of those cycles,
    and the SIMDs' VALU busy fraction, per launch, from profiles/pmc_lds.json
    (tools/pmc_lds.py over a rocprofv3 SQ pass of this workload) -- or None
    when it was measured on other kernel sources."""
    path = os.path.join(HERE, "profiles", "pmc_lds.json")
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        return None
    if d.get("kernel") != kernel or n != 1 << 30 or d.get("source_sha256") != source_digest():
        return None
    out = {"busy_frac": d["busy_frac"], "bank_conflict_frac": d["bank_conflict_frac"]}
    if d.get("valu_busy_frac") is not None:
        out["valu_busy_frac"] = d["valu_busy_frac"]
        out["wave_parked_frac"] = d.get("wave_parked_frac")
    out["source"] = "profiles/pmc_lds.json"
    return out


def host_info():
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return os.cpu_count(), model


def cpu_baseline(d_in, level, zt):
    """Oracle (C restatement of src/RawDeflate.ts + src/RawInflate.ts) on the
    first three 4 MiB windows of the bench corpus, on one core and on the
    box's CPU share (16 threads); also the ratio of
    this build's deflate to the reference's bytes per generator."""
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import zt_oracle

    o = zt_oracle.Oracle()
    t_total = 0.0
    nbytes = 0
    ratios = {}
    for w, kind in enumerate(KINDS):
        chunk = bytes(d_in[w * WINDOW:(w + 1) * WINDOW].cpu().numpy())
        t0 = time.perf_counter()
        ref, _ = o.raw_deflate(chunk)
        back, _ = o.raw_inflate(ref)
        t_total += time.perf_counter() - t0
        assert back == chunk
        nbytes += len(chunk)
        ours = zt.deflate_raw(chunk, level=level)
        ratios[kind] = round(len(ours) / len(ref), 4)
    nproc, model = host_info()
    # the same sample on T threads at once (ctypes releases the GIL for the
    # oracle's C calls; its lazily built tables were filled by the pass
    # above): the host's rate, not one core's.  T defaults to 16 -- the CPU
    # share of one GPU on the benchmark box, whose os.cpu_count() reports the
    # whole machine (ZT_CPU_BASELINE_THREADS overrides)
    nthreads = int(os.environ.get("ZT_CPU_BASELINE_THREADS", min(16, nproc or 1)))
    chunks = [bytes(d_in[w * WINDOW:(w + 1) * WINDOW].cpu().numpy()) for w in range(len(KINDS))]

    def one_thread(_):
        for chunk in chunks:
            ref, _ = o.raw_deflate(chunk)
            back, _ = o.raw_inflate(ref)
            assert back == chunk
        return sum(len(c) for c in chunks)

    from concurrent.futures import ThreadPoolExecutor
    t0 = time.perf_counter()
    with ThreadPoolExecutor(nthreads) as ex:
        mt_bytes = sum(ex.map(one_thread, range(nthreads)))
    t_mt = time.perf_counter() - t0
    return {
        "value": round(mt_bytes / t_mt / 2**30, 5),
        "unit": "GiB/s",
        "cores": nthreads,
        "kind": "port",
        "sample": f"RawDeflate (reference defaults) + RawInflate of the first 3 x 4 MiB windows of the corpus "
                  f"(wordsalad, xorshift32, structured), oracle/liboracle.so, on {nthreads} threads at once "
                  f"(each thread the whole sample)",
        "single_thread_value": round(nbytes / t_total / 2**30, 5),
        "host_nproc": nproc,
        "host_cpu_model": model,
    }, ratios


def api_roundtrip(d_in, n, level, zt):
    """The round trip through the host-buffer entry points (what a Node
    caller of RawDeflate / RawInflate runs): zt_deflate_raw of a host copy of
    the corpus, then zt_inflate_raw of the host stream, each C call timed
    after one warm-up call of its own (PCIe transfers included; the outputs
    come from the library's host output pool, which the warm-up's zt_free
    filled -- a steady-state caller's case, zt_api.cpp host_out)."""
    import ctypes

    import numpy as np

    host = d_in.cpu().numpy()
    src = host.ctypes.data_as(ctypes.c_void_p)
    opts = zt.DeflateOpts(2, 0, level)
    out = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    zt._check(zt.lib.zt_deflate_raw(src, n, ctypes.byref(opts), ctypes.byref(out), ctypes.byref(olen)))  # warm
    zt.lib.zt_free(out)
    t0 = time.perf_counter()
    zt._check(zt.lib.zt_deflate_raw(src, n, ctypes.byref(opts), ctypes.byref(out), ctypes.byref(olen)))
    t_def = time.perf_counter() - t0
    iopts = zt.InflateOpts(1, 0x8000, 0)
    back = ctypes.POINTER(ctypes.c_uint8)()
    blen, ip = ctypes.c_size_t(), ctypes.c_size_t()
    zt._check(zt.lib.zt_inflate_raw(out, olen.value, 0, ctypes.byref(iopts), ctypes.byref(back), ctypes.byref(blen),
                                    ctypes.byref(ip)))  # warm (scratch and staging allocated once, as for deflate)
    zt.lib.zt_free(back)
    t0 = time.perf_counter()
    zt._check(zt.lib.zt_inflate_raw(out, olen.value, 0, ctypes.byref(iopts), ctypes.byref(back), ctypes.byref(blen),
                                    ctypes.byref(ip)))
    t_inf = time.perf_counter() - t0
    ok = blen.value == n and np.array_equal(np.ctypeslib.as_array(back, shape=(n,)), host)
    zt.lib.zt_free(back)
    zt.lib.zt_free(out)
    if not ok:
        raise SystemExit("bench: host API round trip mismatch")
    g = n / 2**30
    return {"deflate_GiBps": round(g / t_def, 3), "inflate_GiBps": round(g / t_inf, 3),
            "roundtrip_GiBps": round(g / (t_def + t_inf), 3),
            "note": "zt_deflate_raw of a pageable host copy, then zt_inflate_raw of its host stream, each after one "
                    "warm-up call: PCIe included; outputs from the library's host output pool (zt_free of the warm-up "
                    "outputs registered them, ZT_HOST_POOL_MB)"}


def api_node(d_in, api):
    """The same round trip from Node through the drop-in boundary north_star
    names (the zlib.ts_amd facade over the N-API addon zt.node):
    new RawDeflate(u8).compress() and new RawInflate(s).decompress() on a
    host copy of the corpus (tools/node_bench.mjs: median of 3 calls after a
    warm-up, each after the previous results were collected), plus the
    C0-shaped 64 KiB per-call latency; `vs_api` = the Node rate / the C-ABI
    rate of `api` (1.0 = no boundary overhead)."""
    import shutil
    import tempfile

    node = shutil.which("node")
    addon = os.path.join(HERE, "zlib.ts_amd", "zt.node")
    if not node or not os.path.exists(addon):
        return {"skipped": "node or zlib.ts_amd/zt.node missing"}
    tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.NamedTemporaryFile(dir=tmpdir, suffix=".bin", delete=False) as f:
        path = f.name
        d_in.cpu().numpy().tofile(f)
    try:
        p = subprocess.run([node, "--expose-gc", os.path.join(HERE, "tools", "node_bench.mjs"), path, "3"],
                           capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(path)
    if p.returncode != 0:
        raise SystemExit("bench: node bench failed: " + p.stderr[-2000:])
    r = json.loads(p.stdout.strip().splitlines()[-1])
    if api:
        r["vs_api"] = {k: round(r[k] / api[k], 3) for k in ("deflate_GiBps", "inflate_GiBps", "roundtrip_GiBps")
                       if api.get(k)}
    r["note"] = ("Node " + r.get("node", "") + ": zlib.ts_amd/lib RawDeflate / RawInflate over zt.node (results are "
                 "external ArrayBuffers over libzt's host output pool, no copy), 1 GiB corpus read from a file; "
                 "median of 3 timed calls after one warm-up")
    return r


def source_text(limit=4 << 20):
    """SURVEY 8(d)'s realistic generator: the image's /usr/lib/python3.10/*.py
    concatenated in name order, first `limit` bytes (None if absent)."""
    d = "/usr/lib/python3.10"
    if not os.path.isdir(d):
        return None
    out = bytearray()
    for name in sorted(os.listdir(d)):
        if name.endswith(".py"):
            with open(os.path.join(d, name), "rb") as f:
                out += f.read()
            if len(out) >= limit:
                break
    return bytes(out[:limit]) if len(out) >= limit else None


def per_generator(d_in, n, level, dplan, iplan, d_c, d_out, zt):
    """Untimed by the headline: deflate and inflate of `n` bytes of ONE
    generator each (wordsalad, structured int32 deltas, xorshift32 -- device
    synthetic -- and the source-text sample tiled to n bytes), the mean of 3
    calls after a warm-up through the same device plans as the timed step;
    per kind the ratio, the deflate pipeline and match kernel times and the
    inflate time (HIP events).  Overwrites d_in."""
    import torch

    out = {}
    src = source_text()
    kinds = ["wordsalad", "structured", "xorshift32"] + (["source_text"] if src else [])
    for kind in kinds:
        if kind == "source_text":
            tile = torch.frombuffer(bytearray(src), dtype=torch.uint8).cuda()
            reps = (n + len(src) - 1) // len(src)
            d_in[:n] = tile.repeat(reps)[:n]
        else:
            zt.synth_dev(kind, 11, d_in.data_ptr(), n)
        clen = dplan.run(d_in.data_ptr(), n, d_c.data_ptr())
        olen, _ = iplan.run(d_c.data_ptr(), clen, d_out.data_ptr(), d_out.numel())
        torch.cuda.synchronize()
        if olen != n or not torch.equal(d_out[:n], d_in[:n]):
            raise SystemExit(f"bench: per-generator round trip mismatch ({kind})")
        zt.timing_enable(True)
        for _ in range(3):
            clen = dplan.run(d_in.data_ptr(), n, d_c.data_ptr())
            iplan.run(d_c.data_ptr(), clen, d_out.data_ptr(), d_out.numel())
        torch.cuda.synchronize()
        t = zt.timing_read()
        zt.timing_enable(False)
        k = lambda a, b: t[a] / max(1, t[b])
        pipe, match, inf = k("deflate_pipeline_ms", "deflate_pipelines"), k("deflate_ms", "deflate_launches"), \
            k("inflate_ms", "inflate_launches")
        out[kind] = {"ratio": round(clen / n, 5), "deflate_GiBps": round(n / 2**30 / (pipe * 1e-3), 2),
                     "inflate_GiBps": round(n / 2**30 / (inf * 1e-3), 2), "deflate_pipeline_ms": round(pipe, 3),
                     "match_kernel_ms": round(match, 3), "inflate_ms": round(inf, 3)}
    out["note"] = (f"{n / 2**30:g} GiB of one generator each, level {level}, device-resident, mean of 3 after a "
                   "warm-up (HIP events); source_text = /usr/lib/python3.10/*.py, first 4 MiB, tiled")
    return out


DUMP_SAMPLE = 4 << 20  # elements per dumped array: 16 MiB as float32, two arrays per rank


def dump_outputs(path, rank, world, d_c, clen, d_out, olen):
    """--dump-outputs: what the last timed step returned to its caller, as
    float32 / float64 .npy files under `path` -- `lengths` (stream bytes,
    inflated bytes; -1 where the mode runs no inflate), `deflate_stream` (the
    stream's bytes) and `inflate_output` (the bytes inflated from it).  An
    array of more than DUMP_SAMPLE bytes is dumped as the bytes at
    DUMP_SAMPLE sorted positions drawn by a seeded generator from
    [0, length): the same positions in every run over an output of the same
    length, and a stream of another length is told apart by `lengths`."""
    import numpy as np
    import torch

    os.makedirs(path, exist_ok=True)
    tag = f"_rank{rank}" if world > 1 else ""

    def sample(buf, length):
        if length > DUMP_SAMPLE:
            idx = np.sort(np.random.default_rng(20240611).integers(0, length, size=DUMP_SAMPLE))
            return buf.index_select(0, torch.from_numpy(idx).to(buf.device)).cpu().numpy().astype(np.float32)
        return buf[:length].cpu().numpy().astype(np.float32)

    np.save(os.path.join(path, f"lengths{tag}.npy"),
            np.array([clen, -1 if olen is None else olen], dtype=np.float64))
    np.save(os.path.join(path, f"deflate_stream{tag}.npy"), sample(d_c, clen))
    if olen is not None:
        np.save(os.path.join(path, f"inflate_output{tag}.npy"), sample(d_out, olen))


# ---------------------------------------------------------------- ranks
def run_rank(args):
    import torch
    import torch.distributed as dist

    from zt_shard import max_over_ranks, shard_range, sum_over_ranks

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = torch.cuda.device_count()
    if ndev == 0:
        raise SystemExit("bench: no GPU visible")
    dev = local % ndev
    torch.cuda.set_device(dev)
    import ztamd as zt

    zt.set_device(dev)
    pg = None
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        pg = dist

    if args.mode == "c3":
        total = args.size
        lo, hi = shard_range(total, world, rank)
        n = hi - lo
        last = rank == world - 1
    else:
        total = args.size * world
        lo, n, last = 0, args.size, True
    nalloc = max(1, n)
    d_in = torch.empty(nalloc + 64, dtype=torch.uint8, device="cuda")
    if args.mode == "c3":
        zt.synth_dev_at("mixed", 11, lo, d_in.data_ptr(), n)
    else:
        zt.synth_dev("mixed", 11 + 7919 * rank, d_in.data_ptr(), n)
    bound = zt.deflate_bound(nalloc)
    d_c = torch.empty(bound + 64, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(nalloc + 4096, dtype=torch.uint8, device="cuda")
    dplan = zt.DeflatePlan(nalloc, level=args.level)
    iplan = zt.InflatePlan(bound + 64, nalloc)
    torch.cuda.synchronize()

    def deflate():
        return dplan.run(d_in.data_ptr(), n, d_c.data_ptr(), halo=0, final=1 if last else 0) if n else 0

    def inflate(clen):
        olen, _ = iplan.run(d_c.data_ptr(), clen, d_out.data_ptr(), d_out.numel())
        return olen

    def step():
        clen = deflate()
        if args.mode == "c3":
            return clen, None
        return clen, inflate(clen)

    # correctness of the measured path (untimed): the round trip is exact.
    # A plain weak-mode run checks the last timed step's own output instead
    # (below), which costs no step of its own
    precheck = args.full or args.mode == "c3"
    if precheck:
        clen = deflate()
    if precheck and n:
        slen = clen
        if not last:  # close this shard's stream with an empty final fixed block (03 00)
            d_c[clen:clen + 2] = torch.tensor([3, 0], dtype=torch.uint8, device="cuda")
            slen += 2
        olen = inflate(slen)
        torch.cuda.synchronize()
        if olen != n or not torch.equal(d_out[:n], d_in[:n]):
            raise SystemExit(f"bench: round trip mismatch on rank {rank}")
    for _ in range(args.warmup):
        step()

    def barrier():
        if pg is not None:
            pg.barrier()

    barrier()
    torch.cuda.synchronize()
    zt.timing_enable(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        clen, olen = step()
    torch.cuda.synchronize()
    barrier()
    elapsed = time.perf_counter() - t0
    kt = zt.timing_read()
    zt.timing_enable(False)
    if not precheck and n and (olen != n or not torch.equal(d_out[:n], d_in[:n])):
        raise SystemExit(f"bench: round trip mismatch on rank {rank}")
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, world, d_c, clen, d_out, olen)
    elapsed = max_over_ranks(elapsed, pg)
    total_c = sum_over_ranks(clen, pg)

    value = total * args.steps / elapsed / 2**30
    ms_step = elapsed / args.steps * 1e3
    def_ms = kt["deflate_ms"] / max(1, kt["deflate_launches"])  # match_kernel (dominant deflate kernel)
    pipe_ms = kt["deflate_pipeline_ms"] / max(1, kt["deflate_pipelines"])
    inf_ms = kt["inflate_ms"] / max(1, kt["inflate_launches"])
    tok_ms = kt["inflate_tok_ms"] / max(1, kt["inflate_toks"])
    achieved = n / (def_ms * 1e-3) / 1e9 if def_ms > 0 else 0.0
    if args.mode == "c3":
        workload = (f"config C3: RawDeflate level {args.level} of one {total / 2**30:g} GiB device-resident buffer "
                    f"sharded over {world} GPU(s) (segment-aligned shards, streams concatenate)")
        parallelism = f"shard x{world} (no collective)"
        metric = "GiB/s RawDeflate L6 of one sharded buffer (config C3); ratio vs ref"
    else:
        workload = (f"RawDeflate level {args.level} + RawInflate round trip of a {n / 2**30:g} GiB "
                    "device-resident buffer per GPU")
        parallelism = f"batch split x{world} (no collective)"
        metric = METRIC
    line = {
        "metric": metric,
        "value": round(value, 4),
        "unit": "GiB/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_step, 3),
        "higher_is_better": True,
        "scaling": "strong" if args.mode == "c3" else "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic (device-generated mixed corpus: wordsalad / xorshift32 / structured per 4 MiB window)",
        "config": {"workload": workload, "bytes_total": total, "level": args.level, "parallelism": parallelism},
        "ratio": round(total_c / max(1, total), 5),
        "match_kernel_ms": round(def_ms, 3),
        "deflate_pipeline_ms": round(pipe_ms, 3),
        "deflate_GiBps": round(n / (pipe_ms * 1e-3) / 2**30, 3) if pipe_ms else None,
        "roofline": {"bound": "hbm", "kernel": "match_kernel", "achieved": round(achieved, 3),
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 6),
                     "traffic": pmc_traffic("match_kernel", n),
                     "lds": pmc_lds("match_kernel", n)},
        "devices_visible": ndev,
    }
    if args.mode != "c3":
        line["inflate_kernel_ms"] = round(inf_ms, 3)
        line["inflate_tokenize_ms"] = round(tok_ms, 3)
        line["inflate_GiBps"] = round(n / (inf_ms * 1e-3) / 2**30, 3) if inf_ms else None
    if args.full and rank == 0 and world == 1 and args.mode == "weak":
        if not args.no_cpu_baseline and n >= 3 * WINDOW:
            cb, ratios = cpu_baseline(d_in, args.level, zt)
            line["cpu_baseline"] = cb
            line["ratio_vs_ref"] = ratios
        if not args.no_api:
            line["api"] = api_roundtrip(d_in[:n], n, args.level, zt)
            if not args.no_node:
                line["api_node"] = api_node(d_in[:n], line["api"])
        if not args.no_per_generator:
            line["per_generator"] = per_generator(d_in, n, args.level, dplan, iplan, d_c, d_out, zt)
    if rank == 0:
        print(json.dumps(line), flush=True)
    dplan.close()
    iplan.close()
    if pg is not None:
        pg.destroy_process_group()


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch(args.gpus))
    run_rank(args)


if __name__ == "__main__":
    main()
