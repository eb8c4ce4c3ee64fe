# Inflate digests per path: for each case the output's SHA-256 prefix, the end
# position, the inflate_paths delta ([segment, general, one wave]), the
# general_passes delta and the status.  Two builds (ZT_LIB=...) that must
# behave alike print identical lines.
#   usage: python tools/inf_digest.py            every case; the ZT_INF_NOPIPE and
#                                                ZT_INF_HOST_CHAIN cases in child processes
#          python tools/inf_digest.py plan|raw   one group in this process (what the children run)
import gzip, hashlib, os, random, subprocess, sys, zlib
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'zlib.ts_amd', 'py'))
import torch, ztamd as zt

KINDS = ["wordsalad", "xorshift32", "structured", "mixed"]
N = 64 << 20


def sha(*parts):
    return hashlib.sha256(b"".join(parts)).hexdigest()[:16]


def counted(label, fn):
    """runs fn() -> (outputs, end position); prints the case's line"""
    t0 = zt.timing_read()
    status, outs, end = 0, [], -1
    try:
        outs, end = fn()
    except zt.ZtError as e:
        status = e.code
    t1 = zt.timing_read()
    paths = [b - a for a, b in zip(t0["inflate_paths"], t1["inflate_paths"])]
    print(f"{label:28s} {sha(*outs)} end {end} paths {paths} general_passes "
          f"{t1['general_passes'] - t0['general_passes']} status {status}", flush=True)


def engine_streams():
    """this engine's level-6 stream of each bench generator at 64 MiB"""
    d_in = torch.empty(N, dtype=torch.uint8, device="cuda")
    d_c = torch.empty(zt.deflate_bound(N), dtype=torch.uint8, device="cuda")
    dp = zt.DeflatePlan(N, level=6)
    for kind in KINDS:
        zt.synth_dev(kind, 5, d_in.data_ptr(), N)
        clen = dp.run(d_in.data_ptr(), N, d_c.data_ptr())
        torch.cuda.synchronize()
        yield kind, d_c[:clen].clone()
    dp.close()


def group_plan(tag):
    d_out = torch.empty(N + 4096, dtype=torch.uint8, device="cuda")
    ip = zt.InflatePlan(N, N + 4096)
    for kind, d_s in engine_streams():
        def run():
            olen, end = ip.run(d_s.data_ptr(), d_s.numel(), d_out.data_ptr(), d_out.numel())
            torch.cuda.synchronize()
            return [d_out[:olen].cpu().numpy().tobytes()], end
        counted(f"{tag} {kind}", run)
    ip.close()


def group_raw(tag):
    for kind, d_s in engine_streams():
        s = d_s.cpu().numpy().tobytes()
        def run():
            out, end = zt.inflate_raw(s)
            return [out], end
        counted(f"{tag} {kind}", run)


def child(group, tag, env):
    e = dict(os.environ)
    e.update(env)
    e["INF_DIGEST_TAG"] = tag
    p = subprocess.run([sys.executable, os.path.abspath(__file__), group], env=e, capture_output=True, text=True)
    sys.stdout.write(p.stdout)
    if p.returncode:
        sys.stdout.write(f"{tag}: child exit {p.returncode}\n{p.stderr[-2000:]}\n")
    sys.stdout.flush()


if len(sys.argv) > 1:
    {"plan": group_plan, "raw": group_raw}[sys.argv[1]](os.environ.get("INF_DIGEST_TAG", sys.argv[1]))
    sys.exit(0)

group_plan("plan")
group_raw("raw_pipelined")
child("raw", "raw_nopipe", {"ZT_INF_NOPIPE": "1"})
child("plan", "plan_host_chain", {"ZT_INF_HOST_CHAIN": "1"})

d_in = torch.empty(N, dtype=torch.uint8, device="cuda")
zt.synth_dev("mixed", 9, d_in.data_ptr(), N)
mixed = d_in.cpu().numpy().tobytes()
zs = zlib.compress(mixed, 6)[2:-4]  # a zlib-made raw stream: no sync points, the general path
counted("zlib_made", lambda: (lambda r: ([r[0]], r[1]))(zt.inflate_raw(zs)))
# a multi-member gzip: a large member (this engine's), small ones, an empty one
members = [zt.gzip_compress(mixed[:24 << 20])[0], gzip.compress(mixed[100:70000], 6, mtime=0),
           gzip.compress(b"", mtime=0), zt.gzip_compress(mixed[(30 << 20):(30 << 20) + (3 << 20) + 17])[0],
           gzip.compress(mixed[5:3000], 1, mtime=0)]
counted("gunzip_members", lambda: ([zt.gunzip(b"".join(members))[0]], sum(len(m) for m in members)))
# a 64-stream batch: text, random data, an empty stream and one truncated stream
rng = random.Random(2)
items = []
for k in range(64):
    size = rng.randrange(1 << 10, 400 << 10)
    at = rng.randrange(0, len(mixed) - size)
    items.append(rng.randbytes(size) if k % 5 == 3 else mixed[at:at + size])
items[17] = b""
streams = zt.deflate_raw_batch(items, level=6)
streams[40] = streams[40][:len(streams[40]) // 2]


def batch():
    res = zt.inflate_raw_batch(streams)
    st = ",".join(str(r[0]) for r in res if r[0])
    ips = sha(*[str((r[0], r[2])).encode() for r in res])
    return [r[1] for r in res] + [st.encode(), ips.encode()], sum(r[2] for r in res if r[0] == 0)


counted("batch_64", batch)
# a stream with sync points truncated inside its last unit
ws = next(iter(engine_streams()))[1].cpu().numpy().tobytes()
counted("truncated_last_unit", lambda: (lambda r: ([r[0]], r[1]))(zt.inflate_raw(ws[:len(ws) - 1000])))
