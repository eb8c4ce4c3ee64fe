# Deflate output digests and match/pipeline times per corpus (128 MiB) and
# level: two builds (ZT_LIB=...) that must give identical streams print
# identical digests.   usage: [DF_LEVELS=6,1,9] python tools/df_digest.py [kinds...]
import hashlib, os, sys; sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'zlib.ts_amd', 'py'))
import torch, ztamd as zt
kinds = sys.argv[1:] or ["wordsalad", "xorshift32", "structured", "mixed"]
n = 128 << 20
d_in = torch.empty(n, dtype=torch.uint8, device="cuda")
d_c = torch.empty(zt.deflate_bound(n), dtype=torch.uint8, device="cuda")
for level in [int(x) for x in os.environ.get("DF_LEVELS", "6,1,9").split(",")]:
    dp = zt.DeflatePlan(n, level=level)
    for kind in kinds:
        zt.synth_dev(kind, 5, d_in.data_ptr(), n)
        clen = dp.run(d_in.data_ptr(), n, d_c.data_ptr())
        zt.timing_enable(True)
        for _ in range(2):
            clen = dp.run(d_in.data_ptr(), n, d_c.data_ptr())
        torch.cuda.synchronize()
        t = zt.timing_read(); zt.timing_enable(False)
        h = hashlib.sha256(d_c[:clen].cpu().numpy().tobytes()).hexdigest()[:16]
        print(f"L{level} {kind:10s} {h} ratio {clen/n:.5f} match {t['deflate_ms']/t['deflate_launches']:6.2f} ms "
              f"pipeline {t['deflate_pipeline_ms']/t['deflate_pipelines']:6.2f} ms", flush=True)
    dp.close()

# the driver's other paths (seconds): stored / fixed blocks, n = 0, device
# shards with a halo, the batch and dictionary-batch pipelines, multi-block
# workgroups on a small input
import random


def sha(*parts):
    return hashlib.sha256(b"".join(parts)).hexdigest()[:16]


def corpus(kind, seed, size):
    zt.synth_dev(kind, seed, d_in.data_ptr(), size)
    return d_in[:size].cpu().numpy().tobytes()


mixed = corpus("mixed", 7, 32 << 20)
buf = mixed[:(3 << 20) + 5]
for ct in (0, 1):
    print(f"path ctype{ct}      {sha(zt.deflate_raw(buf, compression_type=ct))}", flush=True)
print(f"path empty       {sha(*[zt.deflate_raw(b'', compression_type=ct) for ct in (0, 1, 2)])}", flush=True)
dp = zt.DeflatePlan(1 << 20)
parts = []
for final in (1, 0):
    k = dp.run(d_in.data_ptr(), 0, d_c.data_ptr(), final=final)
    torch.cuda.synchronize()
    parts.append(d_c[:k].cpu().numpy().tobytes())
dp.close()
print(f"path empty_dev   {sha(*parts)}", flush=True)
# as tests/test_gpu_deflate.py::test_device_shards_concatenate drives it
t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
per = ((len(buf) + 3) // 4 + 32767) // 32768 * 32768
dp = zt.DeflatePlan(per)
parts = []
for k in range(4):
    lo, hi = k * per, min(len(buf), (k + 1) * per)
    m = dp.run(t.data_ptr() + lo, hi - lo, d_c.data_ptr(), halo=min(lo, 32768), final=1 if hi == len(buf) else 0)
    torch.cuda.synchronize()
    parts.append(d_c[:m].cpu().numpy().tobytes())
dp.close()
print(f"path shards      {sha(*parts)}", flush=True)
rng = random.Random(1)
files = []
for _ in range(64):
    size = rng.randrange(1 << 10, 400 << 10)
    at = rng.randrange(0, len(mixed) - size)
    files.append(mixed[at:at + size])
for level in (1, 6, 9):
    print(f"path batch_L{level}    {sha(*zt.deflate_raw_batch(files, level=level))}", flush=True)
print(f"path batch_ct1   {sha(*zt.deflate_raw_batch(files, compression_type=1))}", flush=True)
st = corpus("structured", 3, (1 << 20) + (16 << 10))
dic, msgs = st[:16 << 10], [st[(16 << 10) + 4096 * i:(16 << 10) + 4096 * (i + 1)] for i in range(256)]
print(f"path dict_raw    {sha(*zt.deflate_raw_batch(msgs, dictionary=dic))}", flush=True)
print(f"path dict_zlib   {sha(*zt.zlib_compress_batch(msgs, dictionary=dic))}", flush=True)
os.environ["ZT_DF_SUPER_MIN"] = "4"
print(f"path super_min4  {sha(zt.deflate_raw(mixed[:256 << 10]))}", flush=True)
del os.environ["ZT_DF_SUPER_MIN"]
