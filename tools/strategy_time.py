# Deflate with a strategy against the search, all in one run: the device-
# resident 1 GiB corpus (bench.py's mixed generator) and 1 GiB of each
# generator, deflated with level 1, level 6, ZT_STRATEGY_RLE and
# ZT_STRATEGY_HUFFMAN_ONLY (level 6 parse).  Per configuration: the pipeline's
# GiB/s and the res-producer kernel's time (match_kernel or strategy_kernel:
# the same timing slot), medians with interquartile ranges over --reps runs
# after a warm-up, and the strategies' achieved fraction of the HBM rate (they
# move 5 bytes per input byte: 1 read, 4 written).  No threshold: the
# comparison that matters is against level 1 of the same run.
#   usage: python tools/strategy_time.py [--size BYTES] [--reps N] [--out profiles/strategy_time.json]
import argparse, json, os, statistics, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'zlib.ts_amd', 'py'))
import torch, ztamd as zt

HBM_PEAK = 8.0e12  # bytes/s, the MI355X's specified HBM3E rate
CONFIGS = [("level1", 1, None), ("level6", 6, None), ("rle", 6, zt.STRATEGY_RLE),
           ("huffman_only", 6, zt.STRATEGY_HUFFMAN_ONLY)]
KINDS = ["mixed", "wordsalad", "xorshift32", "structured"]


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return {"median": round(statistics.median(v), 4), "q1": round(q[0], 4), "q3": round(q[2], 4)}


ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1 << 30)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(HERE, '..', 'profiles', 'strategy_time.json'))
args = ap.parse_args()
n = args.size
d_in = torch.empty(n, dtype=torch.uint8, device="cuda")
d_c = torch.empty(zt.deflate_bound(n), dtype=torch.uint8, device="cuda")
result = {"bytes": n, "reps": args.reps, "hbm_peak_bytes_per_s": HBM_PEAK, "generators": {}}
for kind in KINDS:
    zt.synth_dev(kind, 11, d_in.data_ptr(), n)
    row = {}
    for name, level, strategy in CONFIGS:
        dp = zt.DeflatePlan(n, level=level, strategy=strategy)
        dp.run(d_in.data_ptr(), n, d_c.data_ptr())
        torch.cuda.synchronize()
        kern, pipe, clen = [], [], 0
        for _ in range(args.reps):
            zt.timing_enable(True)
            clen = dp.run(d_in.data_ptr(), n, d_c.data_ptr())
            torch.cuda.synchronize()
            t = zt.timing_read()
            zt.timing_enable(False)
            kern.append(t["deflate_ms"])
            pipe.append(t["deflate_pipeline_ms"])
        dp.close()
        r = {"ratio": round(clen / n, 5), "producer_ms": quartiles(kern), "pipeline_ms": quartiles(pipe),
             "deflate_GiBps": round(n / 2**30 / (statistics.median(pipe) * 1e-3), 2)}
        if strategy is not None:
            r["producer_hbm_fraction"] = round(5 * n / (statistics.median(kern) * 1e-3) / HBM_PEAK, 3)
        row[name] = r
        print(f"{kind:11s} {name:13s} ratio {r['ratio']:.4f}  producer {r['producer_ms']['median']:8.3f} ms "
              f"[{r['producer_ms']['q1']:.3f}, {r['producer_ms']['q3']:.3f}]  pipeline {r['pipeline_ms']['median']:8.3f} ms "
              f"[{r['pipeline_ms']['q1']:.3f}, {r['pipeline_ms']['q3']:.3f}]  {r['deflate_GiBps']:7.2f} GiB/s"
              + (f"  HBM {r['producer_hbm_fraction']:.3f}" if strategy is not None else ""), flush=True)
    for name in ("rle", "huffman_only"):
        row[name]["faster_than_level1"] = row[name]["pipeline_ms"]["median"] < row["level1"]["pipeline_ms"]["median"]
    result["generators"][kind] = row
result["every_generator_faster_than_level1"] = {
    name: all(result["generators"][k][name]["faster_than_level1"] for k in KINDS) for name in ("rle", "huffman_only")}
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result["every_generator_faster_than_level1"]))
