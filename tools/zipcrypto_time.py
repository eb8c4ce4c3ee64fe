#!/usr/bin/env python3
"""Measures the ZipCrypto path on the MI355X and writes
profiles/zipcrypto_time.json (the record DESIGN.md quotes).

Every step runs in a child process of its own under a time limit, once with
the CRC table in LDS (ZT_ZC_TABLE=1) and once with the table-free register
step (ZT_ZC_TABLE=0), alternating; the first failure stops the run.  The
cipher rates are device-side: HIP events around the kernels
(zt_zipcrypto_last_kernel_ms), bytes of the streams over the median of the
timed calls after two warm-up calls.  The zip_compress rows are wall time of
the whole C call (upload, deflate, CRC, cipher, download, layout).

    python tools/zipcrypto_time.py [--out profiles/zipcrypto_time.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib.ts_amd", "py"))

MIB = 1 << 20
# name: (kind, streams, bytes each, repeats, time limit of the child in s)
STEPS = {
    "encrypt_1x256MiB": ("enc", 1, 256 * MIB, 5, 240),
    "encrypt_4096x64KiB": ("enc", 4096, 64 << 10, 5, 240),
    "decrypt_1x16MiB": ("dec", 1, 16 * MIB, 3, 240),
    "decrypt_4096x64KiB": ("dec", 4096, 64 << 10, 5, 240),
    "zip_1000x64KiB_plain": ("zip", 1000, 64 << 10, 5, 240),
    "zip_1000x64KiB_password": ("zip_pw", 1000, 64 << 10, 5, 240),
}


def corpus(count, each):
    import numpy as np

    # half text-like, half random, so that the zip rows deflate something
    rs = np.random.RandomState(12345)
    words = rs.randint(97, 123, size=each, dtype=np.uint8).tobytes()
    out = []
    for i in range(count):
        out.append(words[i % 251:] + words[:i % 251] if i % 2 else rs.bytes(each))
    return out


def child(step):
    import ztamd

    kind, count, each, reps, _ = STEPS[step]
    assert ztamd.device_count() > 0, "no GPU visible"
    items = corpus(count, each)
    total = count * each
    times = []
    if kind in ("enc", "dec"):
        fn = ztamd.zipcrypto_encrypt if kind == "enc" else ztamd.zipcrypto_decrypt
        for r in range(reps + 2):
            fn(items, b"password")
            if r >= 2:
                times.append(ztamd.zipcrypto_last_kernel_ms())
    else:
        files = [dict(data=d, name=b"f%04d" % i, method=8) for i, d in enumerate(items)]
        if kind == "zip_pw":
            for f in files:
                f["password"] = b"password"
        for r in range(reps + 2):
            t0 = time.perf_counter()
            ztamd.zip_compress(files)
            if r >= 2:
                times.append((time.perf_counter() - t0) * 1e3)
    ms = statistics.median(times)
    print(json.dumps({"step": step, "streams": count, "bytes_each": each, "ms_median": round(ms, 4),
                      "ms_all": [round(t, 4) for t in times], "GiB_per_s": round(total / (ms * 1e-3) / (1 << 30), 3),
                      "timed": "device events" if kind in ("enc", "dec") else "wall, whole call"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zipcrypto_time.json"))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    rows = []
    for step, spec in STEPS.items():
        for table in ("1", "0"):
            if spec[0] == "zip" and table == "0":
                continue  # no cipher in it
            env = dict(os.environ, ZT_ZC_TABLE=table)
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step], env=env,
                                   capture_output=True, text=True, timeout=spec[4])
            except subprocess.TimeoutExpired:
                print(f"{step} (table {table}): time limit of {spec[4]} s", file=sys.stderr)
                return 1
            if p.returncode != 0:
                print(f"{step} (table {table}): exit {p.returncode}\n{p.stderr[-2000:]}", file=sys.stderr)
                return 1
            row = json.loads(p.stdout.strip().splitlines()[-1])
            row["crc_step"] = "lds_table" if table == "1" else "table_free"
            rows.append(row)
            print(json.dumps(row), flush=True)
    doc = {"tool": "tools/zipcrypto_time.py", "device": "MI355X (gfx950)", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
