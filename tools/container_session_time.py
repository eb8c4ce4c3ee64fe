#!/usr/bin/env python3
"""Times the container sessions (include/zt_stream_container.h) on the MI355X
and writes profiles/container_session_time.json (the record README.md and
DESIGN.md section 7.3 quote).

Workload: 1024 gzip files of 64 KiB each, the C4 mix of kinds
(tests/c4_corpus.py: wordsalad, source text, xorshift32, structured), each one
member made by CPU zlib at level 6, fed in 4 rounds of quarter pieces.

    gzip_sessions   1024 GunzipSessions, 4 zt_container_sessions_feed calls
    raw_sessions    the same DEFLATE bodies (header and trailer cut off)
                    through 1024 InflateSessions, 4 zt_inflate_sessions_feed
                    calls: what the container layer adds on top
    gunzip_batch    one zt_gunzip_batch of the whole files

Neither ratio is a gate: the gates are the launch and work counters of
tests/test_gpu_container_session.py.

Method: wall time through ctypes around calls that end synchronised, outputs
freed inside the timed region (creating and closing the sessions is outside
it); every row runs once per round, the rows alternating in one process;
medians and interquartile ranges over REPS rounds after WARM warm-up rounds;
outputs compared with the data in the first warm-up round only.

    python tools/container_session_time.py [--out profiles/container_session_time.json] [--rehearse]
"""
import argparse
import gzip
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib.ts_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS, WARM = 5, 1
FILES = 1024
FILE_BYTES = 64 << 10
ROUNDS = 4


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def summary(ts):
    q = statistics.quantiles(ts, n=4)
    return {"ms_median": round(statistics.median(ts), 3), "ms_iqr": [round(q[0], 3), round(q[2], 3)],
            "ms_all": [round(t, 3) for t in ts]}


def build_files(oracle):
    from ratio_corpus import source_text

    src = source_text()
    files = []
    for i in range(FILES):
        kind = ("wordsalad", "xorshift32", None, "structured")[i % 4]
        if kind is None:
            off = (i * 104729) % (len(src) - FILE_BYTES)
            files.append(src[off:off + FILE_BYTES])
        else:
            files.append(oracle.gen(kind, 400003 + i, FILE_BYTES))
    return files


def quarters(items):
    return [[s[len(s) * k // ROUNDS:len(s) * (k + 1) // ROUNDS] for s in items] for k in range(ROUNDS)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "container_session_time.json"))
    ap.add_argument("--rehearse", action="store_true", help="build the inputs, print their sizes and stop (no GPU)")
    a = ap.parse_args()
    import zt_oracle

    raws = build_files(zt_oracle.Oracle())
    members = [gzip.compress(r, 6, mtime=0) for r in raws]
    bodies = [m[10:-8] for m in members]
    assert all(m[3] == 0 for m in members)  # (no optional header field: the body starts at byte 10)
    data_bytes = sum(len(r) for r in raws)
    log(f"{len(members)} files, {sum(len(m) for m in members)} -> {data_bytes} bytes")
    if a.rehearse:
        return 0
    import ztamd as zt

    assert zt.device_count() > 0, "no GPU visible"
    check = {"on": True}
    member_q, body_q = quarters(members), quarters(bodies)
    infos = {}

    def gzip_sessions():
        ss = [zt.GunzipSession() for _ in members]
        t0 = time.perf_counter()
        outs = [zt.container_sessions_feed(ss, member_q[k], last=k == ROUNDS - 1) for k in range(ROUNDS)]
        dt = (time.perf_counter() - t0) * 1e3
        if check["on"]:
            for i, raw in enumerate(raws):
                assert all(outs[k][i][0] == 0 for k in range(ROUNDS)), i
                assert b"".join(outs[k][i][1] for k in range(ROUNDS)) == raw, i
            info = [s.info() for s in ss]
            assert all(x["finished"] and x["members_done"] == 1 for x in info)
            infos["gzip_sessions"] = {"launches_max": max(x["launches"] for x in info),
                                      "launches_total": sum(x["launches"] for x in info)}
        for s in ss:
            s.close()
        return dt

    def raw_sessions():
        ss = [zt.InflateSession() for _ in bodies]
        t0 = time.perf_counter()
        outs = [zt.inflate_sessions_feed(ss, body_q[k], last=k == ROUNDS - 1) for k in range(ROUNDS)]
        dt = (time.perf_counter() - t0) * 1e3
        if check["on"]:
            for i, raw in enumerate(raws):
                assert b"".join(outs[k][i][1] for k in range(ROUNDS)) == raw, i
            info = [s.info() for s in ss]
            infos["raw_sessions"] = {"launches_max": max(x["launches"] for x in info),
                                     "launches_total": sum(x["launches"] for x in info)}
        for s in ss:
            s.close()
        return dt

    def gunzip_batch():
        t0 = time.perf_counter()
        res = zt.gunzip_batch(members)
        dt = (time.perf_counter() - t0) * 1e3
        if check["on"]:
            assert all(st == 0 and out == raw for (st, out, _), raw in zip(res, raws))
        return dt

    rows = [("gzip_sessions", gzip_sessions), ("raw_sessions", raw_sessions), ("gunzip_batch", gunzip_batch)]
    times = {name: [] for name, _ in rows}
    for r in range(WARM + REPS):
        check["on"] = r == 0
        for name, fn in rows:
            dt = fn()
            if r >= WARM:
                times[name].append(dt)
            log(f"round {r} {name}: {dt:.2f} ms")
    out_rows = {}
    for name, _ in rows:
        out_rows[name] = summary(times[name])
        out_rows[name]["MiB_per_s"] = round(data_bytes / (1 << 20) / (out_rows[name]["ms_median"] * 1e-3), 1)
        if name in infos:
            out_rows[name]["session_info"] = infos[name]
    med = {k: v["ms_median"] for k, v in out_rows.items()}
    verdict = {
        "gzip_sessions_over_raw_sessions": round(med["gzip_sessions"] / med["raw_sessions"], 3),
        "gzip_sessions_over_gunzip_batch": round(med["gzip_sessions"] / med["gunzip_batch"], 3),
    }
    doc = {"tool": "tools/container_session_time.py", "device": "MI355X (gfx950)",
           "workload": {"files": len(members), "file_bytes": FILE_BYTES, "stream_bytes": sum(len(m) for m in members),
                        "data_bytes": data_bytes, "rounds": ROUNDS,
                        "kind": "C4 mix (wordsalad, source text, xorshift32, structured), CPU zlib level 6"},
           "timed": f"wall through ctypes, calls end synchronised, outputs freed inside, sessions created and closed "
                    f"outside; median and interquartile range of {REPS} rounds after {WARM} warm-up rounds, rows "
                    f"alternating in one process",
           "rows": out_rows, "verdict": verdict}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(verdict))
    return 0


if __name__ == "__main__":
    sys.exit(main())
