#!/usr/bin/env python3
"""Times the inflate sessions (include/zt_stream.h) on the MI355X and writes
profiles/stream_session_time.json (the record README.md and DESIGN.md
section 7 quote).

  (a) one stream in pieces: 8 MiB of wordsalad as the reference's one-block
      stream (the oracle's RawDeflate), fed in 16 and in 128 equal pieces
        session     one InflateSession, only the new bytes per feed
        resume      ztamd.RawInflateStream on the same cuts (zt_inflate_raw_resume:
                    block-granular, the whole input so far on every call)
        batch_of_1  one zt_inflate_raw_batch of that single stream: the one-wave floor
  (b) many small streams: 1024 C2-style 64 KiB reference streams
      (tests/c2_corpus.py)
        sessions    1024 sessions fed in 4 rounds of quarter pieces
                    (4 zt_inflate_sessions_feed calls)
        batch       one zt_inflate_raw_batch of the whole streams

The one condition that follows from the design: a session's total time at
128 pieces is below twice its total time at 16 pieces (its work is linear in
the input; the block-granular path's is the sum of the prefix lengths).

Method: wall time through ctypes around calls that end synchronised, outputs
freed inside the timed region; every row runs once per round, the rows
alternating in one process; medians and interquartile ranges over REPS
rounds after WARM warm-up rounds; outputs compared with the data in the first
warm-up round only.

    python tools/stream_session_time.py [--out profiles/stream_session_time.json] [--rehearse]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib.ts_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS, WARM = 5, 1
ONE_BYTES = 8 << 20
STREAMS = 1024
ROUNDS = 4


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def equal_cuts(n, pieces):
    return [n * (k + 1) // pieces for k in range(pieces)]


def summary(ts):
    q = statistics.quantiles(ts, n=4)
    return {"ms_median": round(statistics.median(ts), 3), "ms_iqr": [round(q[0], 3), round(q[2], 3)],
            "ms_all": [round(t, 3) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_session_time.json"))
    ap.add_argument("--rehearse", action="store_true", help="build the inputs, print their sizes and stop (no GPU)")
    a = ap.parse_args()
    import c2_corpus
    import zt_oracle

    oracle = zt_oracle.Oracle()
    one = oracle.gen("wordsalad", 77, ONE_BYTES)
    one_stream, _ = oracle.raw_deflate(one)
    corpus = c2_corpus.build(oracle, count=STREAMS)
    raws = [r for r, _, _ in corpus]
    streams = [s for _, s, _ in corpus]
    small_bytes = sum(len(r) for r in raws)
    log(f"(a) {len(one)} bytes -> one block of {len(one_stream)} bytes; (b) {len(streams)} streams, "
        f"{sum(len(s) for s in streams)} -> {small_bytes} bytes")
    if a.rehearse:
        return 0
    import ztamd as zt

    assert zt.device_count() > 0, "no GPU visible"
    check = {"on": True}

    def session_pieces(pieces):
        cuts = equal_cuts(len(one_stream), pieces)

        def run():
            parts, prev = [], 0
            with zt.InflateSession() as ses:
                for cut in cuts:
                    parts.append(ses.feed(one_stream[prev:cut], last=cut == len(one_stream)))
                    prev = cut
                info = ses.info()
            if check["on"]:
                assert b"".join(parts) == one and info["finished"]
            return info
        return run

    def resume_pieces(pieces):
        cuts = equal_cuts(len(one_stream), pieces)

        def run():
            st = zt.RawInflateStream()
            parts = [st.decompress(one_stream[:cut]) for cut in cuts]
            if check["on"]:
                assert b"".join(parts) == one and st.bfinal
        return run

    def batch_of_one():
        res = zt.inflate_raw_batch([one_stream])
        if check["on"]:
            assert res[0][0] == 0 and res[0][1] == one

    quarter = [[s[len(s) * k // ROUNDS:len(s) * (k + 1) // ROUNDS] for s in streams] for k in range(ROUNDS)]

    def sessions_rounds():
        ss = [zt.InflateSession() for _ in streams]
        t0 = time.perf_counter()
        outs = [zt.inflate_sessions_feed(ss, quarter[k], last=k == ROUNDS - 1) for k in range(ROUNDS)]
        dt = (time.perf_counter() - t0) * 1e3
        if check["on"]:
            for i, raw in enumerate(raws):
                assert b"".join(outs[k][i][1] for k in range(ROUNDS)) == raw, i
        for s in ss:
            s.close()
        return dt  # (creating and closing 1024 sessions is not part of a feed round)

    def batch_whole():
        res = zt.inflate_raw_batch(streams)
        if check["on"]:
            assert all(st == 0 and out == raw for (st, out, _), raw in zip(res, raws))

    rows = [
        ("a_session_16", session_pieces(16)), ("a_session_128", session_pieces(128)),
        ("a_resume_16", resume_pieces(16)), ("a_resume_128", resume_pieces(128)),
        ("a_batch_of_1", batch_of_one),
        ("b_sessions_4_rounds", sessions_rounds), ("b_batch_whole", batch_whole),
    ]
    times = {name: [] for name, _ in rows}
    infos = {}
    for r in range(WARM + REPS):
        check["on"] = r == 0
        for name, fn in rows:
            t0 = time.perf_counter()
            ret = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if name == "b_sessions_4_rounds":
                dt = ret
            elif isinstance(ret, dict):
                infos[name] = {k: ret[k] for k in ("launches", "decoded_bits", "end_bits")}
            if r >= WARM:
                times[name].append(dt)
            log(f"round {r} {name}: {dt:.2f} ms")
    out_rows = {}
    for name, _ in rows:
        out_rows[name] = summary(times[name])
        nb = small_bytes if name.startswith("b_") else len(one)
        out_rows[name]["MiB_per_s"] = round(nb / (1 << 20) / (out_rows[name]["ms_median"] * 1e-3), 1)
        if name in infos:
            out_rows[name]["session_info"] = infos[name]
    med = {k: v["ms_median"] for k, v in out_rows.items()}
    verdict = {
        "session_128_over_16": round(med["a_session_128"] / med["a_session_16"], 3),
        "session_128_below_twice_16": med["a_session_128"] < 2 * med["a_session_16"],
        "resume_128_over_16": round(med["a_resume_128"] / med["a_resume_16"], 3),
        "session_16_over_batch_of_1": round(med["a_session_16"] / med["a_batch_of_1"], 3),
        "b_sessions_over_batch": round(med["b_sessions_4_rounds"] / med["b_batch_whole"], 3),
    }
    doc = {"tool": "tools/stream_session_time.py", "device": "MI355X (gfx950)",
           "a": {"data_bytes": len(one), "stream_bytes": len(one_stream), "kind": "wordsalad, one dynamic block"},
           "b": {"streams": len(streams), "stream_bytes": sum(len(s) for s in streams), "data_bytes": small_bytes,
                 "rounds": ROUNDS},
           "timed": f"wall through ctypes, calls end synchronised, outputs freed inside; median and interquartile "
                    f"range of {REPS} rounds after {WARM} warm-up rounds, rows alternating in one process",
           "rows": out_rows, "verdict": verdict}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(verdict))
    return 0


if __name__ == "__main__":
    sys.exit(main())
