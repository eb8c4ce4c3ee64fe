#!/usr/bin/env python3
"""Measures the preset-dictionary calls (include/zt_dict.h) on the MI355X and
writes profiles/dict_time.json (the record DESIGN.md and
tests/test_gpu_dict.py quote).

Rows: batches of 4096 messages of about 350 B (tests/dict_corpus.py), 4 KiB
and 64 KiB (records of the same generator joined and cut), each with and
without the corpus dictionary: zt_deflate_raw_batch[_dict] and
zt_inflate_raw_batch[_dict] through ctypes, wall time of the whole C call
(packing, upload, kernels, download; the call ends synchronised), median of 5
after 2 warm-up calls; GiB/s of message bytes; the match kernel's and the
whole deflate pipeline's device time (HIP events, zt_timing_read) of one
further call; the compressed totals and their ratio to zlib level 6 with the
same zdict (64 KiB rows: over the first 256 messages, zlib on the CPU being
the slow part).  Last, one 64 MiB message written with the dictionary and
read back through zt_inflate_raw_dict (one wavefront decodes it).

Each row runs in a child process under a time limit; the first failure stops
the run.

    python tools/dict_time.py [--out profiles/dict_time.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib.ts_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

COUNT = 4096
ROWS = {"350B": 0, "4KiB": 4096, "64KiB": 65536}
LIMIT_S = 400


def batch_messages(each):
    import dict_corpus

    if each == 0:
        return dict_corpus.messages(COUNT)
    text = b"".join(dict_corpus.records(3, COUNT * each // 300 + 64))
    assert len(text) >= COUNT * each
    return [text[i * each:(i + 1) * each] for i in range(COUNT)]


def zlib_total(msgs, d):
    tot = 0
    for m in msgs:
        c = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=d) if d else zlib.compressobj(6, zlib.DEFLATED, -15)
        tot += len(c.compress(m)) + len(c.flush())
    return tot


class Batch:
    """ctypes arrays of one batch, so that the timed region is the C call"""

    def __init__(self, zt, items):
        self.zt = zt
        self.k = len(items)
        self.bs = [bytes(x) for x in items]
        self.ptrs = (ctypes.c_void_p * self.k)(*[ctypes.cast(ctypes.c_char_p(x), ctypes.c_void_p).value
                                                 for x in self.bs])
        self.lens = (ctypes.c_size_t * self.k)(*[len(x) for x in self.bs])
        self.outs = (ctypes.POINTER(ctypes.c_uint8) * self.k)()
        self.olens = (ctypes.c_size_t * self.k)()
        self.ips = (ctypes.c_size_t * self.k)()
        self.st = (ctypes.c_int * self.k)()

    def take(self, keep):
        res = [ctypes.string_at(self.outs[i], self.olens[i]) for i in range(self.k)] if keep else None
        total = sum(self.olens[i] for i in range(self.k))
        for i in range(self.k):
            self.zt.lib.zt_free(self.outs[i])
        return res, total


def timed(fn, reps=5, warm=2):
    ts = []
    for r in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if r >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), [round(t, 3) for t in ts]


def child_batch(name, use_dict):
    import dict_corpus
    import ztamd as zt

    assert zt.device_count() > 0, "no GPU visible"
    d = dict_corpus.dictionary() if use_dict else b""
    dbuf = ctypes.create_string_buffer(d, len(d) or 1)
    msgs = batch_messages(ROWS[name])
    nbytes = sum(len(m) for m in msgs)
    b = Batch(zt, msgs)
    dopts = zt.DeflateOpts(2, 0, -1)
    iopts = zt.InflateOpts(1, 0x8000, 0)
    state = {}

    def deflate(keep=False):
        if use_dict:
            rc = zt.lib.zt_deflate_raw_batch_dict(b.ptrs, b.lens, b.k, ctypes.byref(dopts), dbuf, len(d), b.outs,
                                                  b.olens, b.st)
        else:
            rc = zt.lib.zt_deflate_raw_batch(b.ptrs, b.lens, b.k, ctypes.byref(dopts), b.outs, b.olens, b.st)
        assert rc == 0, zt.lib.zt_last_error_message()
        state["streams"], state["total"] = b.take(keep)

    deflate(keep=True)
    streams, comp_total = state["streams"], state["total"]
    ms_d, all_d = timed(deflate)
    zt.timing_enable(True)
    t0 = zt.timing_read()
    deflate()
    t1 = zt.timing_read()
    zt.timing_enable(False)
    sb = Batch(zt, streams)

    def inflate(keep=False):
        if use_dict:
            rc = zt.lib.zt_inflate_raw_batch_dict(sb.ptrs, sb.lens, sb.k, ctypes.byref(iopts), dbuf, len(d), sb.outs,
                                                  sb.olens, sb.ips, sb.st)
        else:
            rc = zt.lib.zt_inflate_raw_batch(sb.ptrs, sb.lens, sb.k, ctypes.byref(iopts), sb.outs, sb.olens, sb.ips,
                                             sb.st)
        assert rc == 0, zt.lib.zt_last_error_message()
        state["back"], _ = sb.take(keep)

    inflate(keep=True)
    assert state["back"] == msgs, "round trip differs"
    ms_i, all_i = timed(inflate)
    sample = msgs if ROWS[name] < 65536 else msgs[:256]
    ours = comp_total if sample is msgs else sum(len(s) for s in streams[:256])
    ref = zlib_total(sample, d)
    gib = nbytes / (1 << 30)
    print(json.dumps({
        "row": name, "dictionary_bytes": len(d), "items": COUNT, "message_bytes": nbytes,
        "deflate_ms_median": round(ms_d, 3), "deflate_ms_all": all_d, "deflate_GiB_per_s": round(gib / (ms_d * 1e-3), 3),
        "match_kernel_ms": round(t1["deflate_ms"] - t0["deflate_ms"], 3),
        "deflate_pipeline_ms": round(t1["deflate_pipeline_ms"] - t0["deflate_pipeline_ms"], 3),
        "inflate_ms_median": round(ms_i, 3), "inflate_ms_all": all_i, "inflate_GiB_per_s": round(gib / (ms_i * 1e-3), 3),
        "compressed_total": comp_total, "ratio_sample_items": len(sample), "ratio_sample_ours": ours,
        "ratio_sample_zlib6": ref, "ratio_to_zlib6": round(ours / ref, 4),
        "timed": "wall, whole C call, median of 5 after 2 warm-up calls"}))


def child_big():
    import dict_corpus
    import ztamd as zt

    assert zt.device_count() > 0, "no GPU visible"
    d = dict_corpus.dictionary()
    n = 64 << 20
    text = b"".join(dict_corpus.records(4, 4096))
    msg = (text * (n // len(text) + 1))[:n]
    s = zt.deflate_raw(msg, dictionary=d)
    out, ip = zt.inflate_raw(s, dictionary=d)
    assert out == msg and ip == len(s)
    sb, n_s = zt._cbuf(s)
    dbuf = ctypes.create_string_buffer(d, len(d))
    iopts = zt.InflateOpts(1, 0x8000, 0)

    def run():
        o = ctypes.POINTER(ctypes.c_uint8)()
        ol, ipv = ctypes.c_size_t(), ctypes.c_size_t()
        rc = zt.lib.zt_inflate_raw_dict(sb, n_s, 0, ctypes.byref(iopts), dbuf, len(d), ctypes.byref(o),
                                        ctypes.byref(ol), ctypes.byref(ipv))
        assert rc == 0 and ol.value == n
        zt.lib.zt_free(o)

    ms, all_ = timed(run, reps=3, warm=1)
    print(json.dumps({"row": "one_64MiB_stream_inflate", "dictionary_bytes": len(d), "message_bytes": n,
                      "compressed_bytes": len(s), "inflate_ms_median": round(ms, 2), "inflate_ms_all": all_,
                      "inflate_GiB_per_s": round(n / (1 << 30) / (ms * 1e-3), 4),
                      "timed": "wall, whole C call (one wavefront decodes the stream), median of 3 after 1 warm-up"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_time.json"))
    ap.add_argument("--child")
    ap.add_argument("--dict", type=int, default=0)
    a = ap.parse_args()
    if a.child == "big":
        child_big()
        return 0
    if a.child:
        child_batch(a.child, bool(a.dict))
        return 0
    rows = []
    jobs = [(name, dflag) for name in ROWS for dflag in (0, 1)] + [("big", 1)]
    for name, dflag in jobs:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--dict", str(dflag)],
                               capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{name} (dict {dflag}): time limit of {LIMIT_S} s", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"{name} (dict {dflag}): exit {p.returncode}\n{p.stderr[-2000:]}", file=sys.stderr)
            return 1
        row = json.loads(p.stdout.strip().splitlines()[-1])
        rows.append(row)
        print(json.dumps(row), flush=True)
    corpus = next(r for r in rows if r["row"] == "350B" and r["dictionary_bytes"])
    plain = next(r for r in rows if r["row"] == "350B" and not r["dictionary_bytes"])
    doc = {"tool": "tools/dict_time.py", "device": "MI355X (gfx950)",
           "corpus_ratio_to_zlib6": corpus["ratio_to_zlib6"],
           "corpus_dictionary_over_plain": round(corpus["compressed_total"] / plain["compressed_total"], 4),
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
