#!/usr/bin/env python3
"""Measures the read-side container batch calls (include/zt_container_batch.h)
against the single calls on the MI355X and writes
profiles/container_batch_time.json (the record DESIGN.md section 7 quotes).

Workload: the C4 members (tests/c4_corpus.py: 10 000 files, ~1.41 GiB,
written by zt_gzip_compress_batch / zt_zlib_compress_batch).

  gzip (a)  a loop of zt_gunzip per file
  gzip (b)  the members joined 500 to a file, zt_gunzip per file
  gzip (c)  one zt_gunzip_batch of the 10 000
  gzip (d)  one zt_gunzip_batch of the 20 joined files
  zlib (a)  a loop of zt_zlib_decompress per file, verify on
  zlib (c)  one zt_zlib_decompress_batch of the 10 000, verify on
  dict      4096 messages of 4 KiB (the 4 KiB row of tools/dict_time.py) with
            the corpus dictionary: a loop of zt_zlib_decompress_dict against
            one zt_zlib_decompress_batch_dict, verify on

Method: wall time of the whole C call(s) through ctypes (packing, upload,
kernels, download; every call ends synchronised), outputs freed inside the
timed region; median of 5 after 2 warm-up rounds; the old and the new calls
alternate in one process (every round runs each row once).  Every output is
compared with the input once, outside the timed region.  Baselines are (a)
and (b): those entry points are what they were before the batch calls.

    python tools/container_batch_time.py [--out profiles/container_batch_time.json] [--files 10000]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib.ts_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

JOIN = 500
REPS, WARM = 5, 2


def log(msg):
    print(msg, file=sys.stderr, flush=True)


class Items:
    """ctypes views of a list of inputs, so that the timed region is the C calls"""

    def __init__(self, items):
        self.k = len(items)
        self.bs = [bytes(x) for x in items]
        self.addr = [ctypes.cast(ctypes.c_char_p(x), ctypes.c_void_p).value for x in self.bs]
        self.n = [len(x) for x in self.bs]
        self.ptrs = (ctypes.c_void_p * self.k)(*self.addr)
        self.lens = (ctypes.c_size_t * self.k)(*self.n)
        self.outs = (ctypes.POINTER(ctypes.c_uint8) * self.k)()
        self.olens = (ctypes.c_size_t * self.k)()
        self.ips = (ctypes.c_size_t * self.k)()
        self.adl = (ctypes.c_uint32 * self.k)()
        self.mems = None  # (zt_gunzip_batch: set by main, the member type comes from the binding)
        self.cnts = (ctypes.c_size_t * self.k)()
        self.st = (ctypes.c_int * self.k)()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "container_batch_time.json"))
    ap.add_argument("--files", type=int, default=10000)
    a = ap.parse_args()
    import dict_corpus
    import zt_oracle
    import ztamd as zt
    from c4_corpus import c4_files

    lib = zt.lib
    assert zt.device_count() > 0, "no GPU visible"
    files = c4_files(zt_oracle.Oracle(), count=a.files)
    nbytes = sum(len(f) for f in files)
    log(f"corpus: {len(files)} files, {nbytes} bytes")
    gz = zt.gzip_compress_batch(files, mtime=0)
    zl = zt.zlib_compress_batch(files)
    joined = [b"".join(gz[i:i + JOIN]) for i in range(0, len(gz), JOIN)]
    joined_want = [b"".join(files[i:i + JOIN]) for i in range(0, len(files), JOIN)]
    D = dict_corpus.dictionary()
    text = b"".join(dict_corpus.records(3, 4096 * 4096 // 300 + 64))
    msgs = [text[i * 4096:(i + 1) * 4096] for i in range(4096)]
    dz = zt.zlib_compress_batch(msgs, dictionary=D)
    dbytes = sum(len(m) for m in msgs)
    dbuf = ctypes.create_string_buffer(D, len(D))
    G, Z, J, DZ = Items(gz), Items(zl), Items(joined), Items(dz)
    for I in (G, J):
        I.mems = (ctypes.POINTER(zt.GzipMember) * I.k)()
    u8p = ctypes.POINTER(ctypes.c_uint8)
    check = {"on": True}

    def loop_gunzip(I, want):
        def run():
            o, ol, mem, cnt = u8p(), ctypes.c_size_t(), ctypes.POINTER(zt.GzipMember)(), ctypes.c_size_t()
            for i in range(I.k):
                rc = lib.zt_gunzip(I.addr[i], I.n[i], ctypes.byref(o), ctypes.byref(ol), ctypes.byref(mem),
                                   ctypes.byref(cnt))
                assert rc == 0, lib.zt_last_error_message()
                if check["on"]:
                    assert ctypes.string_at(o, ol.value) == want[i]
                lib.zt_free(o)
                lib.zt_free(mem)
        return run

    def batch_gunzip(I, want):
        def run():
            rc = lib.zt_gunzip_batch(I.ptrs, I.lens, I.k, I.outs, I.olens, I.mems, I.cnts, I.st)
            assert rc == 0, lib.zt_last_error_message()
            for i in range(I.k):
                if check["on"]:
                    assert ctypes.string_at(I.outs[i], I.olens[i]) == want[i]
                lib.zt_free(I.outs[i])
                lib.zt_free(I.mems[i])
        return run

    def loop_zlib(I, want, use_dict):
        def run():
            o, ol, ip, ad = u8p(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint32()
            for i in range(I.k):
                if use_dict:
                    rc = lib.zt_zlib_decompress_dict(I.addr[i], I.n[i], 0, 1, dbuf, len(D), ctypes.byref(o),
                                                     ctypes.byref(ol), ctypes.byref(ip), ctypes.byref(ad))
                else:
                    rc = lib.zt_zlib_decompress(I.addr[i], I.n[i], 0, 1, ctypes.byref(o), ctypes.byref(ol),
                                                ctypes.byref(ip), ctypes.byref(ad))
                assert rc == 0, lib.zt_last_error_message()
                if check["on"]:
                    assert ctypes.string_at(o, ol.value) == want[i]
                lib.zt_free(o)
        return run

    def batch_zlib(I, want, use_dict):
        def run():
            if use_dict:
                rc = lib.zt_zlib_decompress_batch_dict(I.ptrs, I.lens, None, I.k, 1, dbuf, len(D), I.outs, I.olens,
                                                       I.ips, I.adl, I.st)
            else:
                rc = lib.zt_zlib_decompress_batch(I.ptrs, I.lens, None, I.k, 1, I.outs, I.olens, I.ips, I.adl, I.st)
            assert rc == 0, lib.zt_last_error_message()
            for i in range(I.k):
                if check["on"]:
                    assert ctypes.string_at(I.outs[i], I.olens[i]) == want[i]
                lib.zt_free(I.outs[i])
        return run

    rows = [
        ("gzip_a_loop_per_file", loop_gunzip(G, files), nbytes),
        ("gzip_c_batch_files", batch_gunzip(G, files), nbytes),
        ("gzip_b_loop_joined", loop_gunzip(J, joined_want), nbytes),
        ("gzip_d_batch_joined", batch_gunzip(J, joined_want), nbytes),
        ("zlib_a_loop_verify", loop_zlib(Z, files, False), nbytes),
        ("zlib_c_batch_verify", batch_zlib(Z, files, False), nbytes),
        ("dict4k_loop_verify", loop_zlib(DZ, msgs, True), dbytes),
        ("dict4k_batch_verify", batch_zlib(DZ, msgs, True), dbytes),
    ]
    times = {name: [] for name, _, _ in rows}
    stats = {}
    for r in range(WARM + REPS):
        check["on"] = r == 0  # (outputs compared once, in the first warm-up round)
        for name, fn, _ in rows:
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                times[name].append(dt)
            if name.startswith("gzip") and "batch" in name:
                stats[name] = zt.gunzip_batch_stats()
            log(f"round {r} {name}: {dt:.1f} ms")
    out_rows = {}
    for name, _, nb in rows:
        med = statistics.median(times[name])
        out_rows[name] = {"ms_median": round(med, 2), "ms_all": [round(t, 2) for t in times[name]],
                          "GiB_per_s": round(nb / (1 << 30) / (med * 1e-3), 3), "decoded_bytes": nb}
        if name in stats:
            out_rows[name]["stats"] = stats[name]
    pairs = [("gzip_c_batch_files", "gzip_a_loop_per_file"), ("gzip_d_batch_joined", "gzip_b_loop_joined"),
             ("zlib_c_batch_verify", "zlib_a_loop_verify"), ("dict4k_batch_verify", "dict4k_loop_verify")]
    verdict = {}
    for new, old in pairs:
        f = out_rows[old]["ms_median"] / out_rows[new]["ms_median"]
        verdict[f"{new}_over_{old}"] = {"speedup": round(f, 2), "not_slower": f >= 1.0}
    doc = {"tool": "tools/container_batch_time.py", "device": "MI355X (gfx950)", "files": len(files),
           "joined_files": len(joined), "members_per_joined_file": JOIN, "dict_messages": len(msgs),
           "timed": f"wall, whole C call(s) incl. zt_free of the outputs, median of {REPS} after {WARM} warm-up rounds, "
                    "old and new alternating in one process",
           "rows": out_rows, "verdict": verdict}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(verdict))
    return 0


if __name__ == "__main__":
    sys.exit(main())
