# Digests of every batch entry point of the host batch layer: one line per
# call with a SHA-256 prefix over all outputs, statuses and messages.  Two
# builds (ZT_LIB=...) that must behave alike print identical lines.  Each call
# runs on one device, and again in a child process on 3 aliased devices
# (ZT_ALIAS_DEVICES=3, zt_set_devices(0b111)).  Compress and checksum
# batches: a fixed 40-item mix of 0 bytes to 1 MiB; decode batches: the golden
# container and inflate fixtures (tests/golden).
#   usage: python tools/batch_digest.py          both modes
#          python tools/batch_digest.py alias3   the aliased mode alone (what the child runs)
import hashlib, os, random, subprocess, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'zlib.ts_amd', 'py'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import golden_util
import ztamd as zt

MODE = sys.argv[1] if len(sys.argv) > 1 else "dev1"


def digest(label, parts):
    h = hashlib.sha256()
    for p in parts:
        b = p if isinstance(p, bytes) else repr(p).encode()
        h.update(len(b).to_bytes(8, "little") + b)
    print(f"{MODE} {label:24s} {h.hexdigest()[:16]} items {len(parts)}", flush=True)


def guarded(label, fn):
    """fn() -> a list of outputs; a call that fails as a whole prints its code and message"""
    try:
        digest(label, fn())
    except zt.ZtError as e:
        digest(label, [("error", e.code, str(e))])


def mix():
    """40 items, 0 bytes to 1 MiB: text-like, structured and incompressible, in a fixed order"""
    rng = random.Random(20)
    words = [bytes(rng.choices(b"abcdefghijklmnopqrstuvwxyz", k=rng.randrange(2, 9))) for _ in range(300)]
    sizes = [0, 32768, 1 << 20, 1, 255, 32767, 32769, 65535, 65536, 70000]
    while len(sizes) < 40:
        sizes.append(int(2 ** rng.uniform(8, 20)))
    items = []
    for k, n in enumerate(sizes):
        if k % 3 == 2:
            items.append(rng.randbytes(n))  # incompressible (among them the 1 MiB item)
        elif k % 3 == 1:
            items.append((b"%08d;" % k * (n // 9 + 1))[:n])
        else:
            items.append(b" ".join(rng.choices(words, k=n // 3 + 1))[:n])
    return items


def fixtures():
    raw = [golden_util.blob_bytes(r["stream"]) for name in ("inflate.json", "inflate_constructed.json")
           for r in golden_util.load(name)["records"]]
    gz, zl = [], []
    for r in golden_util.load("containers.json")["records"]:
        blob = r.get("output") or r.get("stream")  # (a record of a compress error has neither)
        b = golden_util.blob_bytes(blob) if blob else None
        if b is not None:
            (gz if r["kind"] in ("gzip", "gunzip") else zl).append(b)
    return [s for s in raw if s is not None], gz, zl


def decoded(res):
    """a container batch result as digest parts: status, message, output and what follows"""
    return [(int(r[0]), r[0].message, r[1], r[2:]) for r in res]


if MODE == "alias3":
    assert zt.device_count() == 3, "run with ZT_ALIAS_DEVICES=3"
    zt.set_devices(0b111)
items = mix()
dic = items[12][:4097] + items[13][:4097]
raw, gz, zl = fixtures()
guarded("gzip_compress_batch", lambda: zt.gzip_compress_batch(items, mtime=7, name=b"n"))
guarded("zlib_compress_batch", lambda: zt.zlib_compress_batch(items))
for level in (1, 6, 9):
    guarded(f"deflate_raw_batch_L{level}", lambda: zt.deflate_raw_batch(items, level=level))
for ct in (0, 1):
    guarded(f"deflate_raw_batch_ct{ct}", lambda: zt.deflate_raw_batch(items, compression_type=ct))
guarded("deflate_raw_batch_ct3", lambda: zt.deflate_raw_batch(items, compression_type=3))
guarded("crc32_batch", lambda: zt.crc32_batch(items))
raw_d = zt.deflate_raw_batch(items, dictionary=dic)
zl_d = zt.zlib_compress_batch(items, dictionary=dic)
digest("deflate_raw_batch_dict", raw_d)
digest("zlib_compress_batch_dict", zl_d)
guarded("inflate_raw_batch_dict", lambda: zt.inflate_raw_batch(raw_d, dictionary=dic))
guarded("inflate_raw_batch", lambda: zt.inflate_raw_batch(raw))
guarded("inflate_raw_batch_strict", lambda: zt.inflate_raw_batch(raw, ref_strict=True))
guarded("gunzip_batch", lambda: decoded(zt.gunzip_batch(gz + zl[:3])))
guarded("zlib_decompress_batch", lambda: decoded(zt.zlib_decompress_batch(zl + gz[:3], verify=True)))
guarded("zlib_decompress_batch_d", lambda: decoded(zt.zlib_decompress_batch(zl_d + zl, verify=True, dictionary=dic)))
guarded("zlib_decompress_batch_nd", lambda: decoded(zt.zlib_decompress_batch(zl_d[:5] + zl)))

# ---- every writer of a member's frame (csrc/member_frame.h): the single-buffer
# calls, BGZF and the device-resident batch
text = items[9]  # 70000 bytes of words
guarded("gzip_compress", lambda: list(zt.gzip_compress(text, name=b"n", hcrc=True, mtime=7)))
guarded("gzip_compress_indexed", lambda: list(zt.gzip_compress_indexed(text, name=b"n", hcrc=True, mtime=7)))
guarded("zlib_compress", lambda: list(zt.zlib_compress(text)))
guarded("zlib_compress_indexed", lambda: list(zt.zlib_compress_indexed(text)))
guarded("zlib_compress_dict", lambda: list(zt.zlib_compress(text, dictionary=dic)))
for bs in (4096, 0):
    for level in (0, 6):
        guarded(f"bgzf_compress_bs{bs}_L{level}", lambda: [
            p for n in (0, 1, 4096, 4097, 70000)
            for p in zt.bgzf_compress(text[:n], level=level, block_size=bs, want_index=True)])


def dev_batch(fmt, ct):
    """sizes 0 .. 70000 through zt_deflate_dev_batch, item 3 with too little room:
    per item its status, the length it reports and the bytes it wrote"""
    import torch
    srcs = [text[:n] for n in (0, 1, 65535, 65536, 70000)]
    pieces = [s + bytes(-len(s) % 256 + 256) for s in srcs]  # (each from a 256-byte boundary)
    offs = [sum(len(p) for p in pieces[:k]) for k in range(len(srcs))]
    tin = torch.frombuffer(bytearray(b"".join(pieces)), dtype=torch.uint8).cuda()
    caps = [zt.deflate_dev_batch_bound(len(s), ct, fmt) for s in srcs]
    caps[3] = 100
    room = max(caps) + 256
    out = torch.full((room * len(srcs),), 0xA5, dtype=torch.uint8, device="cuda")
    lens, st = zt.deflate_dev_batch([tin.data_ptr() + o for o in offs], [len(s) for s in srcs],
                                    [out.data_ptr() + k * room for k in range(len(srcs))], caps, format=fmt,
                                    compression_type=ct)
    torch.cuda.synchronize()
    got = out.cpu().numpy().tobytes()
    return [(st[k], lens[k], got[k * room:k * room + (lens[k] if st[k] == 0 else room)]) for k in range(len(srcs))]


for fmt in ("raw", "zlib", "gzip"):
    for ct in (0, 1, 2):
        guarded(f"deflate_dev_batch_{fmt}_ct{ct}", lambda: dev_batch(fmt, ct))
if MODE == "dev1":
    sys.stdout.flush()
    env = dict(os.environ, ZT_ALIAS_DEVICES="3")
    sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "alias3"], env=env).returncode)
