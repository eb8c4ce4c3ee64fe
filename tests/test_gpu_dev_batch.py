"""Device-resident batch deflate and inflate over pointer arrays
(include/zt_dev_batch.h; csrc/dev_batch.hip, csrc/dev_batch_api.cpp).

Every input batch is one uint8 cuda tensor with the items close together at
chosen addresses modulo 16 (the few bytes between two items are junk, so a read
outside an item that mattered would change the result); every output batch is
one tensor filled with 0xA5 in which each item has 64 canary bytes on either
side.  After a call the whole output tensor is compared with its expected
image, so the canaries, the unused capacity behind a result and the buffers of
items that must not be written are all checked byte by byte.

Deflate results are compared with the host batch calls over the same bytes
(byte-identical) and, independently, decoded by Python's zlib; inflate results
with the originals and with zt_inflate_raw_batch's lengths, end positions,
statuses and message."""
import hashlib
import zlib

import pytest

pytestmark = pytest.mark.gpu

ZT_E_ARG = -103
SIZES = [0, 1, 15, 16, 17, 4095, 32767, 32768, 32769, 65535, 65536, 65537, 100001]
FORMATS = {"raw": -15, "zlib": 15, "gzip": 31}  # zlib.decompress's wbits


@pytest.fixture(scope="module")
def zt():
    import ztamd

    assert ztamd.device_count() > 0, "no GPU visible"
    return ztamd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def _gen(oracle, k, n):
    """item k of n bytes: text, incompressible and structured data in turn"""
    return oracle.gen(["wordsalad", "xorshift32", "structured"][k % 3], 100 + k, n)


@pytest.fixture(scope="module")
def sweep_items(oracle):
    """32 items: the first sixteen will sit at source addresses base + 0..15, the
    last sixteen at destination addresses base + 0..15; every size of SIZES
    occurs in both halves"""
    return [_gen(oracle, k, SIZES[(k * 5 + k // 16) % len(SIZES)]) for k in range(32)]


SWEEP_SRC = [k % 16 if k < 16 else 0 for k in range(32)]
SWEEP_DST = [0 if k < 16 else k % 16 for k in range(32)]


@pytest.fixture(scope="module")
def host_ref(zt, sweep_items):
    """the host batch calls' outputs over the sweep items, computed once per (format, level)"""
    cache = {}

    def get(fmt, level, items=None, compression_type=2):
        key = (fmt, level, compression_type, id(items) if items is not None else 0)
        if key not in cache:
            fn = {"raw": zt.deflate_raw_batch, "zlib": zt.zlib_compress_batch, "gzip": zt.gzip_compress_batch}[fmt]
            cache[key] = fn(items if items is not None else sweep_items, level=level,
                            compression_type=compression_type)
        return cache[key]

    return get


def _to_dev(torch, items, mis=None):
    """items placed one after the other, item k at an address = mis[k] mod 16;
    returns (tensor, device pointers)"""
    mis = mis or [0] * len(items)
    buf, offs = bytearray(b"\x3c" * 256), []
    for k, it in enumerate(items):
        while len(buf) % 16 != mis[k]:
            buf.append(0xC0 | (len(buf) & 15))
        offs.append(len(buf))
        buf += it
    buf += b"\x3c" * 64
    t = torch.frombuffer(buf, dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t, [t.data_ptr() + o for o in offs]


class Outputs:
    """one 0xA5 tensor; item k's buffer of caps[k] bytes at an address = mis[k]
    mod 16 with 64 canary bytes before and after it"""

    def __init__(self, torch, caps, mis=None):
        mis = mis or [0] * len(caps)
        pos, self.offs = 0, []
        for k, c in enumerate(caps):
            pos += 64
            while pos % 16 != mis[k]:
                pos += 1
            self.offs.append(pos)
            pos += c + 64
        self.total = pos + 64
        self.t = torch.full((self.total,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptrs = [self.t.data_ptr() + o for o in self.offs]
        self.caps = list(caps)

    def check(self, expected):
        """expected[k]: the bytes item k's buffer must start with, or None for a
        buffer that must be untouched; everything else must still be 0xA5"""
        img = bytearray(b"\xa5" * self.total)
        for o, e in zip(self.offs, expected):
            if e is not None:
                img[o:o + len(e)] = e
        got = self.t.cpu().numpy().tobytes()
        if got != bytes(img):
            bad = next(i for i in range(self.total) if got[i] != img[i])
            item = max([k for k, o in enumerate(self.offs) if o - 64 <= bad], default=-1)
            raise AssertionError(f"output image differs at byte {bad} (item {item}, offset {bad - self.offs[item]})")


def _dev_deflate(zt, torch, items, fmt, level, src_mis=None, dst_mis=None, caps=None, compression_type=2, stream=None):
    tin, ptrs = _to_dev(torch, items, src_mis)
    if caps is None:
        caps = [zt.deflate_dev_batch_bound(len(x), compression_type, fmt, level) for x in items]
    out = Outputs(torch, caps, dst_mis)
    lens, st = zt.deflate_dev_batch(ptrs, [len(x) for x in items], out.ptrs, caps, format=fmt, level=level,
                                    compression_type=compression_type, stream=stream)
    torch.cuda.synchronize()
    return out, lens, st


def _dev_inflate(zt, torch, streams, caps, src_mis=None, dst_mis=None, checksums=False, index=None):
    tin, ptrs = _to_dev(torch, streams, src_mis)
    out = Outputs(torch, caps, dst_mis)
    res = zt.inflate_dev_batch(ptrs, [len(x) for x in streams], out.ptrs, caps, index=index, checksums=checksums)
    torch.cuda.synchronize()
    return (out,) + tuple(res)


# ---- alignment sweep ----------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("fmt", ["raw", "zlib", "gzip"])
def test_deflate_alignment_sweep(zt, torch, sweep_items, host_ref, fmt, level):
    want = host_ref(fmt, level)
    out, lens, st = _dev_deflate(zt, torch, sweep_items, fmt, level, SWEEP_SRC, SWEEP_DST)
    assert st == [0] * 32
    assert lens == [len(w) for w in want]
    out.check(want)  # byte-identical to the host call, nothing else written
    for item, w in zip(sweep_items, want):  # independently: Python's zlib reads them
        assert zlib.decompress(w, FORMATS[fmt]) == item


def test_inflate_alignment_sweep(zt, torch, sweep_items, host_ref):
    streams = host_ref("raw", 6)
    ref = zt.inflate_raw_batch(streams)
    out, lens, ips, st = _dev_inflate(zt, torch, streams, [len(x) for x in sweep_items], SWEEP_SRC, SWEEP_DST)
    assert st == [r[0] for r in ref] == [0] * 32
    assert lens == [len(r[1]) for r in ref] == [len(x) for x in sweep_items]
    assert ips == [r[2] for r in ref]
    out.check(sweep_items)


def test_groups_do_not_change_a_byte(zt, torch, sweep_items, host_ref, monkeypatch):
    """ZT_DEV_BATCH_GROUP_BYTES (read at every call) cuts the sweep into several
    groups that reuse the scratch one after the other: the same bytes, lengths,
    end positions and checksums"""
    monkeypatch.setenv("ZT_DEV_BATCH_GROUP_BYTES", "200000")
    for fmt in ("gzip", "raw"):
        want = host_ref(fmt, 6)
        out, lens, st = _dev_deflate(zt, torch, sweep_items, fmt, 6, SWEEP_SRC, SWEEP_DST)
        assert st == [0] * 32 and lens == [len(w) for w in want]
        out.check(want)
    streams = host_ref("raw", 6)
    short = [len(x) - (1 if k in (5, 30) else 0) for k, x in enumerate(sweep_items)]
    out, lens, ips, st, crcs, adlers = _dev_inflate(zt, torch, streams, short, SWEEP_SRC, SWEEP_DST, checksums=True)
    assert st == [ZT_E_ARG if k in (5, 30) else 0 for k in range(32)]
    assert lens == [len(x) for x in sweep_items] and ips == [r[2] for r in zt.inflate_raw_batch(streams)]
    assert crcs == [zlib.crc32(x) for x in sweep_items] and adlers == [zlib.adler32(x) for x in sweep_items]
    out.check([None if k in (5, 30) else x for k, x in enumerate(sweep_items)])


# ---- both decoder routes --------------------------------------------------------------
@pytest.fixture(scope="module")
def route_streams(zt, oracle):
    """(original, raw stream) pairs: Python's zlib at levels 0, 1, 6, 9 and with
    Z_FIXED, and the engine's own streams"""
    pairs = []
    for k, (n, level, strategy) in enumerate([(70001, 0, 0), (40000, 1, 0), (100001, 6, 0), (32769, 9, 0),
                                              (5000, 6, zlib.Z_FIXED), (17, 6, 0), (0, 6, 0)]):
        d = _gen(oracle, 40 + k, n)
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        pairs.append((d, c.compress(d) + c.flush()))
    own = [_gen(oracle, 50 + k, n) for k, n in enumerate([65537, 1, 33000])]
    pairs += list(zip(own, zt.deflate_raw_batch(own)))
    return pairs


@pytest.mark.parametrize("checksums", [False, True])
@pytest.mark.parametrize("count", [1, 3, 9])
def test_inflate_routes(zt, torch, route_streams, count, checksums):
    """count < 8 without checksums: the one-wave decoder; count >= 8 or
    checksums: two-phase, its leftovers and too-small first guesses by one wave"""
    batches = [[route_streams[(a + j) % len(route_streams)] for j in range(count)]
               for a in range(0, len(route_streams), count)]
    for batch in batches:
        data, streams = [b[0] for b in batch], [b[1] for b in batch]
        ref = zt.inflate_raw_batch(streams)
        res = _dev_inflate(zt, torch, streams, [len(d) for d in data], src_mis=[(3 * j + 1) % 16 for j in range(count)],
                           dst_mis=[(7 * j + 5) % 16 for j in range(count)], checksums=checksums)
        out, lens, ips, st = res[:4]
        assert st == [r[0] for r in ref] == [0] * count
        assert lens == [len(d) for d in data] and ips == [r[2] for r in ref]
        out.check(data)
        if checksums:
            assert res[4] == [zlib.crc32(d) for d in data]
            assert res[5] == [zlib.adler32(d) for d in data]


def test_inflate_index_skips_a_header(zt, torch, oracle):
    d = [_gen(oracle, 60 + k, 20000 + k) for k in range(3)]
    members = [zlib.compress(x, 6) for x in d]  # 2-byte header, stream, Adler-32
    out, lens, ips, st = _dev_inflate(zt, torch, members, [len(x) for x in d], index=[2, 2, 2])
    assert st == [0, 0, 0] and lens == [len(x) for x in d]
    assert ips == [len(m) - 4 for m in members]
    out.check(d)


# ---- capacity ---------------------------------------------------------------------------
def test_deflate_capacity(zt, torch, sweep_items, host_ref):
    """exact capacity succeeds; one byte less: ZT_E_ARG, the length needed,
    buffer and canaries untouched, neighbours right"""
    items = sweep_items[3:12]
    want = zt.gzip_compress_batch(items, level=6)
    exact = [len(w) for w in want]
    out, lens, st = _dev_deflate(zt, torch, items, "gzip", 6, caps=exact, dst_mis=list(range(9)))
    assert st == [0] * 9 and lens == exact
    out.check(want)
    short = [c - 1 if k in (0, 4, 8) else c for k, c in enumerate(exact)]
    out, lens, st = _dev_deflate(zt, torch, items, "gzip", 6, caps=short, dst_mis=list(range(9)))
    assert st == [ZT_E_ARG if k in (0, 4, 8) else 0 for k in range(9)]
    assert lens == exact
    assert zt.lib.zt_last_error_message() == b"output capacity too small"
    out.check([None if k in (0, 4, 8) else w for k, w in enumerate(want)])


def test_inflate_capacity_and_sizes_only(zt, torch, sweep_items, host_ref):
    items = sweep_items[16:28]
    streams = zt.deflate_raw_batch(items)
    exact = [len(x) for x in items]
    out, lens, ips, st = _dev_inflate(zt, torch, streams, exact)
    assert st == [0] * 12 and lens == exact
    out.check(items)
    tight = [k for k in range(12) if exact[k] > 0][::3]
    short = [c - 1 if k in tight else c for k, c in enumerate(exact)]
    for sub in (slice(0, 12), slice(0, 3)):  # both routes
        sel = list(range(12))[sub]
        out, lens, ips, st = _dev_inflate(zt, torch, streams[sub], short[sub])
        assert st == [ZT_E_ARG if k in tight else 0 for k in sel]
        assert lens == exact[sub]
        assert zt.lib.zt_last_error_message() == b"output capacity too small"
        out.check([None if k in tight else items[k] for k in sel])
        # sizes only: the same lengths, nothing written (there is nothing to write to)
        tin, ptrs = _to_dev(torch, streams[sub])
        lens2, ips2, st2 = zt.inflate_dev_batch(ptrs, [len(s) for s in streams[sub]], None)
        assert lens2 == exact[sub] and st2 == [0] * len(sel) and ips2 == ips


@pytest.mark.parametrize("ctype", [0, 1, 2])
def test_bound_holds_on_incompressible(zt, torch, oracle, ctype):
    """out_cap = the bound always succeeds and no output exceeds it: random
    bytes, where every block is coded at its worst"""
    items = [oracle.gen("xorshift32", 7 + k, n) for k, n in enumerate(SIZES + [33 * 32768 + 5])]
    for fmt in ("raw", "gzip"):
        caps = [zt.deflate_dev_batch_bound(len(x), ctype, fmt) for x in items]
        out, lens, st = _dev_deflate(zt, torch, items, fmt, 6, caps=caps, compression_type=ctype)
        assert st == [0] * len(items)
        assert all(l <= c for l, c in zip(lens, caps))
        got = out.t.cpu().numpy().tobytes()
        for x, o, l in zip(items, out.offs, lens):
            assert zlib.decompress(got[o:o + l], FORMATS[fmt]) == x


# ---- errors among good items ------------------------------------------------------------
def test_errors_among_good_items(zt, torch, oracle):
    d = [_gen(oracle, 70 + k, 30000 + 1000 * k) for k in range(10)]
    good = zt.deflate_raw_batch(d)
    for count in (10, 4):  # two-phase with one-wave leftovers; one wave alone
        streams, data = list(good[:count]), list(d[:count])
        streams[1] = streams[1][:len(streams[1]) // 2]  # truncated
        # a stored block with a bad NLEN: like the reference (src/RawInflate.ts:277)
        # the decoder never compares NLEN with ~LEN, its NLEN error is a field
        # that does not lie whole inside the input
        streams[2] = b"\x01\x05\x00\xfa"
        ref = zt.inflate_raw_batch(streams)
        ref_msg = zt.lib.zt_last_error_message()
        assert ref[1][0] != 0 and ref[2][0] == -14  # ZT_E_STORED_NLEN
        out, lens, ips, st = _dev_inflate(zt, torch, streams, [len(x) for x in data])
        assert zt.lib.zt_last_error_message() == ref_msg
        assert st == [r[0] for r in ref]
        assert lens == [len(r[1]) for r in ref]
        assert [ips[k] for k in range(count) if st[k] == 0] == [ref[k][2] for k in range(count) if st[k] == 0]
        out.check([None if st[k] else data[k] for k in range(count)])


# ---- stored and empty -------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["raw", "zlib", "gzip"])
def test_stored_and_empty(zt, torch, sweep_items, fmt):
    items = sweep_items[:14] + [b"", b""]
    fn = {"raw": zt.deflate_raw_batch, "zlib": zt.zlib_compress_batch, "gzip": zt.gzip_compress_batch}[fmt]
    for kw in (dict(compression_type=0, level=6), dict(compression_type=2, level=0)):
        want = fn(items, **kw)
        out, lens, st = _dev_deflate(zt, torch, items, fmt, kw["level"], src_mis=list(range(16)),
                                     dst_mis=[(k * 3) % 16 for k in range(16)],
                                     compression_type=kw["compression_type"])
        assert st == [0] * 16 and lens == [len(w) for w in want]
        out.check(want)
    # an empty item, compressing options: the final empty stored block, framed
    out, lens, st = _dev_deflate(zt, torch, [b"", b"abc", b""], fmt, 6)
    got = out.t.cpu().numpy().tobytes()
    frame = {"raw": (b"", b""), "zlib": (b"\x78\x9c", b"\x00\x00\x00\x01"),
             "gzip": (b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03", b"\x00" * 8)}[fmt]
    for k in (0, 2):
        assert got[out.offs[k]:out.offs[k] + lens[k]] == frame[0] + b"\x01\x00\x00\xff\xff" + frame[1]
    assert zlib.decompress(got[out.offs[1]:out.offs[1] + lens[1]], FORMATS[fmt]) == b"abc"


# ---- the caller's stream ------------------------------------------------------------------
def test_callers_stream(zt, torch):
    """inputs produced by a torch op on a non-default stream, that stream passed,
    outputs consumed on it with no synchronisation in between"""
    n, k = 1 << 16, 12
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        # (a long enough chain of ops that the inputs are not ready when the call is made)
        x = torch.arange(n * k, device="cuda", dtype=torch.int64)
        for _ in range(20):
            x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 40)
        src = ((x >> 20) % 7 + 65).to(torch.uint8)  # compressible letters
        caps = [zt.deflate_dev_batch_bound(n, 2, "gzip")] * k
        comp = torch.full((k * 70000,), 0xA5, dtype=torch.uint8, device="cuda")
        lens, st = zt.deflate_dev_batch([src.data_ptr() + i * n for i in range(k)], [n] * k,
                                        [comp.data_ptr() + i * 70000 for i in range(k)], caps, format="gzip",
                                        stream=s.cuda_stream)
        assert st == [0] * k
        back = torch.zeros(n * k, dtype=torch.uint8, device="cuda")
        lens2, ips, st2 = zt.inflate_dev_batch([comp.data_ptr() + i * 70000 for i in range(k)], lens,
                                               [back.data_ptr() + i * n for i in range(k)], [n] * k, index=[10] * k,
                                               stream=s.cuda_stream)
        same = torch.equal(back, src)  # consumed on the same stream
        comp_host = comp.cpu()
        src_host = src.cpu().numpy().tobytes()
    assert st2 == [0] * k and lens2 == [n] * k and same
    cb = comp_host.numpy().tobytes()
    for i in range(k):
        assert zlib.decompress(cb[i * 70000:i * 70000 + lens[i]], 31) == src_host[i * n:(i + 1) * n]


# ---- the host calls are unchanged ------------------------------------------------------------
# sha256 over the host batch calls' outputs for the corpus of _host_digest,
# produced once by running the parent commit's build (the commit before the
# device-resident calls were added) on an MI355X
PARENT_HOST_DIGEST = "4f473ee46b4c25ffdd4a6d3a3bb08a8f709bf0fca37cf4204e2e43f047e62f8d"


def _host_digest(zt, oracle):
    items = [_gen(oracle, 200 + k, SIZES[(3 * k) % len(SIZES)] + 7 * k) for k in range(26)]
    h = hashlib.sha256()

    def add(parts):
        for p in parts:
            h.update(len(p).to_bytes(8, "little"))
            h.update(p)

    for level in (1, 6, 9):
        add(zt.deflate_raw_batch(items, level=level))
    for ct in (0, 1):
        add(zt.deflate_raw_batch(items, compression_type=ct))
    add(zt.gzip_compress_batch(items, level=6))
    add(zt.gzip_compress_batch(items[:5], level=9))
    streams = zt.deflate_raw_batch(items) + [zlib.compress(x, lv)[2:-4] for lv, x in enumerate(items[:10])]
    streams[3] = streams[3][:len(streams[3]) // 2]
    for sub in (streams, streams[:5]):  # two-phase and one-wave routes
        for st, data, ip in zt.inflate_raw_batch(sub):
            add([st.to_bytes(4, "little", signed=True), data, (ip if st == 0 else 0).to_bytes(8, "little")])
    return h.hexdigest()


def test_host_calls_unchanged(zt, oracle):
    assert _host_digest(zt, oracle) == PARENT_HOST_DIGEST


# ---- torch conveniences --------------------------------------------------------------------
def test_tensor_round_trip(zt, torch, oracle):
    big = torch.frombuffer(bytearray(_gen(oracle, 90, 300000)), dtype=torch.uint8).cuda()
    ts = [big[1:40001], big[40001:40001], big[50003:150004], torch.empty(0, dtype=torch.uint8, device="cuda"),
          big[150007:150008], big[200000:]]
    for fmt in ("raw", "gzip"):
        comp = zt.deflate_tensors(ts, format=fmt)
        assert len(comp) == len(ts) and all(c.is_cuda and c.dtype == torch.uint8 for c in comp)
        for t, c in zip(ts, comp):
            assert zlib.decompress(c.cpu().numpy().tobytes(), FORMATS[fmt]) == t.cpu().numpy().tobytes()
    comp = zt.deflate_tensors(ts)
    back = zt.inflate_tensors(comp)
    assert [b.numel() for b in back] == [t.numel() for t in ts]
    assert all(torch.equal(b, t) for b, t in zip(back, ts))
    back = zt.inflate_tensors(comp, out_sizes=[t.numel() for t in ts])
    assert all(torch.equal(b, t) for b, t in zip(back, ts))
    # on a non-default current stream too
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        back = zt.inflate_tensors(zt.deflate_tensors(ts, format="raw"))
        ok = all(torch.equal(b, t) for b, t in zip(back, ts))
    assert ok
    assert zt.deflate_tensors([]) == [] and zt.inflate_tensors([]) == []
