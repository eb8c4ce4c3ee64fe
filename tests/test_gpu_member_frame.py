"""The writers of a gzip, zlib or raw member agree (csrc/member_frame.h is their
one description of the frame): the single-buffer call, the host batch call and
zt_deflate_dev_batch give the same member for the same input, format and
compression type, and every member decodes with Python's zlib to the input with
nothing left over.

No combination is left out: on the build before member_frame.h the three
writers already agreed byte for byte for all five inputs, the three formats and
both compression types (the single-buffer call and the batch pipeline write the
same body here even above one 32 KiB block), so BODY_DIFFERS is empty.  A
combination listed there would still have its prefix and trailer bytes compared
and every member decoded."""
import zlib

import pytest

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 65535, 65536, 70000]
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
FRAME = {"raw": (0, 0), "zlib": (2, 4), "gzip": (10, 8)}  # prefix and trailer bytes (gzip: default options)
# (format, compression type, input bytes) whose single-buffer body is not the batch pipeline's: none
BODY_DIFFERS = set()


@pytest.fixture(scope="module")
def items(oracle):
    return [oracle.gen("wordsalad", 7, n) for n in SIZES]


def single_members(zt, fmt, ct, items):
    if fmt == "raw":
        return [zt.deflate_raw(x, compression_type=ct) for x in items]
    fn = zt.zlib_compress if fmt == "zlib" else zt.gzip_compress
    return [fn(x, compression_type=ct)[0] for x in items]


def batch_members(zt, fmt, ct, items):
    fn = {"raw": zt.deflate_raw_batch, "zlib": zt.zlib_compress_batch, "gzip": zt.gzip_compress_batch}[fmt]
    return fn(items, compression_type=ct)


def dev_members(zt, torch, fmt, ct, items):
    pieces = [x + bytes(-len(x) % 256 + 256) for x in items]  # (each from a 256-byte boundary)
    offs = [sum(len(p) for p in pieces[:k]) for k in range(len(items))]
    tin = torch.frombuffer(bytearray(b"".join(pieces)), dtype=torch.uint8).cuda()
    caps = [zt.deflate_dev_batch_bound(len(x), ct, fmt) for x in items]
    room = max(caps) + 256
    out = torch.full((room * len(items),), 0xA5, dtype=torch.uint8, device="cuda")
    lens, st = zt.deflate_dev_batch([tin.data_ptr() + o for o in offs], [len(x) for x in items],
                                    [out.data_ptr() + k * room for k in range(len(items))], caps, format=fmt,
                                    compression_type=ct)
    torch.cuda.synchronize()
    assert st == [0] * len(items)
    got = out.cpu().numpy().tobytes()
    return [got[k * room:k * room + lens[k]] for k in range(len(items))]


@pytest.mark.parametrize("ct", [0, 2])
@pytest.mark.parametrize("fmt", ["raw", "zlib", "gzip"])
def test_writers_agree(oracle, items, fmt, ct):
    import torch
    import ztamd as zt

    one, batch, dev = single_members(zt, fmt, ct, items), batch_members(zt, fmt, ct, items), dev_members(
        zt, torch, fmt, ct, items)
    plen, tl = FRAME[fmt]
    for x, a, b, d in zip(items, one, batch, dev):
        assert b == d, (fmt, ct, len(x))
        if (fmt, ct, len(x)) in BODY_DIFFERS:
            assert a[:plen] == b[:plen] and a[len(a) - tl:] == b[len(b) - tl:], (fmt, ct, len(x))
        else:
            assert a == b, (fmt, ct, len(x))
        for m in (a, b):
            z = zlib.decompressobj(WBITS[fmt])
            assert z.decompress(m) == x and z.eof and z.unused_data == b"", (fmt, ct, len(x))
