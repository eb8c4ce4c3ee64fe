"""BGZF in plain Python (zlib, struct, gzip only): a writer and a parser of
the block layout of SAM spec 4.1, independent of the engine, for the tests of
include/zt_bgzf.h.

  write(data, ...)  -> a BGZF file
  walk(file)        -> [Block(offset, size, cdata, crc, isize), ...]
  gzi(file)         -> the .gzi blob by the writer's rule
  voffset(c, u)     -> the virtual offset
"""
import collections
import struct
import zlib

BLOCK_MAX = 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEADER = EOF[:16]  # up to BSIZE

Block = collections.namedtuple("Block", "offset size cdata crc isize")


def block(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, extra_subfields=b"", crc=None, isize=None):
    """One block holding `payload`; extra_subfields go in front of BC."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    cdata = c.compress(payload) + c.flush()
    xlen = 6 + len(extra_subfields)
    size = 12 + xlen + len(cdata) + 8
    assert size <= 65536, size
    head = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255]) + struct.pack("<H", xlen) + extra_subfields
    head += b"BC" + struct.pack("<HH", 2, size - 1)
    return head + cdata + struct.pack("<II", zlib.crc32(payload) if crc is None else crc,
                                      len(payload) if isize is None else isize)


def write(data, block_size=BLOCK_MAX, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, extra_subfields=b"", eof=True):
    data = bytes(data)
    out = [block(data[p:p + block_size], level, strategy, extra_subfields) for p in range(0, len(data), block_size)]
    return b"".join(out) + (EOF if eof else b"")


def walk(f):
    """Every block of the file: the BSIZE chain, with the BC subfield looked up
    among the extra subfields.  Raises ValueError where the chain breaks."""
    f = bytes(f)
    out, at = [], 0
    while at < len(f):
        if len(f) - at < 12 or f[at:at + 4] != b"\x1f\x8b\x08\x04":
            raise ValueError(f"not a BGZF block at {at}")
        xlen, = struct.unpack_from("<H", f, at + 10)
        sub, bsize = 0, None
        while sub + 4 <= xlen:
            si, slen = f[at + 12 + sub:at + 14 + sub], struct.unpack_from("<H", f, at + 14 + sub)[0]
            if si == b"BC" and slen == 2 and bsize is None:
                bsize, = struct.unpack_from("<H", f, at + 16 + sub)
            sub += 4 + slen
        if bsize is None or at + bsize + 1 > len(f) or bsize + 1 < 12 + xlen + 10:
            raise ValueError(f"not a BGZF block at {at}")
        size = bsize + 1
        crc, isize = struct.unpack_from("<II", f, at + size - 8)
        out.append(Block(at, size, f[at + 12 + xlen:at + size - 8], crc, isize))
        at += size
    return out


def gzi_pairs(f):
    """(compressed offset, uncompressed offset) of every block with ISIZE > 0
    after the first such block."""
    pairs, u, first = [], 0, True
    for b in walk(f):
        if b.isize:
            if not first:
                pairs.append((b.offset, u))
            first = False
        u += b.isize
    return pairs


def gzi_blob(pairs):
    return struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", c, u) for c, u in pairs)


def gzi(f):
    return gzi_blob(gzi_pairs(f))


def voffset(coffset, uoffset):
    return (coffset << 16) | uoffset


def touched(f, ranges):
    """The distinct data blocks the (clamped) byte ranges touch: their count and
    the sum of their sizes."""
    blocks = walk(f)
    total = sum(b.isize for b in blocks)
    hit = set()
    for off, ln in ranges:
        if off > total:
            continue
        end = min(total, off + ln)
        if end <= off:
            continue
        u = 0
        for b in blocks:
            if b.isize and u < end and u + b.isize > off:
                hit.add(b.offset)
            u += b.isize
    return len(hit), sum(b.size for b in blocks if b.offset in hit)
