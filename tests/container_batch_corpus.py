"""Inputs of the container batch tests (tests/test_gpu_container_batch.py, its
alias-device child and tests/test_js_container_batch.py): hand-framed gzip
members and the deterministic item lists.  Python's zlib writes the DEFLATE
bodies.  Test infrastructure only."""
import hashlib
import random
import zlib


def raw_deflate(data, level=6, zdict=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, zdict=zdict) if zdict else zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def frame(data, extra=None, name=None, comment=None, level=6, mtime=0, flg_or=0, cm=8):
    """One RFC 1952 member framed by hand (no FHCRC)."""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | flg_or
    h = bytes([0x1F, 0x8B, cm, flg]) + mtime.to_bytes(4, "little") + bytes([0, 3])
    if extra is not None:
        h += len(extra).to_bytes(2, "little") + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    return h + raw_deflate(data, level) + zlib.crc32(data).to_bytes(4, "little") + (len(data) & 0xFFFFFFFF).to_bytes(4, "little")


def gzip_member(data, level=6):
    """As gzip.compress(data, level, mtime=0) (a 10-byte header)."""
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def data_of(oracle, k, n):
    return oracle.gen(("wordsalad", "xorshift32", "structured")[k % 3], 1000 + k, n)


def alias_items(oracle, count=256):
    """(gzip items, zlib items, their data): `count` of each, 1 - 64 KiB;
    every eighth gzip item has three members."""
    rng = random.Random(11)
    gz, zl, datas = [], [], []
    for k in range(count):
        d = data_of(oracle, k, rng.randint(1 << 10, 64 << 10))
        datas.append(d)
        if k % 8 == 7:
            cut = [0, len(d) // 3, len(d) // 2, len(d)]
            gz.append(b"".join(frame(d[cut[j]:cut[j + 1]], name=b"part%d" % j, level=1 + k % 9) for j in range(3)))
        else:
            gz.append(gzip_member(d, 1 + k % 9))
        zl.append(zlib.compress(d, k % 10))
    return gz, zl, datas


def results_digest(results):
    """sha256 over every item's status, output and member fields, in order."""
    h = hashlib.sha256()
    for r in results:
        h.update(repr(int(r[0])).encode())
        h.update(b"-" if r[1] is None else len(r[1]).to_bytes(8, "little") + r[1])
        for x in r[2:]:
            if isinstance(x, list):  # members
                for m in x:
                    h.update(repr(sorted((k, v) for k, v in m.items() if k != "data")).encode())
            else:
                h.update(repr(x).encode())
    return h.hexdigest()
