"""Inputs of the deflate block audit (tests/test_gpu_deflate_audit.py), shared
with the CPU tests that check the reference against zlib on the same bytes.
Every input is at most 128 KiB and built once."""
import functools
import random

from deflate_builder import LEN_BASE

BLOCK = 32 << 10
ORACLE_N = (96 << 10) + 13


@functools.lru_cache(maxsize=None)
def dense_input():
    """Three 32 KiB blocks that use every literal, most distances and all 29
    length symbols, and still compress (zlib level 6: ratio 0.44): 15 KiB of
    bytes drawn with weight 1 / (1 + v), every byte value once, then copies
    of earlier spans of the block whose lengths sit on the length codes'
    bases (or one above), each followed by one random byte."""
    rng = random.Random(274)
    weights = [1.0 / (1 + v) for v in range(256)]
    out = bytearray()
    for _ in range(3):
        blk = bytearray(rng.choices(range(256), weights, k=15 << 10))
        every = list(range(256))
        rng.shuffle(every)
        blk += bytes(every)
        while len(blk) < BLOCK:
            n = min(258, rng.choice(LEN_BASE) + (rng.random() < 0.3))
            p = rng.randrange(len(blk) - n)
            blk += blk[p:p + n]
            blk.append(rng.randrange(256))
        out += blk[:BLOCK]
    return bytes(out)


@functools.lru_cache(maxsize=None)
def oracle_input(kind):
    """`wordsalad` / `structured` of the oracle's generators, 96 KiB + 13."""
    import zt_oracle

    return zt_oracle.Oracle().gen(kind, 1, ORACLE_N)


@functools.lru_cache(maxsize=None)
def no_match_input():
    """200 bytes over 16 values in which no three-byte sequence occurs twice:
    nothing to match, so the distance histogram stays empty."""
    rng = random.Random(200)
    out, seen = bytearray(), set()
    while len(out) < 200:
        c = 65 + rng.randrange(16)
        tri = bytes(out[-2:]) + bytes([c])
        if len(tri) == 3 and tri in seen:
            continue
        seen.add(tri)
        out.append(c)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def seven_bit_input():
    return bytes(b & 0x7F for b in random.Random(5).randbytes((64 << 10) + 3))


def period5_input():
    return (b"\x01\x7fab\xf0" * ((48 << 10) // 5 + 1))[:(48 << 10) + 1]


def zeros_input():
    return bytes((64 << 10) + 5)
