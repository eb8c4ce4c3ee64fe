"""The corpus of the indexed range tests (tests/test_gpu_index.py,
tests/test_js_index.py): 2.5 MiB + 5 bytes of wordsalad with 96 KiB of
xorshift32 centred on the 1 MiB mark (stored blocks straddle the first
restart point), 96 KiB of zeros centred on the 2 MiB mark (258-byte matches
straddle the second) and structured data at the end: three segments and a
ragged last unit."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
TOTAL = 5 * (MIB // 2) + 5


def corpus(oracle):
    d = bytearray(oracle.gen("wordsalad", 11, TOTAL))
    half = 48 << 10
    d[MIB - half:MIB + half] = oracle.gen("xorshift32", 12, 2 * half)
    d[2 * MIB - half:2 * MIB + half] = bytes(2 * half)
    tail = oracle.gen("structured", 13, 150000)
    d[TOTAL - len(tail):] = tail
    assert len(d) == TOTAL
    return bytes(d)


def restart_spacing():
    """bytes between restart markers, from the code (zt_internal.h)"""
    src = open(os.path.join(ROOT, "zlib.ts_amd", "csrc", "zt_internal.h")).read()
    m = re.search(r"kRestartBlocks = \(1u << (\d+)\) / DF_BLOCK", src)
    return 1 << int(m.group(1))
