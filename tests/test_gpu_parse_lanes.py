"""The deflate parse's two walks (csrc/deflate_post.hip): lane-parallel steps of
2048 positions (parse_block_lanes, the default) and the serial walk over
64-position windows (parse_block_regs, ZT_PARSE_SERIAL=1).  Both emit the
same tokens in the same order and count the same histograms, in parse_kernel
and in price_kernel, so the streams are byte-identical."""
import contextlib
import os
import random
import zlib

import pytest

pytestmark = pytest.mark.gpu

KIB = 1024
# edges of a lane (32 positions), a step (2048), a block (32 KiB) and a
# segment (1 MiB)
SIZES = [1, 31, 33, 2047, 2049, 32768, 32769, 12 * KIB + 5, 96 * KIB + 13, 1024 * KIB + 4 * KIB + 7]
# level, compression_type: greedy; the DP's path (levels 6 and 9); fixed codes
# only, where the DP is off and the one-step lazy rule runs
MODES = [(1, 2), (6, 2), (9, 2), (6, 1)]
DATA = ["wordsalad", "structured", "zeros", "period7", "period5", "random7bit", "random_then_wordsalad"]
NMAX = max(SIZES)


@pytest.fixture(scope="module")
def zt():
    import ztamd

    return ztamd


@pytest.fixture(scope="module")
def corpora(zt):
    """NMAX bytes per data set, made once; the cases take prefixes."""
    import torch

    def synth(kind):
        d = torch.empty(NMAX, dtype=torch.uint8, device="cuda")
        zt.synth_dev(kind, 7, d.data_ptr(), NMAX)
        torch.cuda.synchronize()
        return d.cpu().numpy().tobytes()

    ws = synth("wordsalad")
    return {
        "wordsalad": ws,
        "structured": synth("structured"),
        # 258-byte matches that skip whole lanes and never join the path a lane guessed
        "zeros": bytes(NMAX),
        # 258-byte matches at a phase that drifts through the lanes
        "period7": (b"\x03abc\xf1\x80z" * (NMAX // 7 + 1))[:NMAX],
        "period5": (b"\x01\x7fab\xf0" * (NMAX // 5 + 1))[:NMAX],
        # searched (7-bit bytes pass the classifier), nearly every position a literal
        "random7bit": bytes(b & 0x7F for b in random.Random(5).randbytes(NMAX)),
        "random_then_wordsalad": random.Random(3).randbytes(8 * KIB) + ws[:NMAX - 8 * KIB],
    }


@contextlib.contextmanager
def parse_serial(on):
    """ZT_PARSE_SERIAL for the calls inside (False: unset, the default walk)."""
    old = os.environ.pop("ZT_PARSE_SERIAL", None)
    if on:
        os.environ["ZT_PARSE_SERIAL"] = "1"
    try:
        yield
    finally:
        os.environ.pop("ZT_PARSE_SERIAL", None)
        if old is not None:
            os.environ["ZT_PARSE_SERIAL"] = old


@pytest.mark.parametrize("level,ctype", MODES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", DATA)
def test_streams_do_not_depend_on_the_walk(zt, corpora, kind, n, level, ctype):
    data = corpora[kind][:n]
    with parse_serial(True):
        serial = zt.deflate_raw(data, compression_type=ctype, level=level)
    with parse_serial(False):
        lanes = zt.deflate_raw(data, compression_type=ctype, level=level)
    assert lanes == serial, "the lane-parallel walk changed the stream"
    assert zlib.decompress(lanes, -15) == data


def test_batch_streams_do_not_depend_on_the_walk(zt, corpora):
    ws, st = corpora["wordsalad"], corpora["structured"]
    items = [ws[:40 * KIB + 3], st[:2049], bytes(70 * KIB + 1), ws[100000:100000 + 31]]
    with parse_serial(True):
        serial = zt.deflate_raw_batch(items, level=6)
    with parse_serial(False):
        lanes = zt.deflate_raw_batch(items, level=6)
    assert lanes == serial
    for stream, item in zip(lanes, items):
        assert zlib.decompress(stream, -15) == item


def test_dictionary_batch_streams_do_not_depend_on_the_walk(zt, corpora):
    ws = corpora["wordsalad"]
    d = ws[:20000]
    items = [ws[20000:20000 + 40 * KIB + 3], ws[100000:100000 + 70 * KIB + 1]]
    with parse_serial(True):
        serial = zt.deflate_raw_batch(items, level=6, dictionary=d)
    with parse_serial(False):
        lanes = zt.deflate_raw_batch(items, level=6, dictionary=d)
    assert lanes == serial
    for stream, item in zip(lanes, items):
        o = zlib.decompressobj(-15, zdict=d)
        assert o.decompress(stream) + o.flush() == item
