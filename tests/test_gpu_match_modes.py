"""The deflate match kernel's two ways of measuring candidates (at once, or
through the waves' queues, chosen per block from the block's probe sub-chunk;
csrc/deflate.hip, ZT_DF_MQ): both find the same matches, so the streams are
byte-identical whatever the threshold, and the engagement counter
(zt_debug_match_modes) shows which way the blocks went."""
import contextlib
import os
import random
import zlib

import pytest

pytestmark = pytest.mark.gpu

KIB = 1024
# one block with a probe, one whole queued sub-chunk and a ragged last one
# (lanes past the end stay in the queued loop); three blocks, each with its
# own decision; a second workgroup that starts with history; a restart point
SIZES = [12 * KIB + 5, 96 * KIB + 13, 160 * KIB + 1, 1024 * KIB + 4 * KIB + 7]
LEVELS = [1, 6, 9]
DATA = ["wordsalad", "structured", "zeros", "period5", "random_then_wordsalad"]
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
        # 258-byte matches at distance 1: the nice_len clamp and the exact-length path
        "zeros": bytes(NMAX),
        # many candidates of equal length: the nearest must win
        "period5": (b"\x01\x7fab\xf0" * (NMAX // 5 + 1))[:NMAX],
        # a block that starts with incompressible bytes before searched text
        "random_then_wordsalad": random.Random(3).randbytes(8 * KIB) + ws[:NMAX - 8 * KIB],
        "random": random.Random(4).randbytes(96 * KIB + 13),
    }


@contextlib.contextmanager
def mq(setting):
    """ZT_DF_MQ for the calls inside (None: the level's default)."""
    old = os.environ.pop("ZT_DF_MQ", None)
    if setting is not None:
        os.environ["ZT_DF_MQ"] = str(setting)
    try:
        yield
    finally:
        os.environ.pop("ZT_DF_MQ", None)
        if old is not None:
            os.environ["ZT_DF_MQ"] = old


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", DATA)
def test_streams_do_not_depend_on_the_mode(zt, corpora, kind, n, level):
    data = corpora[kind][:n]
    streams = []
    for setting in (0, 1, None):
        with mq(setting):
            streams.append(zt.deflate_raw(data, level=level))
    assert streams[1] == streams[0], "queued measurement changed the stream"
    assert streams[2] == streams[0], "the default threshold changed the stream"
    assert zlib.decompress(streams[0], -15) == data


def test_dictionary_batch_streams_do_not_depend_on_the_mode(zt, corpora):
    ws = corpora["wordsalad"]
    d = ws[:20000]
    items = [ws[20000:20000 + 40 * KIB + 3], ws[100000:100000 + 70 * KIB + 1]]
    outs = []
    for setting in (0, 1, None):
        with mq(setting):
            outs.append(zt.deflate_raw_batch(items, level=6, dictionary=d))
    assert outs[1] == outs[0]
    assert outs[2] == outs[0]
    for stream, item in zip(outs[0], items):
        o = zlib.decompressobj(-15, zdict=d)
        assert o.decompress(stream) + o.flush() == item


def modes_of(zt, data, setting, level=6):
    zt.debug_match_modes()  # (clears)
    with mq(setting):
        zt.deflate_raw(data, level=level)
    return zt.debug_match_modes()


def test_engagement(zt, corpora):
    ws = corpora["wordsalad"][:96 * KIB + 13]
    queued, at_once = modes_of(zt, ws, 1)
    assert queued >= 1
    queued, at_once = modes_of(zt, ws, 0)
    assert queued == 0 and at_once >= 1
    # the level-6 default: text queues, incompressible bytes do not
    queued, _ = modes_of(zt, ws, None)
    assert queued >= 1
    queued, _ = modes_of(zt, corpora["random"], None)
    assert queued == 0
