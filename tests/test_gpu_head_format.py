"""The deflate match kernel's two chain-head formats (u32 while a workgroup's
blocks measure their candidates at once, u16 while they measure through the
waves' queues, changed in place between blocks; csrc/deflate.hip,
ZT_DF_HEADS): both formats and every change between them give the same links,
so the streams are byte-identical whatever the format, and the counter
(zt_debug_head_formats) shows that the changes ran.

A workgroup takes more than one block only on inputs of many MiB; the cases
run with the default geometry (one block per workgroup at these sizes: a
change to u16 at most) and with ZT_DF_SUPER_MIN=4 (four blocks per workgroup,
as on large inputs: changes in both directions inside one workgroup).

Measured on the `alternating` data set, a wordsalad block behind 28 KiB of
structured history measures between 1536 and 2048 candidates per 4096
positions of its probe: below level 6's threshold of 2048, so its verdicts
alternate only with ZT_DF_MQ lowered (1024 here).  `alternating64` changes
the source every two blocks: the second wordsalad block of a pair has
wordsalad history and queues at the default threshold."""
import contextlib
import os
import zlib

import pytest

pytestmark = pytest.mark.gpu

KIB = 1024
# two blocks, one change; a whole super-chunk of four blocks, both directions,
# across a sweep; a second workgroup that primes 28 KiB of history in u32; a
# restart point, then a block
SIZES = [64 * KIB + 5, 128 * KIB + 13, 160 * KIB + 1, 1024 * KIB + 36 * KIB + 7]
LEVELS = [1, 6, 9]
DATA = ["wordsalad", "structured", "alternating", "alternating64", "zeros", "period5"]
GEOMETRY = [None, 4]
NMAX = max(SIZES)
BLOCK = 32 * KIB
HOOKS = ("ZT_DF_HEADS", "ZT_DF_MQ", "ZT_DF_SUPER_MIN")


@pytest.fixture(scope="module")
def zt():
    import ztamd

    return ztamd


@pytest.fixture(scope="module")
def corpora(zt):
    """NMAX bytes per data set, made once; the cases take prefixes."""
    import torch

    def synth(kind):
        d = torch.empty(NMAX + BLOCK, dtype=torch.uint8, device="cuda")
        zt.synth_dev(kind, 7, d.data_ptr(), NMAX + BLOCK)
        torch.cuda.synchronize()
        return d.cpu().numpy().tobytes()

    ws, st = synth("wordsalad"), synth("structured")
    # 32 KiB blocks, wordsalad and structured in turn: every block's verdict
    # differs from the one before.  The last 8 KiB of a block repeat the bytes
    # 24 KiB before them: long matches through chains linked before a change
    def alternating(run):
        blocks = []
        for i in range(NMAX // BLOCK + 1):
            text = (i // run) % 2 == 0
            src = ws if text else st
            b = src[i * BLOCK:i * BLOCK + 24 * KIB]
            b += b[:8 * KIB]
            assert len(b) == BLOCK
            if text:  # (text that compresses: its probe measures candidates)
                assert len(zlib.compress(b[:24 * KIB], 6)) < 12 * KIB
            blocks.append(b)
        return b"".join(blocks)[:NMAX]

    return {
        "wordsalad": ws[:NMAX],
        "structured": st[:NMAX],
        "alternating": alternating(1),
        "alternating64": alternating(2),
        "zeros": bytes(NMAX),
        "period5": (b"\x01\x7fab\xf0" * (NMAX // 5 + 1))[:NMAX],
    }


@contextlib.contextmanager
def hooks(heads=None, mq=None, super_min=None):
    """ZT_DF_HEADS, ZT_DF_MQ and ZT_DF_SUPER_MIN for the calls inside (None: unset)."""
    old = {k: os.environ.pop(k, None) for k in HOOKS}
    for k, v in zip(HOOKS, (heads, mq, super_min)):
        if v is not None:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k in HOOKS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


# (heads, mq): the u16 reference first, u32 throughout, the per-block choice,
# the per-block choice where every block that measured anything queues, and
# at the threshold where `alternating`'s verdicts alternate
SETTINGS = [(16, None), (32, None), (None, None), (None, 1), (None, 1024)]


@pytest.mark.parametrize("super_min", GEOMETRY)
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", DATA)
def test_streams_do_not_depend_on_the_head_format(zt, corpora, kind, n, level, super_min):
    data = corpora[kind][:n]
    streams = []
    for heads, mq in SETTINGS:
        with hooks(heads, mq, super_min):
            streams.append(zt.deflate_raw(data, level=level))
    assert streams[1] == streams[0], "u32 heads changed the stream"
    assert streams[2] == streams[0], "the per-block format changed the stream"
    assert streams[3] == streams[0], "the per-block format with ZT_DF_MQ=1 changed the stream"
    assert streams[4] == streams[0], "the per-block format with ZT_DF_MQ=1024 changed the stream"
    assert zlib.decompress(streams[0], -15) == data


@pytest.mark.parametrize("kind", ["wordsalad", "alternating"])
def test_dictionary_batch_streams_do_not_depend_on_the_head_format(zt, corpora, kind):
    c = corpora[kind]
    d = corpora["wordsalad"][:20000]
    items = [c[32 * KIB:72 * KIB + 3], c[128 * KIB:198 * KIB + 1]]
    outs = []
    for heads, mq in SETTINGS:
        with hooks(heads, mq):
            outs.append(zt.deflate_raw_batch(items, level=6, dictionary=d))
    assert outs[1] == outs[0]
    assert outs[2] == outs[0]
    assert outs[3] == outs[0]
    assert outs[4] == outs[0]
    for stream, item in zip(outs[0], items):
        o = zlib.decompressobj(-15, zdict=d)
        assert o.decompress(stream) + o.flush() == item


def formats_of(zt, data, heads=None, level=6, super_min=None, mq=None):
    zt.debug_head_formats()  # (clears)
    with hooks(heads, mq, super_min):
        zt.deflate_raw(data, level=level)
    return zt.debug_head_formats()


def test_engagement(zt, corpora):
    alt = corpora["alternating"][:128 * KIB + 13]
    # four blocks in one workgroup, each verdict unlike the one before
    to16, to32 = formats_of(zt, alt, super_min=4, mq=1024)
    assert to16 >= 1 and to32 >= 1
    # at the default threshold: text, text (queues), structured, structured
    to16, to32 = formats_of(zt, corpora["alternating64"][:128 * KIB + 13], super_min=4)
    assert to16 >= 1 and to32 >= 1
    # one block per workgroup: the heads start as u32 and change once at most
    to16, to32 = formats_of(zt, alt, mq=1024)
    assert to16 >= 1 and to32 == 0
    for super_min in GEOMETRY:
        assert formats_of(zt, corpora["structured"][:128 * KIB + 13], super_min=super_min) == (0, 0)
        assert formats_of(zt, alt, heads=16, super_min=super_min) == (0, 0)
        assert formats_of(zt, alt, heads=32, super_min=super_min) == (0, 0)
        assert formats_of(zt, alt, level=1, super_min=super_min) == (0, 0)
        assert formats_of(zt, alt, level=9, super_min=super_min) == (0, 0)
    to16, to32 = formats_of(zt, corpora["wordsalad"][:96 * KIB + 13])
    assert to16 >= 1 and to32 == 0
