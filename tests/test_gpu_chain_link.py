"""The match kernel's serial link (csrc/deflate.hip: link_range): whole groups
of steps without bounds selects and the progress word stored behind the
group's link stores without a drain must give the links of the former link
(ZT_DF_LINK=0), so the streams are byte-equal at
every level and in both chain-head formats, and inflate back to the input.

The inputs are the smallest at which the link can go wrong: lengths 8 KiB + r
(a ragged last group, a ragged last step, a range shorter than a step);
64 KiB + r with the default grouping (the second one-block workgroup primes
28 KiB of history); 160 KiB + 511 in a four-block workgroup (ZT_DF_SUPER_MIN=4:
the ring wraps and the head format changes); a dictionary batch
(match_dict_kernel: the links start at the dictionary's floor)."""
import contextlib
import os
import random
import zlib

import pytest

pytestmark = pytest.mark.gpu

KIB = 1024
RAGGED = [1, 63, 64, 65, 511, 513]
# (size, ZT_DF_SUPER_MIN)
SIZES = ([(8 * KIB + r, None) for r in RAGGED] + [(64 * KIB + r, None) for r in RAGGED] + [(160 * KIB + 511, 4)])
NMAX = max(n for n, _ in SIZES)
LEVELS = [1, 6, 9]
HEADS = [None, 16, 32]
DATA = ["wordsalad", "structured", "one_byte", "period3", "period64", "text_then_random"]
HOOKS = ("ZT_DF_LINK", "ZT_DF_HEADS", "ZT_DF_SUPER_MIN")


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
        zt.synth_dev(kind, 11, d.data_ptr(), NMAX)
        torch.cuda.synchronize()
        return d.cpu().numpy().tobytes()

    ws, st = synth("wordsalad"), synth("structured")
    # every 8 KiB: 3 KiB of text, then 5 KiB of random bytes -- the text keeps
    # the blocks below classify_kernel's stored-block verdict, so they are searched
    rnd = random.Random(5)
    mixed = b"".join(ws[i:i + 3 * KIB] + bytes(rnd.getrandbits(8) for _ in range(5 * KIB))
                     for i in range(0, NMAX, 8 * KIB))[:NMAX]
    return {
        "wordsalad": ws,
        "structured": st,
        "one_byte": b"\x41" * NMAX,  # every lane of a step in one bucket: lane order decides
        "period3": (b"\x00\xfe\x37" * (NMAX // 3 + 1))[:NMAX],
        "period64": (bytes(range(100, 164)) * (NMAX // 64 + 1))[:NMAX],
        "text_then_random": mixed,
    }


@contextlib.contextmanager
def hooks(link=None, heads=None, super_min=None):
    """ZT_DF_LINK, ZT_DF_HEADS and ZT_DF_SUPER_MIN for the calls inside (None: unset)."""
    old = {k: os.environ.pop(k, None) for k in HOOKS}
    for k, v in zip(HOOKS, (link, heads, super_min)):
        if v is not None:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k in HOOKS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


@pytest.mark.parametrize("n,super_min", SIZES)
@pytest.mark.parametrize("kind", DATA)
def test_streams_do_not_depend_on_the_link(zt, corpora, kind, n, super_min):
    data = corpora[kind][:n]
    for level in LEVELS:
        for heads in HEADS:
            with hooks(0, heads, super_min):
                former = zt.deflate_raw(data, level=level)
            with hooks(None, heads, super_min):
                new = zt.deflate_raw(data, level=level)
            assert new == former, f"level {level}, ZT_DF_HEADS {heads}: the link changed the stream"
            assert zlib.decompress(new, -15) == data


def test_dictionary_batch_streams_do_not_depend_on_the_link(zt, corpora):
    d = corpora["wordsalad"][40 * KIB:40 * KIB + 5000]
    st = corpora["structured"]
    items = [st[:8 * KIB + 65], corpora["wordsalad"][:12 * KIB + 511]]
    for level in LEVELS:
        for heads in HEADS:
            with hooks(0, heads):
                former = zt.deflate_raw_batch(items, level=level, dictionary=d)
            with hooks(None, heads):
                new = zt.deflate_raw_batch(items, level=level, dictionary=d)
            assert new == former, f"level {level}, ZT_DF_HEADS {heads}: the link changed a stream"
            for stream, item in zip(new, items):
                o = zlib.decompressobj(-15, zdict=d)
                assert o.decompress(stream) + o.flush() == item
