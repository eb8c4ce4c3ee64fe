"""Preset dictionaries (include/zt_dict.h) on the GPU: raw DEFLATE streams with
a dictionary in their history and zlib streams with FDICT, against Python's
zlib with `zdict` (the independent reference: the project this engine was
modelled on has no dictionary support, so there are no goldens)."""
import json
import os
import random
import subprocess
import sys
import zlib

import pytest

import dict_corpus

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICT_LENS = [1, 3, 257, 4095, 4096, 4097, 28352, 28353, 32768, 40000]
MSG_LENS = [1, 2, 258, 4097, 32768, 32769, 100000]


@pytest.fixture(scope="module")
def zt():
    import ztamd

    return ztamd


_TEXT = b"".join(dict_corpus.records(1, 200))  # > 40000 bytes of records
_OTHER = b"".join(dict_corpus.records(5, 400))


def make_dict(n):
    return _TEXT[:n]


def make_msg(n, d, seed):
    """n bytes: slices of the dictionary (its first and last bytes included),
    record text the dictionary does not hold, and a few random bytes."""
    rng = random.Random(seed * 1000003 + n)
    out = bytearray(d[:64])  # the dictionary's first bytes: the farthest sources
    out += d[-64:]
    while len(out) < n:
        k = rng.randrange(4)
        ln = rng.randint(3, 400)
        if k <= 1:
            a = rng.randrange(len(d))
            out += d[a:a + ln]
        elif k == 2:
            a = rng.randrange(len(_OTHER))
            out += _OTHER[a:a + ln]
        else:
            out += bytes(rng.getrandbits(8) for _ in range(rng.randint(1, 24)))
    return bytes(out[:n])


def z_inflate_raw(stream, d):
    o = zlib.decompressobj(-15, zdict=d)
    out = o.decompress(stream)
    assert o.eof and o.unused_data == b""
    return out


def z_deflate_raw(msg, d):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=d)
    return c.compress(msg) + c.flush()


def z_deflate_fdict(msg, d):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, zdict=d)
    return c.compress(msg) + c.flush()


def far_match_stream(length=200):
    """One final fixed-Huffman block holding a single match of `length`
    (195..226) at distance 32768, the farthest RFC 1951 allows (zlib itself
    never writes distances above 32506)."""
    bits = []

    def put(v, n, msb):
        for k in (range(n - 1, -1, -1) if msb else range(n)):
            bits.append((v >> k) & 1)

    put(1, 1, False)  # BFINAL
    put(1, 2, False)  # BTYPE = fixed
    put(0b11000000 + (283 - 280), 8, True)  # length symbol 283: 195..226, 5 extra bits
    put(length - 195, 5, False)
    put(29, 5, True)  # distance symbol 29: 24577..32768, 13 extra bits
    put(32768 - 24577, 13, False)
    put(0, 7, True)  # end of block
    bits += [0] * (-len(bits) % 8)
    return bytes(sum(b << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))


def mixed_batch(d, seed):
    """65 items of mixed lengths, several of them longer than one 32 KiB block"""
    rng = random.Random(seed)
    lens = list(MSG_LENS) + [rng.choice([1, 7, 300, 350, 4096, 5000, 32768, 40000, 70000]) for _ in range(58)]
    return [make_msg(n, d, 100 + i) for i, n in enumerate(lens)]


# ---- 1. deflate with a dictionary, decoded by zlib ---------------------------------
@pytest.mark.parametrize("dlen", DICT_LENS)
def test_deflate_dict_single(zt, dlen):
    d = make_dict(dlen)
    for n in MSG_LENS:
        msg = make_msg(n, d, 1)
        s = zt.deflate_raw(msg, dictionary=d)
        assert z_inflate_raw(s, d) == msg, (dlen, n)


@pytest.mark.parametrize("dlen", DICT_LENS)
def test_deflate_dict_batch(zt, dlen):
    d = make_dict(dlen)
    items = mixed_batch(d, dlen)
    assert len(items) == 65
    outs = zt.deflate_raw_batch(items, dictionary=d)
    for i, (msg, s) in enumerate(zip(items, outs)):
        assert z_inflate_raw(s, d) == msg, (dlen, i, len(msg))
    # a stream does not depend on its neighbours in the batch
    assert zt.deflate_raw(items[9], dictionary=d) == outs[9]
    assert zt.deflate_raw(items[5], dictionary=d) == outs[5]  # (32 769 bytes: two blocks)


def test_deflate_dict_uses_far_bytes(zt):
    """The first usable dictionary byte is a match source: a message that is
    the dictionary's tail of exactly the encoder's reach compresses to matches."""
    d = make_dict(28352)
    rng = random.Random(11)
    d = bytes(rng.getrandbits(8) for _ in range(512)) + d[512:]  # (random: no nearer copy of these bytes)
    msg = d[:512]
    s = zt.deflate_raw(msg, dictionary=d)
    assert z_inflate_raw(s, d) == msg
    assert len(s) < 64, len(s)


# ---- 2. padding and neighbour poison ------------------------------------------------
@pytest.mark.parametrize("fill", [0x00, 0xFF, 0xAA])
def test_one_byte_dictionary_padding(zt, fill):
    """A one-byte dictionary leaves 4095 bytes of padding in front of it in the
    match kernel's history: a match into the padding makes zlib fail or
    return other bytes."""
    d = b"\x01"
    msg = bytes([fill]) * 5000
    s = zt.deflate_raw(msg, dictionary=d)
    assert z_inflate_raw(s, d) == msg
    outs = zt.deflate_raw_batch([msg, b"\x01" * 5000, msg], dictionary=d)
    for m, o in zip([msg, b"\x01" * 5000, msg], outs):
        assert z_inflate_raw(o, d) == m


def test_neighbour_poison(zt):
    """Every message starts with the last 300 bytes of the previous one: a
    match that reached into the neighbour (the bytes in front of the stream in
    the packed batch) would decode wrongly against the 1000-byte dictionary."""
    d = make_dict(1000)
    rng = random.Random(21)
    items = []
    prev = bytes(rng.getrandbits(8) for _ in range(300))
    for i in range(48):
        n = rng.choice([350, 4096, 32768, 33000, 1000])
        body = bytes(rng.getrandbits(8) for _ in range(200)) + make_msg(n, d, 300 + i)
        m = prev + body
        items.append(m)
        prev = m[-300:]
    outs = zt.deflate_raw_batch(items, dictionary=d)
    for i, (m, s) in enumerate(zip(items, outs)):
        assert z_inflate_raw(s, d) == m, i


# ---- 3. classify: the dictionary counts as history ----------------------------------
def test_classify_counts_dictionary(zt):
    rng = random.Random(31)
    d = bytes(rng.getrandbits(8) for _ in range(16384))
    msg = d[4000:12192]
    s = zt.deflate_raw(msg, dictionary=d)
    assert z_inflate_raw(s, d) == msg
    assert len(s) < len(msg) // 4, len(s)  # (stored: len + 5; 258-byte matches: ~130 bytes)
    items = [d[64 * k:64 * k + 8192] for k in range(64)]
    outs = zt.deflate_raw_batch(items, dictionary=d)
    for m, o in zip(items, outs):
        assert z_inflate_raw(o, d) == m
        assert len(o) < len(m) // 4, len(o)


# ---- 4. the dictionary helps --------------------------------------------------------
# measured ratio of the GPU total to zlib level 6 with the same zdict on this
# corpus: profiles/dict_time.json, "corpus_ratio_to_zlib6" (373 972 bytes
# against zlib's 334 180; without a dictionary 1 007 390 against 984 941).
# The output is deterministic: the margin below only absorbs later tuning.
RATIO_TO_ZLIB6 = 1.1191


def test_dictionary_helps(zt):
    d = dict_corpus.dictionary()
    msgs = dict_corpus.messages()
    plain = sum(len(s) for s in zt.deflate_raw_batch(msgs))
    outs = zt.deflate_raw_batch(msgs, dictionary=d)
    with_d = sum(len(s) for s in outs)
    for m, s in zip(msgs[::37], outs[::37]):
        assert z_inflate_raw(s, d) == m
    ref = sum(len(z_deflate_raw(m, d)) for m in msgs)
    print(f"dict corpus: plain {plain} with dictionary {with_d} zlib6+zdict {ref} ratio {with_d / ref:.4f}")
    assert with_d <= 0.5 * plain, (with_d, plain)
    assert with_d / ref <= RATIO_TO_ZLIB6 + 0.01, (with_d, ref)


# ---- 5. inflate of streams zlib wrote -----------------------------------------------
@pytest.mark.parametrize("dlen", DICT_LENS)
def test_inflate_zlib_streams(zt, dlen):
    d = make_dict(dlen)
    for n in MSG_LENS:
        msg = make_msg(n, d, 2)
        raw = z_deflate_raw(msg, d)
        out, ip = zt.inflate_raw(raw, dictionary=d)
        assert out == msg and ip == len(raw), (dlen, n)
        out, ip = zt.inflate_raw(b"\x55\xAA\x00" + raw + b"tail", index=3, dictionary=d)
        assert out == msg and ip == 3 + len(raw), (dlen, n)
        fd = z_deflate_fdict(msg, d)
        assert fd[1] & 0x20
        out, ip = zt.zlib_decompress(fd, verify=True, dictionary=d)
        assert out == msg and ip == len(fd) - 4, (dlen, n)


def test_inflate_batch_corpus(zt):
    d = dict_corpus.dictionary()
    msgs = dict_corpus.messages()
    streams = [z_deflate_raw(m, d) for m in msgs]
    res = zt.inflate_raw_batch(streams, dictionary=d)
    assert len(res) == 4096
    for (st, out, ip), m, s in zip(res, msgs, streams):
        assert st == 0 and out == m and ip == len(s)


def test_inflate_batch_mixed_status(zt):
    """per-item status: a stream that reaches before the dictionary fails alone"""
    d = make_dict(4097)
    long_d = make_dict(40000)
    items = mixed_batch(d, 7)[:12]
    streams = [z_deflate_raw(m, d) for m in items]
    bad = far_match_stream()  # distance 32768 > 4097
    assert z_inflate_raw(bad, long_d) == long_d[7232:7432]
    streams.insert(5, bad)
    res = zt.inflate_raw_batch(streams, dictionary=d)
    for k, (st, out, ip) in enumerate(res):
        if k == 5:
            assert st == -15
        else:
            m = items[k if k < 5 else k - 1]
            assert st == 0 and out == m and ip == len(streams[k])


def test_inflate_distance_32768(zt):
    """zlib uses the last 32768 bytes of a 40000-byte dictionary: the message
    repeats the first 200 of them, a distance of (nearly) 32768."""
    d = make_dict(40000)
    rng = random.Random(41)
    d = d[:7232] + bytes(rng.getrandbits(8) for _ in range(200)) + d[7432:]
    msg = d[7232:7432]
    for m in (msg, msg + d[7500:7800] + msg):
        raw = z_deflate_raw(m, d)  # (zlib's own far matches: up to 32506 back)
        out, ip = zt.inflate_raw(raw, dictionary=d)
        assert out == m and ip == len(raw)
    raw = far_match_stream()  # exactly 32768 back
    assert z_inflate_raw(raw, d) == msg
    out, ip = zt.inflate_raw(raw, dictionary=d)
    assert out == msg and ip == len(raw)
    res = zt.inflate_raw_batch([raw] * 3, dictionary=d)
    assert all(st == 0 and o == msg and ip == len(raw) for st, o, ip in res)
    # one byte further back is before the window: with the window cut by one
    # byte the same stream reaches before the dictionary
    with pytest.raises(zt.ZtError) as e:
        zt.inflate_raw(raw, dictionary=d[7233:])
    assert e.value.code == -15


# ---- 6. errors ----------------------------------------------------------------------
def test_errors(zt):
    d = dict_corpus.dictionary()
    msg = dict_corpus.messages(8)[3]
    fd = z_deflate_fdict(msg, d)
    wrong = bytes([d[0] ^ 1]) + d[1:]
    with pytest.raises(zt.ZtError) as e:
        zt.zlib_decompress(fd, dictionary=wrong)
    assert e.value.code == -44
    assert e.value.msg == "invalid dictionary id: 0x%x / 0x%x" % (zlib.adler32(d), zlib.adler32(wrong))
    # the old entry point, and the new one without a dictionary: unchanged
    with pytest.raises(zt.ZtError) as e:
        zt.zlib_decompress(fd)
    assert e.value.code == -42 and e.value.msg == "fdict flag is not supported"
    with pytest.raises(zt.ZtError) as e:
        zt.zlib_decompress(fd, dictionary=b"")
    assert e.value.code == -42 and e.value.msg == "fdict flag is not supported"
    # a raw stream without its dictionary
    raw = z_deflate_raw(msg, d)
    with pytest.raises(zt.ZtError) as e:
        zt.inflate_raw(raw)
    assert e.value.code == -15
    # FDICT clear: the dictionary is ignored
    plain = zlib.compress(msg, 6)
    assert zt.zlib_decompress(plain, verify=True, dictionary=d) == zt.zlib_decompress(plain, verify=True)


def test_empty_dictionary_is_plain_call(zt):
    msgs = dict_corpus.messages(64) + [make_msg(100000, make_dict(4096), 3), b""]
    for m in msgs[-3:]:
        assert zt.deflate_raw(m, dictionary=b"") == zt.deflate_raw(m)
        assert zt.zlib_compress(m, dictionary=b"") == zt.zlib_compress(m)
        s = zt.deflate_raw(m)
        assert zt.inflate_raw(s, dictionary=b"") == zt.inflate_raw(s)
    assert zt.deflate_raw_batch(msgs, dictionary=b"") == zt.deflate_raw_batch(msgs)
    assert zt.zlib_compress_batch(msgs, dictionary=b"") == zt.zlib_compress_batch(msgs)
    streams = zt.deflate_raw_batch(msgs)
    assert zt.inflate_raw_batch(streams, dictionary=b"") == zt.inflate_raw_batch(streams)


# ---- 7. container round trip --------------------------------------------------------
@pytest.mark.parametrize("dlen", [1, 4097, 40000])
def test_zlib_container_round_trip(zt, dlen):
    d = make_dict(dlen)
    items = [b"", b"x"] + [make_msg(n, d, 4) for n in (350, 32769, 100000)]
    members = zt.zlib_compress_batch(items, dictionary=d)
    for m, s in zip(items, members):
        single, adler = zt.zlib_compress(m, dictionary=d)
        assert single == s and adler == zlib.adler32(m)
        assert s[0] == 0x78 and s[1] & 0x20 and (s[0] * 256 + s[1]) % 31 == 0
        assert s[1] >> 6 == 2  # FLEVEL as zlib_compress writes it (the compression type)
        assert s[2:6] == zlib.adler32(d).to_bytes(4, "big")
        o = zlib.decompressobj(zdict=d)
        assert o.decompress(s) == m and o.eof and o.unused_data == b""
        out, ip = zt.zlib_decompress(s, verify=True, dictionary=d)
        assert out == m and ip == len(s) - 4
    for m in items:
        fd = z_deflate_fdict(m, d)
        out, ip = zt.zlib_decompress(fd, verify=True, dictionary=d)
        assert out == m and ip == len(fd) - 4


# ---- 8. two logical devices ---------------------------------------------------------
def test_alias_devices_dict():
    """zt_set_devices with a dictionary batch on two logical devices of this
    one GPU (ZT_ALIAS_DEVICES, tests/alias_dict_child.py): the same outputs as
    one device, each device with its own copy of the dictionary."""
    env = dict(os.environ, ZT_ALIAS_DEVICES="2")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "alias_dict_child.py")], env=env,
                       capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res == {"logical_devices": 2, "deflate_equal": True, "zlib_equal": True, "inflate_equal": True,
                   "zlib_ok": True}, res
