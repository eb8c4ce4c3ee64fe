"""A DEFLATE block parser that keeps what an encoder decided.

An inflate only says that a stream decodes.  `parse` returns, per block, the
header fields as they were read, the code lengths, the tokens and their
histograms, so that a test can hold the encoder's decisions against an
independent computation (tests/huffman_ref.py): code optimality, header
minima, the run-length coding, the choice of block type.

Tokens follow deflate_builder: an int is a literal, (length, distance) a
match, (258, distance, True) a length 258 written as symbol 284 + extra 31.
"""
from deflate_builder import (CL_EXTRA, CL_ORDER, CL_REP0, DIST_BASE, DIST_EXTRA, FIXED_DIST, FIXED_LIT, LEN_BASE,
                             LEN_EXTRA, canonical_codes)


class AuditError(ValueError):
    pass


class Block:
    """One block as read.  Stored: `stored_len`.  Huffman (btype 1 / 2):
    lit_lens / dist_lens (as transmitted: HLIT / HDIST entries), tokens,
    lit_hist[286] (end-of-block included) / dist_hist[30]; dynamic also hlit,
    hdist, hclen, cl_lens[19] (by symbol), cl_syms [(symbol, extra value)] and
    cl_hist[19].  bit_start / bit_end: the block's bits in the stream,
    header_bits: up to the first token.  out: the bytes it produced."""

    def __init__(self, btype, final, bit_start):
        self.btype, self.final, self.bit_start = btype, final, bit_start
        self.bit_end = self.header_bits = None
        self.stored_len = None
        self.hlit = self.hdist = self.hclen = None
        self.cl_lens = self.cl_syms = self.cl_hist = None
        self.lit_lens = self.dist_lens = None
        self.tokens, self.lit_hist, self.dist_hist = [], [0] * 286, [0] * 30
        self.out = b""

    @property
    def used_lit(self):
        return sum(1 for f in self.lit_hist if f)


class _Bits:
    def __init__(self, data):
        self.d, self.p, self.end = bytes(data), 0, 8 * len(data)

    def take(self, n):
        if self.p + n > self.end:
            raise AuditError("stream ends inside a block")
        b = self.p >> 3
        v = (int.from_bytes(self.d[b:b + 4], "little") >> (self.p & 7)) & ((1 << n) - 1)
        self.p += n
        return v

    def peek15(self):
        b = self.p >> 3
        return (int.from_bytes(self.d[b:b + 3], "little") >> (self.p & 7)) & 0x7FFF


def _decoder(lens, what, may_lack=False):
    """(table, widest): table[the next `widest` bits, LSB first] = (symbol,
    length).  The code must be complete; may_lack: a single code of one bit
    is allowed too (zlib's rule for the literal/length and distance codes),
    and so is an empty distance code (RFC 1951 3.2.7)."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    used = len(lens) - count[0]
    kraft = sum(count[l] << (15 - l) for l in range(1, 16))
    if kraft > 32768:
        raise AuditError("over-subscribed %s code" % what)
    if kraft < 32768 and not (may_lack and (used == 0 or (used == 1 and count[1] == 1))):
        raise AuditError("incomplete %s code" % what)
    widest = max(lens) if used else 0
    table = [None] * (1 << widest)
    for s, (l, c) in enumerate(zip(lens, canonical_codes(list(lens)))):
        if l:
            r = int(format(c, "0%db" % l)[::-1], 2)  # as the bits arrive
            for k in range(r, 1 << widest, 1 << l):
                table[k] = (s, l)
    return table, widest


def _symbol(bits, dec, what):
    table, widest = dec
    e = table[bits.peek15() & ((1 << widest) - 1)] if widest else None
    if e is None:
        raise AuditError("unassigned %s code" % what)
    if bits.p + e[1] > bits.end:
        raise AuditError("stream ends inside a block")
    bits.p += e[1]
    return e[0]


def _dynamic_header(bits, b):
    b.hlit, b.hdist, b.hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    if b.hlit > 286 or b.hdist > 30:
        raise AuditError("HLIT %d / HDIST %d" % (b.hlit, b.hdist))
    b.cl_lens = [0] * 19
    for i in range(b.hclen):
        b.cl_lens[CL_ORDER[i]] = bits.take(3)
    dec = _decoder(b.cl_lens, "code-length")
    b.cl_syms, b.cl_hist, lens = [], [0] * 19, []
    total = b.hlit + b.hdist
    while len(lens) < total:
        s = _symbol(bits, dec, "code-length")
        x = bits.take(CL_EXTRA[s]) if s >= 16 else 0
        b.cl_syms.append((s, x))
        b.cl_hist[s] += 1
        if s < 16:
            lens.append(s)
        else:
            if s == 16 and not lens:
                raise AuditError("repeat with no length before it")
            lens += [lens[-1] if s == 16 else 0] * (CL_REP0[s] + x)
    if len(lens) > total:
        raise AuditError("code lengths run past HLIT + HDIST")
    b.lit_lens, b.dist_lens = lens[:b.hlit], lens[b.hlit:]
    if not b.lit_lens[256]:
        raise AuditError("no end-of-block code")


def _body(bits, b, out):
    lit = _decoder(b.lit_lens, "literal/length", may_lack=True)
    # (the fixed distance code has 32 five-bit codes; 30 and 31 never occur)
    dist = _decoder([5] * 32 if b.btype == 1 else b.dist_lens, "distance", may_lack=True)
    start = len(out)
    while True:
        s = _symbol(bits, lit, "literal/length")
        b.lit_hist[s] += 1 if s < 286 else 0
        if s < 256:
            b.tokens.append(s)
            out.append(s)
            continue
        if s == 256:
            break
        if s > 285:
            raise AuditError("length symbol %d" % s)
        x = bits.take(LEN_EXTRA[s - 257])
        length = LEN_BASE[s - 257] + x
        ds = _symbol(bits, dist, "distance")
        if ds > 29:
            raise AuditError("distance symbol %d" % ds)
        b.dist_hist[ds] += 1
        d = DIST_BASE[ds] + bits.take(DIST_EXTRA[ds])
        if d > len(out):
            raise AuditError("distance %d with %d bytes produced" % (d, len(out)))
        b.tokens.append((258, d, True) if s == 284 and x == 31 else (length, d))
        p = len(out) - d
        for k in range(length):
            out.append(out[p + k])
    b.out = bytes(out[start:])


def parse(stream, history=b""):
    """The blocks of the DEFLATE stream at the start of `stream`, up to and
    including the one with BFINAL.  Raises AuditError on anything RFC 1951
    forbids (a reserved type, LEN / NLEN, a bad code, a distance too far)."""
    bits, out, blocks = _Bits(stream), bytearray(history), []
    while True:
        p0 = bits.p
        final, btype = bits.take(1), bits.take(2)
        b = Block(btype, bool(final), p0)
        if btype == 0:
            bits.p = (bits.p + 7) & ~7
            n, nn = bits.take(16), bits.take(16)
            if n ^ nn != 0xFFFF:
                raise AuditError("stored LEN / NLEN")
            a = bits.p >> 3
            if a + n > len(bits.d):
                raise AuditError("stream ends inside a block")
            b.stored_len, b.out = n, bits.d[a:a + n]
            b.tokens = list(b.out)
            out += b.out
            bits.p += 8 * n
            b.header_bits = bits.p - 8 * n - p0
        elif btype == 3:
            raise AuditError("reserved block type")
        else:
            if btype == 1:
                b.lit_lens, b.dist_lens = list(FIXED_LIT), list(FIXED_DIST)
            else:
                _dynamic_header(bits, b)
            b.header_bits = bits.p - p0
            _body(bits, b, out)
        b.bit_end = bits.p
        blocks.append(b)
        if final:
            return blocks


def expand_blocks(blocks):
    return b"".join(b.out for b in blocks)
