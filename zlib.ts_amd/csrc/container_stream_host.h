// container_stream_host.h -- the framing of the container sessions
// (include/zt_stream_container.h), no HIP: the incremental "is this member
// header complete, and how long is it" test over the bytes held back, the
// AUTO decision, the trailer that arrives in pieces, the member records and
// the state machine that walks header | body | trailer | next member over a
// feed's bytes.  Every check and every error text is the one-shot calls' own:
// gzip_parse_header / gzip_check_trailer (gunzip_chain.h) and
// zlib_parse_header / zlib_header_status (dict_host.h) are called on the
// accumulated bytes.  Pure functions, checked on the CPU by
// tools/container_stream_check.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../include/zt_dict.h"
#include "dict_host.h"
#include "gunzip_chain.h"
#include "stream_host.h"

namespace zt {

// (include/zt_stream_container.h: ZT_SESSION_*)
enum CsFormat : int { CS_AUTO = 0, CS_GZIP = 1, CS_ZLIB = 2 };

// the record turn-over of a session that starts a new member (session_turn.hip)
struct SessTurn {
  SessRec *rec;
  uint64_t op;  // 0, or the preset window's length (FDICT)
};

constexpr size_t kCsHeaderMax = 1u << 20;  // header fields of one member: the cap of the carry buffer
constexpr size_t kCsGzipTrailer = 8, kCsZlibTrailer = 4;

// ---- the gzip header, incrementally -------------------------------------------------
// Over p[0 .. n), the bytes from a member's first one: `decided` when
// gzip_parse_header can give its final answer -- the header is complete (len
// = its length), or a field that fails is (the signature at 2 bytes, the
// method at 3; len = the bytes that decide).  Else more bytes are needed.
struct GzHeaderScan {
  bool decided;
  size_t len;
};
inline GzHeaderScan gz_header_scan(const uint8_t *p, size_t n) {
  if (n < 2) return {false, 0};
  if (p[0] != 0x1F || p[1] != 0x8B) return {true, 2};
  if (n < 3) return {false, 0};
  if (p[2] != 8) return {true, 3};
  if (n < 10) return {false, 0};
  const uint32_t flg = p[3];
  size_t at = 10;
  if (flg & 0x04) {
    if (n < at + 2) return {false, 0};
    at += 2 + ((size_t)p[at] | ((size_t)p[at + 1] << 8));
    if (n < at) return {false, 0};
  }
  for (const uint32_t bit : {0x08u, 0x10u})
    if (flg & bit) {
      const void *z = at < n ? memchr(p + at, 0, n - at) : nullptr;
      if (!z) return {false, 0};
      at = (size_t)(static_cast<const uint8_t *>(z) - p) + 1;
    }
  if (flg & 0x02) at += 2;
  if (n < at) return {false, 0};
  return {true, at};
}

// ---- AUTO ------------------------------------------------------------------------------
// On a stream's first two bytes: 1F 8B is gzip, a valid CMF / FLG pair is
// zlib, anything else (a shorter input included) is left to the gzip
// signature check.
inline CsFormat cs_auto(const uint8_t *p, size_t n) {
  if (n >= 2 && !(p[0] == 0x1F && p[1] == 0x8B) && (p[0] & 0x0F) == 8 && (((uint32_t)p[0] << 8) + p[1]) % 31 == 0)
    return CS_ZLIB;
  return CS_GZIP;
}

// ISIZE of a member of `len` bytes: RFC 1952's length modulo 2^32
inline uint32_t cs_isize(uint64_t len) { return (uint32_t)(len & 0xFFFFFFFFu); }

// Adler-32 of a few host bytes (a dictionary's id)
inline uint32_t adler32_small(const uint8_t *p, size_t n) {
  uint32_t s1 = 1, s2 = 0;
  while (n) {
    const size_t k = n < 5552 ? n : 5552;
    for (size_t i = 0; i < k; ++i) {
      s1 += p[i];
      s2 += s1;
    }
    s1 %= 65521;
    s2 %= 65521;
    p += k;
    n -= k;
  }
  return s1 | (s2 << 16);
}

// ---- a session's framing ---------------------------------------------------------
struct CsMember {
  zt_gzip_member m{};          // name_off / comment_off count from the member's start; data_off / data_len unused
  std::string name, comment;   // copies of the header's bytes
  uint64_t data_off = 0, data_len = 0, in_off = 0;
};
enum CsState : int {
  CS_START = 0,  // AUTO, undecided
  CS_BETWEEN,    // gzip: at a member's end (the start included)
  CS_HEADER,
  CS_BODY,       // the inflate session decodes
  CS_TRAILER,
  CS_DONE,
  CS_FAILED,
};
struct CsFrame {
  int format = CS_AUTO;
  int verify = 1;
  CsState state = CS_START;
  // done ones, and behind them the one being read.  A deque: a member, and with it the name and
  // comment bytes zt_container_session_member hands out, keeps its address while later ones are added
  std::deque<CsMember> members;
  uint64_t members_done = 0;
  uint32_t crc = 0, adler = 1;    // of the current member's output so far
  uint64_t member_out = 0;        // its length so far
  uint64_t total_out = 0;         // output of the members done
  uint64_t unused = 0;            // zlib: bytes behind the trailer
  uint32_t dict_len = 0;          // the preset window's length (at most 32 KiB of the dictionary)
  bool has_dict = false;
  uint32_t dict_id = 0;           // Adler-32 of the whole dictionary
  int code = ZT_OK;
  std::string msg;

  void init(int fmt, int vfy) {
    format = fmt;
    verify = vfy;
    state = fmt == CS_AUTO ? CS_START : fmt == CS_GZIP ? CS_BETWEEN : CS_HEADER;
  }
  bool at_member_end() const { return state == CS_BETWEEN || (state == CS_DONE && code == ZT_OK); }
};

enum CsAction : int {
  CS_ACT_WAIT = 0,  // more input is needed: the bytes not consumed stay pending
  CS_ACT_BODY,      // a DEFLATE body starts behind the consumed bytes
  CS_ACT_DONE,      // the session is finished; what is left trails it
  CS_ACT_ERROR,     // f->code / f->msg
};
struct CsStep {
  size_t consumed = 0;
  CsAction action = CS_ACT_WAIT;
  bool turn = false;  // CS_ACT_BODY: the device record is turned over first ...
  uint64_t op = 0;    // ... to this output position (the preset window's length)
  bool window = false;  // ... and the preset window is uploaded before that
};

inline CsStep cs_fail(CsFrame *f, size_t consumed, int code, const std::string &msg) {
  f->state = CS_FAILED;
  f->code = code;
  f->msg = msg;
  CsStep st;
  st.consumed = consumed;
  st.action = CS_ACT_ERROR;
  return st;
}

// One walk over p[0 .. avail), the session's unconsumed bytes, while it is
// not inside a body: trailer, member end, next header.  in_pos: p[0]'s offset
// in the total input.  Stops at the first of: a body starts, more input is
// needed, the session is done, an error.
inline CsStep cs_step(CsFrame *f, const uint8_t *p, size_t avail, int last, uint64_t in_pos) {
  CsStep st;
  for (;;) {
    const uint8_t *q = p + st.consumed;
    const size_t n = avail - st.consumed;
    switch (f->state) {
      case CS_START: {
        if (n < 2 && !last) return st;
        f->format = cs_auto(q, n);
        f->state = f->format == CS_GZIP ? CS_BETWEEN : CS_HEADER;
        break;
      }
      case CS_BETWEEN: {
        if (n == 0) {
          if (!last) return st;
          f->state = CS_DONE;
          st.action = CS_ACT_DONE;
          return st;
        }
        f->state = CS_HEADER;
        break;
      }
      case CS_HEADER: {
        CsMember mem;
        mem.in_off = in_pos + st.consumed;
        mem.data_off = f->total_out;
        size_t body = 0;
        if (f->format == CS_GZIP) {
          const GzHeaderScan sc = gz_header_scan(q, n);
          const size_t have = sc.decided ? sc.len : n;
          if (have > kCsHeaderMax) return cs_fail(f, st.consumed, ZT_E_ARG, "gzip header fields exceed 1 MiB");
          if (!sc.decided && !last) return st;
          GzError ge;
          if (gzip_parse_header(q, have, 0, &mem.m, &body, &ge)) return cs_fail(f, st.consumed, ge.code, ge.msg);
          if (mem.m.flg & 0x08) mem.name.assign(reinterpret_cast<const char *>(q) + mem.m.name_off, mem.m.name_len);
          if (mem.m.flg & 0x10)
            mem.comment.assign(reinterpret_cast<const char *>(q) + mem.m.comment_off, mem.m.comment_len);
          st.turn = !f->members.empty();
          st.op = 0;
        } else {
          // the method is decided by the first byte, FCHECK by the second
          if (n < 2 && !last && !(n == 1 && (q[0] & 0x0F) != 8)) return st;
          ZlibHeader h;
          const ZlibHdr hs = zlib_parse_header(q, n, 0, &h);
          int code;
          std::string msg;
          if (zlib_header_status(hs, h, &code, &msg)) return cs_fail(f, st.consumed, code, msg);
          if (h.fdict) {  // zt_zlib_decompress_dict's checks in its order
            if (!f->has_dict) return cs_fail(f, st.consumed, ZT_E_ZLIB_FDICT, "fdict flag is not supported");
            if (hs == ZH_BROKEN) {
              if (!last) return st;
              return cs_fail(f, st.consumed, ZT_E_INPUT_BROKEN, "input buffer is broken");
            }
            if (f->dict_id != h.dictid) {
              char text[96];
              snprintf(text, sizeof text, "invalid dictionary id: 0x%x / 0x%x", h.dictid, f->dict_id);
              return cs_fail(f, st.consumed, ZT_E_ZLIB_DICTID, text);
            }
            st.turn = true;
            st.window = f->dict_len != 0;
            st.op = f->dict_len;
          }
          body = h.body;
        }
        f->members.push_back(std::move(mem));
        f->crc = 0;
        f->adler = 1;
        f->member_out = 0;
        f->state = CS_BODY;
        st.consumed += body;
        st.action = CS_ACT_BODY;
        return st;
      }
      case CS_TRAILER: {
        CsMember &mem = f->members.back();
        const size_t need = f->format == CS_GZIP ? kCsGzipTrailer : kCsZlibTrailer;
        if (n < need && !last) return st;
        const size_t have = n < need ? n : need;  // (a truncated trailer reads as zeros, as the one-shot calls read it)
        if (f->format == CS_GZIP) {
          GzError ge;
          size_t next = 0;
          if (gzip_check_trailer(q, have, 0, f->crc, (size_t)cs_isize(f->member_out), &mem.m, &next, &ge))
            return cs_fail(f, st.consumed, ge.code, ge.msg);
        } else {
          uint32_t want = 0;
          for (size_t k = 0; k < 4; ++k) want = (want << 8) | (k < have ? q[k] : 0u);
          if (f->verify && want != f->adler)
            return cs_fail(f, st.consumed, ZT_E_ZLIB_ADLER, "invalid adler-32 checksum");
          mem.m.crc32 = f->adler;
          mem.m.isize = cs_isize(f->member_out);
        }
        mem.data_len = f->member_out;
        f->total_out += f->member_out;
        f->members_done++;
        st.consumed += have;
        if (f->format == CS_GZIP) {
          f->state = CS_BETWEEN;
          break;
        }
        f->state = CS_DONE;
        st.action = CS_ACT_DONE;
        return st;
      }
      case CS_BODY:
        st.action = CS_ACT_BODY;
        return st;
      case CS_DONE:
        st.action = CS_ACT_DONE;
        return st;
      default:
        st.action = CS_ACT_ERROR;
        return st;
    }
  }
}

// ---- where a truncated body ends ---------------------------------------------------
// The session kernel reports a final feed that runs out of input as
// ZT_E_INPUT_BROKEN wherever the input ends; the one-shot decoder reports the
// end inside a stored block's LEN / NLEN as ZT_E_STORED_LEN / ZT_E_STORED_NLEN
// (inflate.hip: LEN at the byte boundary p behind the block's three header
// bits; p + 1 >= n is LEN, p + 3 >= n is NLEN).  A container session reports
// what the one-shot call reports, so after such a failure the host walks the
// tokens of the final feed's bytes itself, from the state the record had
// before the launch (a failing launch leaves it unchanged), and says where
// the input ended.  Lengths only: nothing is produced, distances are not
// judged (the kernel found nothing wrong before the input ended).
enum CsTruncation : int { CS_TRUNC_OTHER = 0, CS_TRUNC_STORED_LEN, CS_TRUNC_STORED_NLEN };

struct CsBits {
  const uint8_t *in;
  uint64_t nbits, pos;
  bool get(int k, uint32_t *v) {
    if (pos + (uint64_t)k > nbits) return false;
    uint32_t r = 0;
    for (int i = 0; i < k; ++i, ++pos) r |= (uint32_t)((in[pos >> 3] >> (pos & 7)) & 1) << i;
    *v = r;
    return true;
  }
};
struct CsHuff {
  uint16_t count[16], symbol[320];
  // canonical code of lens[0 .. n); false: over-subscribed
  bool build(const uint8_t *lens, int n) {
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) {
      if (lens[s] > 15) return false;
      count[lens[s]]++;
    }
    int left = 1;
    for (int l = 1; l < 16; ++l) {
      left = (left << 1) - count[l];
      if (left < 0) return false;
    }
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int s = 0; s < n; ++s)
      if (lens[s]) symbol[offs[lens[s]]++] = (uint16_t)s;
    return true;
  }
  // the next symbol; -1: no such code, -2: the input ended
  int decode(CsBits *b) const {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
      uint32_t bit;
      if (!b->get(1, &bit)) return -2;
      code |= (int)bit;
      const int cnt = count[l];
      if (code - cnt < first) return symbol[index + (code - first)];
      index += cnt;
      first += cnt;
      first <<= 1;
      code <<= 1;
    }
    return -1;
  }
};

// in[0 .. n): the final feed's bytes of a body whose decode ran out of input,
// the decoder standing at bit `bit` in the state (phase, btype, ...) of the
// session record; lens: the record's code lengths (SP_HUFF, BTYPE 2).
inline CsTruncation cs_truncation(const uint8_t *in, size_t n, uint64_t bit, uint32_t phase, uint32_t bfinal,
                                  uint32_t btype, uint32_t stored_left, uint32_t hlit, uint32_t hdist,
                                  const uint8_t *lens) {
  static const uint16_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  static const uint16_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
  static const uint8_t kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  CsBits b{in, (uint64_t)n * 8, bit};
  CsHuff lit, dist;
  uint8_t cl[320];
  auto fixed = [&] {
    for (int s = 0; s < 288; ++s) cl[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
    lit.build(cl, 288);
    for (int s = 0; s < 30; ++s) cl[s] = 5;
    dist.build(cl, 30);
  };
  if (phase == SP_HUFF) {
    if (btype == 1) {
      fixed();
    } else {
      if (hlit > 286 || hdist > 30 || hlit + hdist > 320) return CS_TRUNC_OTHER;
      if (!lit.build(lens, (int)hlit) || !dist.build(lens + hlit, (int)hdist)) return CS_TRUNC_OTHER;
    }
  }
  uint32_t v;
  for (;;) {
    if (phase == SP_DONE) return CS_TRUNC_OTHER;
    if (phase == SP_STORED) {
      const uint64_t have = (b.nbits - b.pos) >> 3;
      if (have < stored_left) return CS_TRUNC_OTHER;  // inside the payload
      b.pos += (uint64_t)stored_left * 8;
      phase = bfinal ? SP_DONE : SP_HEADER;
      continue;
    }
    if (phase == SP_HEADER) {
      if (!b.get(3, &v)) return CS_TRUNC_OTHER;
      bfinal = v & 1;
      btype = v >> 1;
      if (btype == 0) {
        const uint64_t p = (b.pos + 7) >> 3;
        if (p + 1 >= n) return CS_TRUNC_STORED_LEN;
        if (p + 3 >= n) return CS_TRUNC_STORED_NLEN;
        stored_left = (uint32_t)in[p] | ((uint32_t)in[p + 1] << 8);
        b.pos = (p + 4) * 8;
        phase = stored_left ? SP_STORED : (bfinal ? SP_DONE : SP_HEADER);
        continue;
      }
      if (btype == 3) return CS_TRUNC_OTHER;
      if (btype == 1) {
        fixed();
      } else {
        uint32_t nl, nd, nc;
        if (!b.get(5, &nl) || !b.get(5, &nd) || !b.get(4, &nc)) return CS_TRUNC_OTHER;
        nl += 257;
        nd += 1;
        nc += 4;
        if (nl > 286 || nd > 30) return CS_TRUNC_OTHER;
        uint8_t cll[19] = {0};
        for (uint32_t k = 0; k < nc; ++k) {
          if (!b.get(3, &v)) return CS_TRUNC_OTHER;
          cll[kOrder[k]] = (uint8_t)v;
        }
        CsHuff clh;
        if (!clh.build(cll, 19)) return CS_TRUNC_OTHER;
        uint32_t k = 0;
        while (k < nl + nd) {
          const int s = clh.decode(&b);
          if (s < 0) return CS_TRUNC_OTHER;
          if (s < 16) {
            cl[k++] = (uint8_t)s;
            continue;
          }
          uint32_t rep, prev = 0;
          if (s == 16) {
            if (k == 0 || !b.get(2, &rep)) return CS_TRUNC_OTHER;
            prev = cl[k - 1];
            rep += 3;
          } else if (!b.get(s == 17 ? 3 : 7, &rep)) {
            return CS_TRUNC_OTHER;
          } else {
            rep += s == 17 ? 3 : 11;
          }
          if (k + rep > nl + nd) return CS_TRUNC_OTHER;
          while (rep--) cl[k++] = (uint8_t)prev;
        }
        if (!lit.build(cl, (int)nl) || !dist.build(cl + nl, (int)nd)) return CS_TRUNC_OTHER;
      }
      phase = SP_HUFF;
      continue;
    }
    // SP_HUFF
    const int s = lit.decode(&b);
    if (s < 0) return CS_TRUNC_OTHER;
    if (s < 256) continue;
    if (s == 256) {
      phase = bfinal ? SP_DONE : SP_HEADER;
      continue;
    }
    if (s > 285) return CS_TRUNC_OTHER;
    if (kLenExtra[s - 257] && !b.get(kLenExtra[s - 257], &v)) return CS_TRUNC_OTHER;
    const int d = dist.decode(&b);
    if (d < 0 || d >= 30) return CS_TRUNC_OTHER;
    if (kDistExtra[d] && !b.get(kDistExtra[d], &v)) return CS_TRUNC_OTHER;
  }
}

// bits of the fed bytes consumed so far: all but the pending ones, and of the first pending byte bit_off
inline uint64_t cs_end_bits(uint64_t total_in, uint64_t unused, size_t pending, uint32_t bit_off) {
  return (total_in - unused - pending) * 8 + bit_off;
}

}  // namespace zt
