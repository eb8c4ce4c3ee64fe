// gunzip_chain.h -- host-only logic of the gzip read side: the member header
// and trailer checks of src/GUnzip.ts:67-175 (shared by zt_gunzip and
// zt_gunzip_batch), the input bound of a speculatively decoded candidate, and
// the walk that follows an item's member chain through a table of decoded
// candidates (include/zt_container_batch.h).  No device code and no HIP types:
// tools/gunzip_chain_check.cpp runs it under ASan / UBSan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/zt.h"

namespace zt {

// CRC-32 of a few host bytes (headers): table-free bitwise form, host logic only
inline uint32_t crc32_small(const uint8_t *p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

// A byte of the input, or -1 past its end (the reference reads `undefined`).
// u8(): the value a JS bitwise expression gives that byte (`undefined | x`
// counts it as 0: ByteStream.readUint/readShort/readUintBE, src/ByteStream.ts:52-83).
struct Reader {
  const uint8_t *in;
  size_t n, p;
  int byte() { return p < n ? in[p++] : (++p, -1); }
  uint32_t u8() { return p < n ? in[p++] : (++p, 0u); }
};

inline std::string js_num(int v) { return v < 0 ? std::string("undefined") : std::to_string(v); }

struct GzError {
  int code = ZT_OK;
  char msg[128] = {0};
};

// Header of the member at in[ip ..) (src/GUnzip.ts:67-147): the reference's
// checks in their order.  Fills m's header fields and *body (the first
// DEFLATE byte).  hcrc = false skips the FHCRC comparison (the speculative
// pass: the chain walk makes it for the members it accepts).
inline int gzip_parse_header(const uint8_t *in, size_t n, size_t ip, zt_gzip_member *m, size_t *body, GzError *e,
                             bool hcrc = true) {
  memset(m, 0, sizeof *m);
  Reader b{in, n, ip};
  const int id1 = b.byte(), id2 = b.byte();
  if (id1 != 0x1F || id2 != 0x8B) {
    snprintf(e->msg, sizeof e->msg, "invalid file signature:%s,%s", js_num(id1).c_str(), js_num(id2).c_str());
    return e->code = ZT_E_GZIP_SIGNATURE;
  }
  const int cm = b.byte();
  if (cm != 8) {
    snprintf(e->msg, sizeof e->msg, "unknown compression method: %s", js_num(cm).c_str());
    return e->code = ZT_E_GZIP_METHOD;
  }
  const int flg = b.byte();
  m->flg = (uint32_t)(flg < 0 ? 0 : flg);
  uint32_t mt = 0;
  for (int k = 0; k < 4; ++k) mt |= b.u8() << (8 * k);
  m->mtime = mt;
  m->xfl = b.u8();
  m->os = b.u8();
  if (m->flg & 0x04) {  // FEXTRA: skipped (src/GUnzip.ts:100-103,185-187)
    const uint32_t lo = b.u8(), hi = b.u8();
    m->xlen = lo | (hi << 8);
    b.p += m->xlen;
  }
  // a zero-terminated field: the reference reads bytes until one is 0 or
  // `undefined` (past the end) -- p ends one past that byte
  auto skip_string = [&b] {
    const void *z = b.p < b.n ? memchr(b.in + b.p, 0, b.n - b.p) : nullptr;
    b.p = z ? (size_t)(static_cast<const uint8_t *>(z) - b.in) + 1 : (b.p < b.n ? b.n : b.p) + 1;
  };
  if (m->flg & 0x08) {  // FNAME
    m->name_off = b.p;
    skip_string();
    m->name_len = b.p - 1 - m->name_off;
  }
  if (m->flg & 0x10) {  // FCOMMENT
    m->comment_off = b.p;
    skip_string();
    m->comment_len = b.p - 1 - m->comment_off;
  }
  if (m->flg & 0x02) {
    // FHCRC: the reference takes the CRC of input[0 .. p), from the start of
    // the whole input, not of the member (src/GUnzip.ts:127-131)
    const size_t upto = b.p < n ? b.p : n;
    const uint32_t lo = b.u8(), hi = b.u8();
    m->has_crc16 = 1;
    if (hcrc) {
      const uint32_t c16 = crc32_small(in, upto) & 0xFFFF;
      m->crc16 = c16;
      if (c16 != (lo | (hi << 8))) {
        snprintf(e->msg, sizeof e->msg, "invalid header crc16");
        return e->code = ZT_E_GZIP_HCRC;
      }
    }
  }
  if (b.p > n) {
    snprintf(e->msg, sizeof e->msg, "input buffer is broken");
    return e->code = ZT_E_INPUT_BROKEN;
  }
  *body = b.p;
  return ZT_OK;
}

// Trailer at in[eip ..) against the decoded body's CRC-32 and length
// (src/GUnzip.ts:155-172); fills m->crc32 / isize, *next = the next member.
inline int gzip_check_trailer(const uint8_t *in, size_t n, size_t eip, uint32_t crc, size_t olen, zt_gzip_member *m,
                              size_t *next, GzError *e) {
  Reader t{in, n, eip};
  uint32_t want = 0, isize = 0;
  for (int k = 0; k < 4; ++k) want |= t.u8() << (8 * k);
  if (crc != want) {
    snprintf(e->msg, sizeof e->msg, "invalid CRC-32 checksum: 0x%x / 0x%x", crc, want);
    return e->code = ZT_E_GZIP_CRC32;
  }
  for (int k = 0; k < 4; ++k) isize |= t.u8() << (8 * k);
  if ((uint32_t)olen != isize) {
    snprintf(e->msg, sizeof e->msg, "invalid input size: %u / %u", (uint32_t)olen, isize);
    return e->code = ZT_E_GZIP_ISIZE;
  }
  m->crc32 = crc;
  m->isize = isize;
  *next = t.p;
  return ZT_OK;
}

// ---- speculative members -------------------------------------------------------
// A candidate's decode reads at most `slack` bytes past the next candidate of
// its item: kGzSlack (zt_unzip's slack for entries of unknown size) while the
// item has at most one candidate per 4 KiB, less in proportion when they lie
// denser, so that the bounded inputs of an item's candidates add up to at most
// 17 times the item (+ kGzSlackMin per candidate) and device scratch stays
// proportional to the packed input however many candidates there are.  A
// member with a false candidate inside that ends more than `slack` behind it
// fails inside its bound and is decoded again to the item's end.
constexpr size_t kGzSlack = 64u << 10;
constexpr size_t kGzSlackMin = 256;
inline size_t gz_slack(size_t n, size_t ncand) {
  const size_t s = ncand ? n / ncand * 16 : kGzSlack;
  return s > kGzSlack ? kGzSlack : s < kGzSlackMin ? kGzSlackMin : s;
}

// Input bound of the member at `start`: `cands` = the item's sorted candidate
// offsets, n = the item's length.
inline size_t gz_bound(const std::vector<size_t> &cands, size_t start, size_t n, size_t slack = kGzSlack) {
  const auto nx = std::upper_bound(cands.begin(), cands.end(), start);
  if (nx == cands.end()) return n;
  return *nx + slack >= n ? n : *nx + slack;
}

// Host scan: up to `max` positions p > from where 1F 8B 08 starts inside
// in[0 .. n), ascending, appended to *out (the chain walk's way on when a
// start it needs was not in the device's candidate list).
inline void gz_scan(const uint8_t *in, size_t n, size_t from, size_t max, std::vector<size_t> *out) {
  size_t p = from + 1;
  while (max && p + 3 <= n) {
    const void *q = memchr(in + p, 0x1F, n - 2 - p);
    if (!q) return;
    p = (size_t)(static_cast<const uint8_t *>(q) - in);
    if (in[p + 1] == 0x8B && in[p + 2] == 0x08) {
      out->push_back(p);
      --max;
    }
    ++p;
  }
}

// One decoded candidate of an item.
struct GzDecoded {
  size_t start = 0;    // member offset in the item
  size_t bound = 0;    // input length it was decoded with (== the item's n: unbounded)
  int status = ZT_OK;  // decoder status and detail (inflate_error)
  int detail = 0;
  size_t end_ip = 0;   // first byte after the DEFLATE stream
  size_t out_len = 0;
  uint32_t crc = 0;    // CRC-32 of the decoded bytes
  size_t slot = 0;     // caller's handle of the output
  bool exact = true;   // a failing status is the decoder's own (false: "failed" is all that is known)
};

// A decode that finished with every bit it consumed inside its bound stands
// for the unbounded one (a stream cut at the bound reads zeros there, and
// zeros can end a block).  A failure stands only when the member was decoded
// to the item's end and the status is the decoder's own.
inline bool gz_settled(const GzDecoded &d, size_t n) {
  return d.status == ZT_OK ? d.end_ip <= d.bound || d.bound >= n : d.bound >= n && d.exact;
}

// Bound of the next decode of a member that did not settle inside `bound`: 8
// times the input it had (at least 1 MiB), so that a long item's scratch stays
// in proportion to what its members need; the item's end at the latest.
inline size_t gz_wider(size_t start, size_t bound, size_t n) {
  const size_t had = bound > start ? bound - start : 0;
  const size_t want = had >= n / 8 ? n : std::max<size_t>(8 * had, 1u << 20);
  return want >= n - std::min(n, start) ? n : start + want;
}

enum GzWalkState { GZ_WALKING = 0, GZ_DONE, GZ_FAILED, GZ_NEED };

// Chain walk of one item from offset 0, resumable across decode passes.
struct GzWalk {
  GzWalkState state = GZ_WALKING;
  size_t ip = 0;  // next member start
  std::vector<zt_gzip_member> members;  // accepted, data_off = offset in the item's output
  std::vector<size_t> slots;            // their outputs (GzDecoded::slot)
  size_t total = 0;                     // output bytes so far
  GzError err;                          // GZ_FAILED
  int detail = 0;                       // GZ_FAILED with a decoder status: its detail (err.msg is empty)
  size_t need_start = 0;                // GZ_NEED: decode the member here ...
  bool need_full = false;               // ... again, with a wider bound (it did not settle inside need_bound)
  size_t need_bound = 0;
  bool need_exact = false;              // ... and with the decoder's own status (decoded to the item's end already)
};

// Advances w over `table` (the item's decoded candidates, sorted by start; of
// two decodes of one start the later entry wins).  Accepts members in
// zt_gunzip's order of checks: header, decoder status, CRC-32, ISIZE; the
// next start is end_ip + 8.  Stops at GZ_DONE (input consumed), GZ_FAILED
// (the error the single call reports) or GZ_NEED (a start that is not in the
// table, or one that did not settle: see gz_settled).
inline GzWalkState gz_walk(const uint8_t *in, size_t n, const std::vector<GzDecoded> &table, GzWalk *w) {
  if (w->state == GZ_DONE || w->state == GZ_FAILED) return w->state;
  w->state = GZ_WALKING;
  while (w->ip < n) {
    zt_gzip_member m;
    size_t body = 0;
    if (gzip_parse_header(in, n, w->ip, &m, &body, &w->err)) return w->state = GZ_FAILED;
    // last entry with this start
    auto it = std::upper_bound(table.begin(), table.end(), w->ip,
                               [](size_t v, const GzDecoded &d) { return v < d.start; });
    const GzDecoded *d = (it != table.begin() && (it - 1)->start == w->ip) ? &*(it - 1) : nullptr;
    if (!d || !gz_settled(*d, n)) {
      w->need_start = w->ip;
      w->need_full = d != nullptr;
      w->need_bound = d ? d->bound : 0;
      w->need_exact = d && d->bound >= n;
      return w->state = GZ_NEED;
    }
    if (d->status) {
      w->err.code = d->status;
      w->err.msg[0] = 0;
      w->detail = d->detail;
      return w->state = GZ_FAILED;
    }
    size_t next = 0;
    if (gzip_check_trailer(in, n, d->end_ip, d->crc, d->out_len, &m, &next, &w->err)) return w->state = GZ_FAILED;
    m.data_off = w->total;
    m.data_len = d->out_len;
    w->total += d->out_len;
    w->members.push_back(m);
    w->slots.push_back(d->slot);
    w->ip = next;
  }
  return w->state = GZ_DONE;
}

}  // namespace zt
