// ckpt_host.h -- host-only logic of the checkpoint index
// (include/zt_checkpoint.h): the blob layout, its validation, and the planner
// that turns a set of ranges into everything the range kernels need (packed
// block headers and input spans, exact-start units with the state each must
// end in, ChainUnits, copy segments and the window each starts from).  No
// device code and no HIP types: tools/ckpt_host_check.cpp runs it under
// ASan / UBSan.
//
// The blob is a hint that is verified, never trusted.  ckpt_validate is the
// first half of that: after it, every offset the planner derives from the
// blob lies inside the caller's input and inside the buffers the plan sizes.
// The second half is ckpt_verify_kernel (ckpt_api.hip), which holds what the
// tokenizer found to what the blob promised.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/zt_checkpoint.h"
#include "index_host.h"

namespace zt {

constexpr size_t kCkHeader = ZT_CKPT_HEADER_BYTES;
constexpr size_t kCkEntry = ZT_CKPT_ENTRY_BYTES;
constexpr size_t kCkWindow = ZT_CKPT_WINDOW_BYTES;
constexpr size_t kCkWinRec = ZT_CKPT_WINDOW_RECORD_BYTES;
// entry kinds: the general tokenizer's GK_* (zt_internal.h; asserted equal in ckpt_api.hip)
enum : uint32_t { CK_BLOCK = 0, CK_HUFF = 1, CK_STORED = 2, CK_SHDR = 3, CK_FINAL = 4 };
constexpr uint64_t kCkFixedHdr = ZT_CKPT_FIXED_HDR;
constexpr uint64_t kCkNoStop = ~0ull;
// A dynamic block header is at most 3 (BFINAL, BTYPE) + 5 + 5 + 4 (HLIT, HDIST,
// HCLEN) + 19 x 3 (code-length code lengths) = 74 bits, then HLIT + HDIST <=
// 286 + 30 = 316 code lengths.  A length sent on its own costs one
// code-length code of at most 7 bits; the repeat codes 16 / 17 / 18 cost at
// most 7 + 7 = 14 bits for at least 3 lengths, fewer bits per length.  So a
// header holds at most 74 + 316 x 7 = 2286 bits (RFC 1951 3.2.7): 286 bytes,
// 287 when it does not start on a byte.  A slot keeps hdr & 7.
constexpr uint32_t kCkHdrBytesMax = 287;
constexpr uint32_t kCkHdrSlot = 320;  // (64-aligned slots)
// output bytes one token can stand for (a match of 258), tokens a unit can hold
constexpr uint64_t kCkTokBytesMax = 258;
constexpr uint32_t kCkTokMax = 1u << 30;

struct CkEntry {
  uint64_t pos, hdr, out_off;
  uint32_t kind, rem, flags, ntok, win, pad;
};
static_assert(sizeof(CkEntry) == kCkEntry, "entry layout is the interface");

inline size_t ckpt_blob_bytes(size_t nunits, size_t nwin) {
  return kCkHeader + (nunits + 1) * kCkEntry + nwin * kCkWinRec;
}
inline void ckpt_write_header(uint8_t *blob, uint32_t nunits, uint32_t nwin, uint64_t stream_start, uint64_t end_ip,
                              uint64_t total_out, uint64_t span) {
  memset(blob, 0, kCkHeader);
  memcpy(blob, "ZTCK", 4);
  idx_put32(blob + 4, ZT_CKPT_VERSION);
  idx_put32(blob + 8, nunits);
  idx_put32(blob + 12, nwin);
  idx_put64(blob + 16, stream_start);
  idx_put64(blob + 24, end_ip);
  idx_put64(blob + 32, total_out);
  idx_put64(blob + 40, span);
}
inline void ckpt_write_entry(uint8_t *blob, size_t k, const CkEntry &e) {
  uint8_t *p = blob + kCkHeader + k * kCkEntry;
  idx_put64(p, e.pos);
  idx_put64(p + 8, e.hdr);
  idx_put64(p + 16, e.out_off);
  idx_put32(p + 24, e.kind);
  idx_put32(p + 28, e.rem);
  idx_put32(p + 32, e.flags);
  idx_put32(p + 36, e.ntok);
  idx_put32(p + 40, e.win);
  idx_put32(p + 44, 0);
}
inline uint8_t *ckpt_window_at(uint8_t *blob, size_t nunits, size_t w) {
  return blob + kCkHeader + (nunits + 1) * kCkEntry + w * kCkWinRec;
}

// The build's rule: a window goes to the first entry (entry 0 and the
// sentinel apart) at or after every positive multiple of span.  e: nunits + 1
// entries with out_off set; sets flags bit 0 and win, returns the window count.
inline uint32_t ckpt_place_windows(std::vector<CkEntry> &e, uint64_t span) {
  uint32_t nwin = 0;
  const size_t nunits = e.size() - 1;
  uint64_t next = span;
  for (size_t k = 1; k < nunits; ++k) {
    if (e[k].out_off < next) continue;
    e[k].flags |= 1u;
    e[k].win = nwin++;
    next = (e[k].out_off / span + 1) * span;
  }
  return nwin;
}

// A validated blob, parsed: nunits + 1 entries (the sentinel last).
struct CkptView {
  uint32_t nunits = 0, nwin = 0;
  uint64_t stream_start = 0, end_ip = 0, total_out = 0, span = 0;
  std::vector<CkEntry> e;
  std::vector<uint32_t> win_units;  // entry 0, then the window-carrying entries, ascending
  const uint8_t *wins = nullptr;    // the window records (inside the blob)
};

// Checks the blob against itself and against the input length `n`.  Returns
// null and fills *v, or a one-line reason.
inline const char *ckpt_validate(const uint8_t *idx, size_t idx_len, size_t n, CkptView *v) {
  if (!idx || idx_len < kCkHeader + 2 * kCkEntry) return "checkpoint blob truncated";
  if (memcmp(idx, "ZTCK", 4) != 0) return "not a checkpoint blob (magic)";
  if (idx_get32(idx + 4) != ZT_CKPT_VERSION) return "unknown checkpoint blob version";
  const uint64_t nunits = idx_get32(idx + 8), nwin = idx_get32(idx + 12);
  if (nunits == 0 || (uint64_t)idx_len != kCkHeader + (nunits + 1) * kCkEntry + nwin * kCkWinRec)
    return "blob length does not match its unit and window counts";
  v->nunits = (uint32_t)nunits;
  v->nwin = (uint32_t)nwin;
  v->stream_start = idx_get64(idx + 16);
  v->end_ip = idx_get64(idx + 24);
  v->total_out = idx_get64(idx + 32);
  v->span = idx_get64(idx + 40);
  for (size_t k = 48; k < kCkHeader; ++k)
    if (idx[k]) return "blob header padding is not zero";
  if (v->span < ZT_CKPT_SPAN_MIN) return "checkpoint span below the minimum";
  if (v->stream_start > v->end_ip || v->end_ip > n) return "blob positions lie outside the input";
  v->e.resize(nunits + 1);
  for (size_t k = 0; k <= nunits; ++k) {
    const uint8_t *p = idx + kCkHeader + k * kCkEntry;
    CkEntry &e = v->e[k];
    e.pos = idx_get64(p);
    e.hdr = idx_get64(p + 8);
    e.out_off = idx_get64(p + 16);
    e.kind = idx_get32(p + 24);
    e.rem = idx_get32(p + 28);
    e.flags = idx_get32(p + 32);
    e.ntok = idx_get32(p + 36);
    e.win = idx_get32(p + 40);
    e.pad = idx_get32(p + 44);
    if (e.pad) return "entry padding is not zero";
  }
  const uint64_t bit0 = v->stream_start * 8;
  const CkEntry &e0 = v->e[0], &es = v->e[nunits];
  if (e0.pos != bit0 || e0.kind != CK_BLOCK || e0.hdr || e0.out_off || e0.rem || e0.flags || e0.win)
    return "first entry is not the stream start";
  if (es.kind != CK_FINAL || es.pos < bit0 || (es.pos + 7) / 8 != v->end_ip || es.out_off != v->total_out || es.hdr ||
      es.rem || es.flags || es.ntok || es.win)
    return "blob sentinel is wrong";
  v->win_units.assign(1, 0u);
  uint32_t wins = 0;
  for (size_t k = 0; k < nunits; ++k) {
    const CkEntry &e = v->e[k], &nx = v->e[k + 1];
    if (e.pos > nx.pos || e.out_off > nx.out_off) return "blob offsets decrease";
    if (e.pos < bit0) return "blob positions lie outside the input";  // (<= the sentinel's: inside end_ip)
    if (e.kind > CK_SHDR) return "unknown entry kind";
    if (e.flags & ~3u) return "unknown entry flags";
    if (e.kind == CK_BLOCK && (e.flags & 2u)) return "a block start cannot carry BFINAL";
    if (e.kind == CK_HUFF) {
      if (e.hdr != kCkFixedHdr && (e.hdr < bit0 || e.hdr >= e.pos)) return "block header does not lie before its body";
    } else if (e.hdr) {
      return "entry names a header it cannot use";
    }
    if (e.kind == CK_STORED) {
      if ((e.pos & 7) || e.rem == 0 || e.rem > 65535 || e.pos / 8 + e.rem > v->end_ip)
        return "stored payload does not fit the input";
    } else if (e.rem) {
      return "entry has payload bytes it cannot use";
    }
    if (e.kind == CK_SHDR && ((e.pos & 7) || e.pos / 8 + 4 > v->end_ip)) return "stored length field outside the input";
    // a token takes at least one bit (a stored byte eight) and gives at most 258 bytes
    if (e.ntok >= kCkTokMax || e.ntok > nx.pos - e.pos) return "unit token count over what its bits can hold";
    if (nx.out_off - e.out_off > (uint64_t)e.ntok * kCkTokBytesMax) return "unit output larger than its tokens can produce";
    if (e.flags & 1u) {
      // (k == 0 was refused above; span >= 64 KiB puts every window entry past 32 KiB)
      if (e.win != wins || wins >= nwin) return "window index out of range or out of order";
      if (e.out_off < kCkWindow) return "window entry less than 32 KiB into the output";
      ++wins;
      v->win_units.push_back((uint32_t)k);
    } else if (e.win) {
      return "entry without a window names one";
    }
  }
  if (wins != nwin) return "window count is wrong";
  v->wins = idx + kCkHeader + (nunits + 1) * kCkEntry;
  return nullptr;
}
inline uint32_t ckpt_window_crc(const CkptView &v, uint32_t w) { return idx_get32(v.wins + w * kCkWinRec + kCkWindow); }

// ---- the planner ---------------------------------------------------------------
// (the ranges, the span base and the totals: range_plan.h.)  `first` is entry 0
// or a window entry; in_pos is where byte0 lies in the packed input, in_len
// runs up to the byte holding pos[last + 1].
struct CkSpan : RangeSpan {
  uint64_t byte0 = 0;  // first compressed byte in `in`: pos[first] / 8
};
// A dynamic block header that lies before its span, packed once per call.
struct CkHdr {
  uint64_t hdr = 0;   // bit position in `in`
  uint64_t src = 0;   // hdr / 8
  uint32_t len = 0;   // bytes copied (the slot's rest is zero)
  uint64_t slot = 0;  // byte position of the slot in the packed input
};
// A planned unit: an exact start state and the state the next entry says it
// ends in, both in bit positions of the packed input.
struct CkUnit {
  uint64_t pos, hdr, stop;       // start state; stop: the next entry's pos (kCkNoStop: the stream's last unit)
  uint64_t e_pos, e_hdr;         // end state
  uint64_t tok_off;
  uint32_t tok_cap;
  uint32_t kind, rem, bfinal;
  uint32_t e_kind, e_rem, e_bfinal;
  uint32_t ntok, out_len;
  uint32_t entry;                // its entry in the blob
};
// (in_total: header slots, then spans)
struct CkptPlan : RangePlanCore {
  std::vector<CkSpan> spans;
  std::vector<CkHdr> hdrs;        // ascending by hdr
  std::vector<CkUnit> units;
  // per copy segment: its history ring starts as uploaded window seg_win[g]
  // (-1: the stream start, no history)
  std::vector<int32_t> seg_win;
  std::vector<uint32_t> wins;     // blob window of each uploaded window
};

inline CkptPlan ckpt_plan(const CkptView &v, size_t n, const uint64_t *off, const uint64_t *len, size_t count) {
  CkptPlan p;
  auto out_of = [&](uint32_t k) { return v.e[k].out_off; };
  p.spans = range_spans<CkSpan>(v.total_out, v.win_units, v.nunits, out_of, off, len, count, &p.ranges);
  // the headers that lie before the span of a unit that names them, once each
  std::vector<uint64_t> hs;
  for (CkSpan &s : p.spans) {
    s.byte0 = v.e[s.first].pos / 8;
    for (uint32_t u = s.first; u <= s.last + 1 && u < v.nunits; ++u)
      if (v.e[u].kind == CK_HUFF && v.e[u].hdr != kCkFixedHdr && v.e[u].hdr / 8 < s.byte0) hs.push_back(v.e[u].hdr);
  }
  std::sort(hs.begin(), hs.end());
  hs.erase(std::unique(hs.begin(), hs.end()), hs.end());
  for (uint64_t h : hs) {
    CkHdr x;
    x.hdr = h;
    x.src = h / 8;
    x.len = (uint32_t)std::min<uint64_t>(kCkHdrBytesMax, n - x.src);  // (validated: h < a pos <= 8 n)
    x.slot = p.in_total;
    p.in_total += kCkHdrSlot;
    p.in_bytes += x.len;
    p.hdrs.push_back(x);
  }
  // only the stream's first segment may lie at decode offset 0: expand_kernel
  // lets every other segment reach 32 KiB behind its start (into its window)
  if (!p.spans.empty() && p.spans[0].first != 0) p.dec_total = 256;
  for (CkSpan &s : p.spans) {
    s.unit0 = (uint32_t)p.units.size();
    s.in_pos = p.in_total = align_up(p.in_total, 64);
    s.in_len = std::min<uint64_t>((v.e[s.last + 1].pos + 7) / 8, v.end_ip) - s.byte0;
    s.out_pos = p.dec_total = align_up(p.dec_total, 256);
    s.out_len = out_of(s.last + 1) - out_of(s.first);
    // a bit position or header of this span's units, in the packed input
    auto reloc = [&](uint64_t pos) { return pos - s.byte0 * 8 + s.in_pos * 8; };
    auto reloc_hdr = [&](uint64_t h) -> uint64_t {
      if (h == kCkFixedHdr) return h;
      if (h / 8 >= s.byte0) return reloc(h);
      const size_t i = (size_t)(std::lower_bound(hs.begin(), hs.end(), h) - hs.begin());
      return p.hdrs[i].slot * 8 + (h & 7);
    };
    SegLayout lay(p.chain, p.segs, p.desc_total);
    for (uint32_t u = s.first; u <= s.last; ++u) {
      const CkEntry &e = v.e[u], &nx = v.e[u + 1];
      CkUnit j{};
      j.entry = u;
      j.pos = reloc(e.pos);
      j.hdr = e.kind == CK_HUFF ? reloc_hdr(e.hdr) : 0;
      j.kind = e.kind;
      j.rem = e.rem;
      j.bfinal = (e.flags >> 1) & 1u;
      j.stop = u + 1 == v.nunits ? kCkNoStop : reloc(nx.pos);
      j.e_pos = reloc(nx.pos);
      j.e_hdr = nx.kind == CK_HUFF ? reloc_hdr(nx.hdr) : 0;
      j.e_kind = nx.kind;
      j.e_rem = nx.rem;
      j.e_bfinal = (nx.flags >> 1) & 1u;
      j.ntok = e.ntok;
      j.out_len = (uint32_t)(nx.out_off - e.out_off);  // (validated: fits its tokens, < 2^32)
      j.tok_off = p.tok_total;
      j.tok_cap = e.ntok;
      p.tok_total += align_up((uint64_t)e.ntok + 1, 64);
      // a segment that starts at a window entry starts from that window
      if (lay.add(j.tok_off, s.out_pos + (e.out_off - out_of(s.first)), e.ntok, j.out_len, e.flags & 1u)) {
        p.seg_win.push_back((e.flags & 1u) ? (int32_t)p.wins.size() : -1);
        if (e.flags & 1u) p.wins.push_back(e.win);
      }
      p.units.push_back(j);
    }
    p.in_total += s.in_len;
    p.in_bytes += s.in_len;
    p.dec_total += s.out_len;
    p.dec_bytes += s.out_len;
  }
  range_place(p.spans, out_of, &p);
  return p;
}

}  // namespace zt
