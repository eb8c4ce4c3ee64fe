// index_host.h -- host-only logic of the indexed range inflate
// (include/zt_index.h): the blob layout, its validation, and the planner that
// turns a set of ranges into everything the two-phase kernels need (packed
// input spans, stops, TokJobs, ChainUnits, SegJobs).  No device code and no HIP
// types: tools/index_host_check.cpp runs it under ASan / UBSan.
//
// The index is a hint that is verified, never trusted.  index_validate is the
// first half of that: after it, every offset the planner derives from the
// blob lies inside the caller's input and inside the buffers the plan sizes.
// The second half is range_verify_kernel (index_api.hip), which compares what
// the tokenizer found with what the blob promised.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/zt_index.h"
#include "range_plan.h"

namespace zt {

constexpr size_t kIdxHeader = ZT_INDEX_HEADER_BYTES;
constexpr size_t kIdxEntry = ZT_INDEX_ENTRY_BYTES;
// a unit's token capacity on the sync-point path (inflate_seg.hip: kUnitTokCap,
// asserted equal there): no unit the build accepts holds more
constexpr uint32_t kIdxUnitTokCap = 32768 + 64;
// output bytes one token can stand for (a stored-run token: len << 16)
constexpr uint64_t kIdxTokBytesMax = 65535;

// A planned unit's token slot.  tokenize_kernel bounds a stored block's payload
// by the slot (tokens so far + LEN <= capacity) before it turns a long payload
// into three run tokens, so a slot of exactly `ntok` tokens would refuse every
// stored run: the slot also has room for one stored payload (<= 65535 bytes,
// and no more than the unit's output).  range_verify_kernel compares the
// count itself with the index.
inline uint32_t idx_tok_slot(uint32_t ntok, uint64_t out_len) {
  return ntok + (uint32_t)std::min<uint64_t>(out_len, 65535);
}

// what index_pack_kernel writes per unit (little-endian hosts and devices)
struct IdxEntry {
  uint64_t in_off;
  uint64_t out_off;
  uint32_t ntok;
  uint32_t flags;
};
static_assert(sizeof(IdxEntry) == kIdxEntry, "entry layout is the interface");

inline void idx_put32(uint8_t *p, uint32_t v) {
  for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
inline void idx_put64(uint8_t *p, uint64_t v) {
  for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
inline uint32_t idx_get32(const uint8_t *p) {
  uint32_t v = 0;
  for (int k = 0; k < 4; ++k) v |= (uint32_t)p[k] << (8 * k);
  return v;
}
inline uint64_t idx_get64(const uint8_t *p) {
  uint64_t v = 0;
  for (int k = 0; k < 8; ++k) v |= (uint64_t)p[k] << (8 * k);
  return v;
}

inline size_t index_blob_bytes(size_t nunits) { return kIdxHeader + (nunits + 1) * kIdxEntry; }

inline void index_write_header(uint8_t *blob, uint32_t nunits, uint32_t nseg, uint64_t stream_start, uint64_t end_ip,
                               uint64_t total_out) {
  memset(blob, 0, kIdxHeader);
  memcpy(blob, "ZTIX", 4);
  idx_put32(blob + 4, ZT_INDEX_VERSION);
  idx_put32(blob + 8, nunits);
  idx_put32(blob + 12, nseg);
  idx_put64(blob + 16, stream_start);
  idx_put64(blob + 24, end_ip);
  idx_put64(blob + 32, total_out);
}
inline void index_write_entry(uint8_t *blob, size_t k, const IdxEntry &e) {
  uint8_t *p = blob + kIdxHeader + k * kIdxEntry;
  idx_put64(p, e.in_off);
  idx_put64(p + 8, e.out_off);
  idx_put32(p + 16, e.ntok);
  idx_put32(p + 20, e.flags);
}

// A validated index, parsed: nunits + 1 entries (the sentinel last).
struct IndexView {
  uint32_t nunits = 0, nseg = 0;
  uint64_t stream_start = 0, end_ip = 0, total_out = 0;
  std::vector<uint64_t> in_off, out_off;
  std::vector<uint32_t> ntok, flags;
  std::vector<uint32_t> seg_units;  // the flagged units, ascending
};

// Checks the blob against itself and against the input length `n`.  Returns
// null and fills *v, or a one-line reason.
inline const char *index_validate(const uint8_t *idx, size_t idx_len, size_t n, IndexView *v) {
  if (!idx || idx_len < kIdxHeader + 2 * kIdxEntry) return "index truncated";
  if (memcmp(idx, "ZTIX", 4) != 0) return "not an index (magic)";
  if (idx_get32(idx + 4) != ZT_INDEX_VERSION) return "unknown index version";
  const uint64_t nunits = idx_get32(idx + 8);
  if (nunits == 0 || (idx_len - kIdxHeader) % kIdxEntry != 0 || (idx_len - kIdxHeader) / kIdxEntry != nunits + 1)
    return "index length does not match its unit count";
  v->nunits = (uint32_t)nunits;
  v->nseg = idx_get32(idx + 12);
  v->stream_start = idx_get64(idx + 16);
  v->end_ip = idx_get64(idx + 24);
  v->total_out = idx_get64(idx + 32);
  for (size_t k = 40; k < kIdxHeader; ++k)
    if (idx[k]) return "index header padding is not zero";
  if (v->stream_start > v->end_ip || v->end_ip > n) return "index positions lie outside the input";
  v->in_off.resize(nunits + 1);
  v->out_off.resize(nunits + 1);
  v->ntok.resize(nunits + 1);
  v->flags.resize(nunits + 1);
  v->seg_units.clear();
  for (size_t k = 0; k <= nunits; ++k) {
    const uint8_t *p = idx + kIdxHeader + k * kIdxEntry;
    v->in_off[k] = idx_get64(p);
    v->out_off[k] = idx_get64(p + 8);
    v->ntok[k] = idx_get32(p + 16);
    v->flags[k] = idx_get32(p + 20);
  }
  if (v->in_off[0] != v->stream_start || v->out_off[0] != 0) return "index does not start at the stream start";
  if (!(v->flags[0] & 1)) return "first unit is not a segment start";
  if (v->in_off[nunits] != v->end_ip || v->out_off[nunits] != v->total_out || v->ntok[nunits] || v->flags[nunits])
    return "index sentinel is wrong";
  for (size_t k = 0; k < nunits; ++k) {
    if (v->in_off[k] > v->in_off[k + 1] || v->out_off[k] > v->out_off[k + 1]) return "index offsets decrease";
    if (v->in_off[k] < v->stream_start || v->in_off[k + 1] > v->end_ip) return "index positions lie outside the input";
    if (v->flags[k] & ~1u) return "unknown index flags";
    if (v->ntok[k] > kIdxUnitTokCap) return "unit token count over the unit capacity";
    if (v->out_off[k + 1] - v->out_off[k] > (uint64_t)v->ntok[k] * kIdxTokBytesMax)
      return "unit output larger than its tokens can produce";
    if (v->flags[k] & 1) v->seg_units.push_back((uint32_t)k);
  }
  if (v->seg_units.size() != v->nseg) return "index segment count is wrong";
  return nullptr;
}

// ---- the planner ---------------------------------------------------------------
// (the ranges, the spans and the totals: range_plan.h.  A span's `first` is a
// segment start; in_pos is where in_off[first] lies in the packed input and
// in_len = in_off[last + 1] - in_off[first].)
struct RangePlan : RangePlanCore {
  std::vector<RangeSpan> spans;
  // per planned unit (all spans, in stream order)
  std::vector<uint64_t> stops;   // packed position where the unit ends (= the next unit's start): sorted
  std::vector<TokJob> jobs;
  uint32_t final_unit = 0xFFFFFFFFu;  // the planned unit that is the stream's last (ends at BFINAL), if planned
};

inline RangePlan index_plan(const IndexView &v, const uint64_t *off, const uint64_t *len, size_t count) {
  RangePlan p;
  auto out_of = [&](uint32_t k) { return v.out_off[k]; };
  p.spans = range_spans<RangeSpan>(v.total_out, v.seg_units, v.nunits, out_of, off, len, count, &p.ranges);
  // the tables of every span's units
  for (RangeSpan &s : p.spans) {
    s.unit0 = (uint32_t)p.jobs.size();
    s.in_pos = p.in_total = align_up(p.in_total, 64);
    s.in_len = v.in_off[s.last + 1] - v.in_off[s.first];
    s.out_pos = p.dec_total = align_up(p.dec_total, 256);
    s.out_len = v.out_off[s.last + 1] - v.out_off[s.first];
    SegLayout lay(p.chain, p.segs, p.desc_total);
    for (uint32_t u = s.first; u <= s.last; ++u) {
      TokJob j;
      j.start = s.in_pos + (v.in_off[u] - v.in_off[s.first]);
      j.tok_off = p.tok_total;
      const uint64_t ol64 = v.out_off[u + 1] - v.out_off[u];
      j.tok_cap = idx_tok_slot(v.ntok[u], ol64);
      j.stop_first = (uint32_t)p.stops.size();
      j.end = s.in_pos + s.in_len;
      // (validated: the unit's output fits its tokens, < 2^32)
      lay.add(j.tok_off, s.out_pos + (v.out_off[u] - v.out_off[s.first]), v.ntok[u], (uint32_t)ol64, v.flags[u] & 1);
      p.stops.push_back(s.in_pos + (v.in_off[u + 1] - v.in_off[s.first]));
      if (u + 1 == v.nunits) p.final_unit = (uint32_t)p.jobs.size();
      p.jobs.push_back(j);
      p.tok_total += j.tok_cap;
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
