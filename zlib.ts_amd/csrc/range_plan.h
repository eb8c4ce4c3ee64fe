// range_plan.h -- what every planner of a range call shares (index_host.h,
// ckpt_host.h): a call's ranges clamped to the output, each mapped to the units
// [start entry at or before its first byte, unit holding its last byte], those
// merged into spans that are decoded once, and every range's place in its span
// and in the packed output.  The segment layout of the spans' units is
// SegLayout (inflate_chain.h).  No device code and no HIP types: the host
// checks under tools/ run it under ASan / UBSan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "inflate_chain.h"

namespace zt {

// One range of a call, clamped.
struct PlannedRange {
  uint64_t off = 0, len = 0;  // len clamped to total_out - off
  int32_t status = ZT_OK;     // ZT_E_ARG: off > total_out
  int32_t span = -1;          // the merged span that decodes it (-1: empty, nothing to decode)
  uint64_t src = 0;           // its first byte in the decode buffer
  uint64_t dst = 0;           // its place in the packed output (256-aligned; an empty range reserves 256 bytes)
};
// Units [first, last] of a blob, decoded as one piece: `first` is a start
// entry, `last` holds the last byte any of its ranges asks for.
struct RangeSpan {
  uint32_t first = 0, last = 0;
  uint32_t unit0 = 0;    // its first planned unit (chain index)
  uint64_t in_pos = 0;   // where its first compressed byte lies in the packed input (64-aligned)
  uint64_t in_len = 0;   // compressed bytes
  uint64_t out_pos = 0;  // where out_off[first] lies in the decode buffer (256-aligned)
  uint64_t out_len = 0;  // out_off[last + 1] - out_off[first]
};
// What every plan holds; a format's plan adds its spans and its unit tables.
struct RangePlanCore {
  std::vector<PlannedRange> ranges;
  // per planned unit (all spans, in stream order), and the units' segments
  std::vector<ChainUnit> chain;
  std::vector<SegJob> segs;
  uint64_t in_total = 0;    // packed input bytes
  uint64_t in_bytes = 0;    // of them, compressed bytes (the rest is alignment)
  uint64_t dec_total = 0;   // decode buffer bytes
  uint64_t dec_bytes = 0;   // of them, decoded bytes
  uint64_t desc_total = 0;  // descriptors
  uint64_t tok_total = 0;   // tokens
  uint64_t dst_total = 0;   // packed output bytes
  uint64_t ret_bytes = 0;   // sum of the clamped lengths
};

// the last k in [0, n) with key(k) <= x (key ascending, key(0) <= x)
template <class Key>
size_t last_at_or_before(size_t n, uint64_t x, Key key) {
  size_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) / 2;
    if (key(mid) <= x)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// Clamps the requests into `ranges` (off, len, status) and returns the spans
// they need, ascending, `first` and `last` set.  starts: the blob's start
// entries, ascending, starts[0] = 0; out_off(k): entry k's output offset,
// k <= nunits (the sentinel's is total_out).
template <class Span, class OutOff>
std::vector<Span> range_spans(uint64_t total_out, const std::vector<uint32_t> &starts, size_t nunits, OutOff out_off,
                              const uint64_t *off, const uint64_t *len, size_t count,
                              std::vector<PlannedRange> *ranges) {
  ranges->resize(count);
  std::vector<Span> want, spans;
  for (size_t i = 0; i < count; ++i) {
    PlannedRange &r = (*ranges)[i];
    r.off = off[i];
    if (r.off > total_out) {
      r.status = ZT_E_ARG;
      continue;
    }
    r.len = std::min<uint64_t>(len[i], total_out - r.off);
    if (r.len == 0) continue;
    Span s;
    // first: the last start entry with out_off <= off (starts[0] = 0 has out_off 0 <= off)
    s.first = starts[last_at_or_before(starts.size(), r.off, [&](size_t k) { return out_off(starts[k]); })];
    // last: the unit that holds byte off + len - 1 (the last entry with out_off <= it; < total_out,
    // so never the sentinel)
    s.last = (uint32_t)last_at_or_before(nunits, r.off + r.len - 1, [&](size_t k) { return out_off((uint32_t)k); });
    want.push_back(s);
  }
  // spans that overlap or touch become one: no unit is decoded twice
  std::sort(want.begin(), want.end(),
            [](const Span &a, const Span &b) { return a.first != b.first ? a.first < b.first : a.last < b.last; });
  for (const Span &s : want) {
    if (!spans.empty() && s.first <= spans.back().last + 1)
      spans.back().last = std::max(spans.back().last, s.last);
    else
      spans.push_back(s);
  }
  return spans;
}

// Every range's place in the packed output and, where it has bytes, its span
// (the last one whose first byte is at or before `off`) and its first byte in
// the decode buffer; the spans' out_pos are set.
template <class Span, class OutOff>
void range_place(const std::vector<Span> &spans, OutOff out_off, RangePlanCore *p) {
  for (PlannedRange &r : p->ranges) {
    r.dst = p->dst_total;
    p->dst_total += align_up(r.len ? r.len : 1, 256);
    if (r.status != ZT_OK || r.len == 0) continue;
    p->ret_bytes += r.len;
    const size_t k = last_at_or_before(spans.size(), r.off, [&](size_t j) { return out_off(spans[j].first); });
    r.span = (int32_t)k;
    r.src = spans[k].out_pos + (r.off - out_off(spans[k].first));
  }
}

}  // namespace zt
