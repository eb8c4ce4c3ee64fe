// tools/index_host_check.cpp -- drives the host-only half of the indexed range
// inflate (zlib.ts_amd/csrc/index_host.h) without a device: the validation of
// an index blob and the planner that turns ranges into spans, jobs, stops,
// chain units and segments.  Meant to be built with a sanitizer and run on its
// own (tests/test_index_host.py):
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o index_host_check tools/index_host_check.cpp
//   ./index_host_check
//
// Every blob is a heap allocation of exactly its bytes, so a read outside it
// stops the run.  Prints "index_host_check ok"; exit 1 on a broken invariant.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../zlib.ts_amd/csrc/index_host.h"

using namespace zt;

static int fails = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      if (fails < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
      ++fails;                                                   \
    }                                                            \
  } while (0)

static uint32_t rng_state = 0x2545F491u;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

// 3 segments x 32 units; the last two units of every segment are the two
// empty units of a restart marker, and unit 7 of each is empty too
struct Synth {
  std::vector<IdxEntry> e;  // with the sentinel
  uint64_t n = 0;           // input length (a few bytes past end_ip)
  uint32_t nseg = 0;
};
static Synth synth(uint64_t stream_start) {
  Synth s;
  uint64_t in = stream_start, out = 0;
  for (int seg = 0; seg < 3; ++seg) {
    for (int u = 0; u < 32; ++u) {
      const bool empty = u == 7 || u == 30 || u == 31;  // (30, 31: a restart marker's halves)
      const uint32_t ol = empty ? 0 : 1000 + 37 * (uint32_t)u + (seg == 2 && u == 29 ? 5 : 0);
      IdxEntry x;
      x.in_off = in;
      x.out_off = out;
      x.ntok = empty ? 0 : ol / 2 + 3;
      x.flags = u == 0 ? 1u : 0u;
      s.e.push_back(x);
      in += empty ? 5 : ol / 3 + 9;
      out += ol;
    }
    ++s.nseg;
  }
  s.e.push_back(IdxEntry{in, out, 0, 0});
  s.n = in + 4;
  return s;
}
static std::vector<uint8_t> blob_of(const Synth &s, uint64_t stream_start) {
  const size_t nunits = s.e.size() - 1;
  std::vector<uint8_t> b(index_blob_bytes(nunits));
  index_write_header(b.data(), (uint32_t)nunits, s.nseg, stream_start, s.e.back().in_off, s.e.back().out_off);
  for (size_t k = 0; k <= nunits; ++k) index_write_entry(b.data(), k, s.e[k]);
  return b;
}
// validation on a heap copy of exactly `len` bytes
static const char *validate(const std::vector<uint8_t> &b, size_t len, size_t n, IndexView *v) {
  uint8_t *h = (uint8_t *)malloc(len ? len : 1);
  memcpy(h, b.data(), len);
  const char *why = index_validate(h, len, n, v);
  free(h);
  return why;
}

// every invariant of a plan; `n`: the input length the blob was validated against
static void check_plan(const IndexView &v, const RangePlan &p, const uint64_t *off, const uint64_t *len, size_t count,
                       size_t n) {
  CHECK(p.ranges.size() == count);
  CHECK(p.jobs.size() == p.chain.size() && p.jobs.size() == p.stops.size());
  // spans: flagged start, in order, not overlapping or touching, inside the index
  uint64_t units = 0, tok = 0;
  for (size_t k = 0; k < p.spans.size(); ++k) {
    const RangeSpan &s = p.spans[k];
    CHECK(s.first <= s.last && s.last < v.nunits);
    CHECK(v.flags[s.first] & 1);
    if (k) CHECK(s.first > p.spans[k - 1].last + 1);
    CHECK(s.unit0 == units);
    CHECK(s.in_pos % 64 == 0 && s.out_pos % 256 == 0);
    CHECK(s.in_len == v.in_off[s.last + 1] - v.in_off[s.first]);
    CHECK(s.in_pos + s.in_len <= p.in_total && s.out_pos + s.out_len <= p.dec_total);
    if (k) {
      CHECK(s.in_pos >= p.spans[k - 1].in_pos + p.spans[k - 1].in_len);
      CHECK(s.out_pos >= p.spans[k - 1].out_pos + p.spans[k - 1].out_len);
    }
    // what the host copies out of the caller's input
    CHECK(v.in_off[s.first] + s.in_len <= n);
    for (uint32_t u = s.first; u <= s.last; ++u, ++units) {
      const TokJob &j = p.jobs[units];
      const ChainUnit &c = p.chain[units];
      CHECK(j.start == s.in_pos + v.in_off[u] - v.in_off[s.first]);
      CHECK(j.start <= j.end && j.end == s.in_pos + s.in_len && j.end <= p.in_total);
      CHECK(p.stops[units] == s.in_pos + v.in_off[u + 1] - v.in_off[s.first]);
      CHECK(j.stop_first == units);
      // the prefix sum of the slots: ntok plus room for one stored payload (idx_tok_slot)
      const uint64_t ol = v.out_off[u + 1] - v.out_off[u];
      CHECK(j.tok_off == tok && j.tok_cap == v.ntok[u] + (ol < 65535 ? ol : 65535));
      tok += j.tok_cap;
      CHECK(c.tok_off == j.tok_off && c.ntok == v.ntok[u]);
      CHECK(c.out_off == s.out_pos + v.out_off[u] - v.out_off[s.first]);
      CHECK(c.out_len == v.out_off[u + 1] - v.out_off[u]);
      CHECK(c.out_off + c.out_len <= p.dec_total);
      CHECK(c.seg_off <= c.out_off && c.seg_off >= s.out_pos);
      CHECK(c.desc_off + c.out_len <= p.desc_total);
      if (u + 1 == v.nunits) CHECK(p.final_unit == units);
    }
  }
  CHECK(units == p.jobs.size() && tok == p.tok_total);
  for (size_t k = 1; k < p.stops.size(); ++k) CHECK(p.stops[k - 1] <= p.stops[k]);
  // segments: cover the chain in order, each starts 512-aligned in the descriptors
  uint32_t at = 0;
  for (const SegJob &sj : p.segs) {
    CHECK(sj.first == at && sj.count > 0 && !(sj.count >> 31));
    CHECK(p.chain[sj.first].desc_off % 512 == 0);
    for (uint32_t k = 0; k < sj.count; ++k) {
      const ChainUnit &c = p.chain[sj.first + k];
      CHECK(c.seg_off == p.chain[sj.first].out_off);
      CHECK(c.desc_off == p.chain[sj.first].desc_off + (c.out_off - c.seg_off));
    }
    at += sj.count;
  }
  CHECK(at == p.chain.size());
  // ranges
  uint64_t ret = 0;
  for (size_t i = 0; i < count; ++i) {
    const PlannedRange &r = p.ranges[i];
    CHECK(r.dst % 256 == 0 && r.dst + r.len <= p.dst_total);
    if (i) CHECK(r.dst >= p.ranges[i - 1].dst + (p.ranges[i - 1].len ? p.ranges[i - 1].len : 1));
    if (off[i] > v.total_out) {
      CHECK(r.status == ZT_E_ARG && r.span < 0 && r.len == 0);
      continue;
    }
    CHECK(r.status == ZT_OK);
    CHECK(r.len == std::min<uint64_t>(len[i], v.total_out - off[i]));
    ret += r.len;
    if (r.len == 0) {
      CHECK(r.span < 0);
      continue;
    }
    CHECK(r.span >= 0 && (size_t)r.span < p.spans.size());
    const RangeSpan &s = p.spans[r.span];
    // the span covers the range: it starts at or before the range's own
    // segment start and ends at or after the unit holding its last byte
    CHECK(v.out_off[s.first] <= r.off);
    CHECK(r.off + r.len <= v.out_off[s.last + 1]);
    CHECK(r.src == s.out_pos + (r.off - v.out_off[s.first]));
    CHECK(r.src + r.len <= s.out_pos + s.out_len);
  }
  CHECK(ret == p.ret_bytes);
}

// one range alone: the span is exactly [last segment start <= off, unit holding the last byte]
static void check_single(const IndexView &v, uint64_t off, uint64_t len, size_t n) {
  const RangePlan p = index_plan(v, &off, &len, 1);
  check_plan(v, p, &off, &len, 1, n);
  const uint64_t cl = off <= v.total_out ? std::min<uint64_t>(len, v.total_out - off) : 0;
  if (cl == 0) {
    CHECK(p.spans.empty() && p.jobs.empty());
    return;
  }
  CHECK(p.spans.size() == 1);
  if (p.spans.size() != 1) return;
  uint32_t first = 0, last = 0;
  for (uint32_t u = 0; u < v.nunits; ++u) {
    if ((v.flags[u] & 1) && v.out_off[u] <= off) first = u;
    if (v.out_off[u] <= off + cl - 1 && off + cl - 1 < v.out_off[u + 1]) last = u;
  }
  CHECK(p.spans[0].first == first && p.spans[0].last == last);
}

int main() {
  const uint64_t start = 10;
  const Synth s = synth(start);
  const std::vector<uint8_t> blob = blob_of(s, start);
  const size_t nunits = s.e.size() - 1;
  IndexView v;
  CHECK(validate(blob, blob.size(), s.n, &v) == nullptr);
  CHECK(v.nunits == nunits && v.nseg == 3 && v.total_out == s.e.back().out_off && v.stream_start == start);

  // ---- validator ---------------------------------------------------------------
  {
    IndexView w;
    for (size_t len : {(size_t)0, (size_t)3, (size_t)63, (size_t)64, (size_t)87, blob.size() - 24, blob.size() - 1})
      CHECK(validate(blob, len, s.n, &w) != nullptr);  // truncated
    std::vector<uint8_t> longer = blob;
    longer.resize(blob.size() + 24);
    CHECK(validate(longer, longer.size(), s.n, &w) != nullptr);
    auto broken = [&](size_t at, uint64_t val, int bytes, size_t n) {
      std::vector<uint8_t> b = blob;
      for (int k = 0; k < bytes; ++k) b[at + k] = (uint8_t)(val >> (8 * k));
      return validate(b, b.size(), n, &w) != nullptr;
    };
    auto entry = [&](size_t k) { return kIdxHeader + k * kIdxEntry; };
    CHECK(broken(0, 'Y', 1, s.n));                                    // magic
    CHECK(broken(4, 2, 4, s.n));                                      // version
    CHECK(broken(8, nunits - 1, 4, s.n));                             // nunits
    CHECK(broken(8, nunits + 1, 4, s.n));
    CHECK(broken(8, 0, 4, s.n));
    CHECK(broken(8, 0xFFFFFFFFu, 4, s.n));
    CHECK(broken(12, 2, 4, s.n));                                     // nseg
    CHECK(broken(entry(5), s.e[6].in_off + 1, 8, s.n));               // decreasing in_off
    CHECK(broken(entry(5) + 8, s.e[6].out_off + 1, 8, s.n));          // decreasing out_off
    CHECK(broken(entry(5), ~0ull, 8, s.n));                           // past n
    CHECK(broken(entry(3), start - 1, 8, s.n));                       // before the stream start
    CHECK(broken(entry(0) + 20, 0, 4, s.n));                          // unflagged entry 0
    CHECK(broken(entry(2) + 20, 2, 4, s.n));                          // unknown flag
    CHECK(broken(entry(2) + 16, kIdxUnitTokCap + 1, 4, s.n));         // token count over the capacity
    CHECK(broken(entry(7) + 16, 0, 4, s.n) == false);                 // (an empty unit has no tokens)
    CHECK(broken(entry(2) + 16, 0, 4, s.n));                          // output without tokens
    CHECK(broken(entry(nunits) + 16, 1, 4, s.n));                     // sentinel
    CHECK(broken(24, s.e.back().in_off + 1, 8, s.n));                 // end_ip against the sentinel
    CHECK(broken(32, s.e.back().out_off - 1, 8, s.n));                // total_out against the sentinel
    CHECK(broken(40, 1, 1, s.n));                                     // padding
    CHECK(validate(blob, blob.size(), (size_t)s.e.back().in_off - 1, &w) != nullptr);  // n cut below end_ip
    CHECK(validate(blob, blob.size(), (size_t)s.e.back().in_off, &w) == nullptr);
  }
  // seeded random mutations: rejected, or accepted with every planner offset in bounds
  {
    size_t accepted = 0;
    for (int it = 0; it < 4000; ++it) {
      std::vector<uint8_t> b = blob;
      const int edits = 1 + (int)(rnd() % 3);
      for (int k = 0; k < edits; ++k) {
        const size_t at = rnd() % b.size();
        switch (rnd() % 4) {
          case 0: b[at] ^= (uint8_t)(1u << (rnd() % 8)); break;
          case 1: b[at] = (uint8_t)rnd(); break;
          case 2: b[at] = 0xFF; break;
          default: b[at] = 0; break;
        }
      }
      size_t len = b.size();
      if (rnd() % 16 == 0) len = rnd() % (b.size() + 1);
      IndexView w;
      if (validate(b, len, s.n, &w) != nullptr) continue;
      ++accepted;
      uint64_t off[8], ln[8];
      for (int k = 0; k < 8; ++k) {
        off[k] = w.total_out ? rnd() % (w.total_out + 2) : 0;
        ln[k] = rnd() % 40000;
      }
      off[7] = 0;
      ln[7] = ~0ull;
      const RangePlan p = index_plan(w, off, ln, 8);
      check_plan(w, p, off, ln, 8, s.n);
    }
    printf("mutations accepted: %zu of 4000\n", accepted);
  }

  // ---- planner -------------------------------------------------------------------
  const uint64_t total = v.total_out;
  for (uint32_t u = 0; u <= v.nunits; ++u) {  // unit and segment edges
    const uint64_t b = v.out_off[u];
    if (b > 0) check_single(v, b - 1, 1, s.n);
    check_single(v, b, 1, s.n);
    if (b > 0) check_single(v, b - 1, 2, s.n);      // crossing the edge
    if (b > 0) check_single(v, b - 1, 3000, s.n);   // crossing several units
  }
  for (uint32_t u : v.seg_units) {
    const uint64_t b = v.out_off[u];
    if (b >= 5000) check_single(v, b - 5000, 10000, s.n);  // crossing a segment edge
  }
  check_single(v, 0, total, s.n);       // the whole output
  check_single(v, 0, ~0ull, s.n);       // clamped
  check_single(v, total - 1, 1, s.n);   // the last byte
  check_single(v, total - 1, 100, s.n);
  check_single(v, total - 3, 100, s.n);
  check_single(v, total, 0, s.n);       // off == total
  check_single(v, total, 5, s.n);
  check_single(v, total + 1, 5, s.n);   // ZT_E_ARG
  check_single(v, 12345, 0, s.n);
  {
    // the whole output: one span from unit 0 to the last unit with output
    // (the synthetic stream ends in two empty units, which no byte needs)
    const uint64_t off = 0, len = total;
    const RangePlan p = index_plan(v, &off, &len, 1);
    uint32_t last = 0;
    for (uint32_t u = 0; u < v.nunits; ++u)
      if (v.out_off[u + 1] > v.out_off[u]) last = u;
    CHECK(last == v.nunits - 3);
    CHECK(p.spans.size() == 1 && p.jobs.size() == last + 1 && p.segs.size() == 3);
    CHECK(p.final_unit == 0xFFFFFFFFu);
    CHECK(p.in_bytes == v.in_off[last + 1] - v.stream_start && p.dec_bytes == total);
  }
  {
    // an index whose last unit has output: planning its last byte plans the stream's final unit
    Synth t = s;
    t.e.resize(t.e.size() - 3);  // drop the two empty units and the sentinel
    const uint64_t in_end = t.e.back().in_off + 400, out_end = t.e.back().out_off + 1000;
    t.e.back().ntok = 600;
    t.e.push_back(IdxEntry{in_end, out_end, 0, 0});
    t.n = in_end;
    const std::vector<uint8_t> b2 = blob_of(t, start);
    IndexView w;
    CHECK(validate(b2, b2.size(), t.n, &w) == nullptr);
    const uint64_t off = w.total_out - 1, len = 1;
    const RangePlan p = index_plan(w, &off, &len, 1);
    check_plan(w, p, &off, &len, 1, t.n);
    CHECK(p.final_unit == p.jobs.size() - 1 && p.spans.size() == 1 && p.spans[0].last == w.nunits - 1);
  }
  for (int round = 0; round < 50; ++round) {  // 64 random overlapping ranges
    uint64_t off[64], len[64];
    for (int k = 0; k < 64; ++k) {
      off[k] = rnd() % (total + 1);
      len[k] = rnd() % 3 == 0 ? rnd() % 200 : rnd() % 30000;
    }
    off[10] = off[3];
    len[10] = len[3];  // a duplicate
    len[20] = 0;
    off[21] = total;
    const RangePlan p = index_plan(v, off, len, 64);
    check_plan(v, p, off, len, 64, s.n);
    CHECK(p.jobs.size() <= v.nunits);
  }
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  puts("index_host_check ok");
  return 0;
}
