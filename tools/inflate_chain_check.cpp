// tools/inflate_chain_check.cpp -- drives the host-only chain logic of the
// two-phase inflate (zlib.ts_amd/csrc/inflate_chain.h) without a device:
// seg_chain_host and batch_chain_host over hand-made unit tables, the layout
// checked field by field.  Meant to be built with a sanitizer and run on its
// own (tests/test_container_batch_host.py):
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o inflate_chain_check tools/inflate_chain_check.cpp
//   ./inflate_chain_check
//
// Every table is a heap allocation of exactly its entries (restart flags:
// units - 1), so a read outside it stops the run.  Prints
// "inflate_chain_check ok"; exit 1 on a broken invariant.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../zlib.ts_amd/csrc/inflate_chain.h"

using namespace zt;

static int fails = 0;
#define CHECK(c)                                      \
  do {                                                \
    if (!(c)) {                                       \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
      ++fails;                                        \
    }                                                 \
  } while (0)

constexpr uint32_t kDirect = 3u << 30;  // TokResult::ntok: stored runs only
constexpr uint32_t kRuns = 1u << 30;    // the bit a mixed segment clears

struct Tables {
  std::vector<TokResult> res;
  std::vector<uint8_t> restart;  // units - 1
  std::vector<uint64_t> tok_off;
  ChainPlan run() const {
    // (exact-size copies: vectors may have spare capacity the sanitizer does not guard)
    TokResult *r = new TokResult[res.size()];
    uint8_t *f = new uint8_t[restart.size()];
    uint64_t *t = new uint64_t[tok_off.size()];
    std::copy(res.begin(), res.end(), r);
    std::copy(restart.begin(), restart.end(), f);
    std::copy(tok_off.begin(), tok_off.end(), t);
    ChainPlan p = seg_chain_host(r, f, t, res.size());
    delete[] r;
    delete[] f;
    delete[] t;
    return p;
  }
};

// `units` units, every one on the chain (unit u stops at sync point u, the
// last at BFINAL), unit u with out_len[u] bytes, 10 + u tokens, slot 1000 u
static Tables chain_of(const std::vector<uint64_t> &out_len) {
  Tables T;
  const size_t n = out_len.size();
  for (size_t u = 0; u < n; ++u) {
    TokResult r{};
    r.out_len = out_len[u];
    r.end_bits = 8000 * (u + 1) + 3;
    r.ntok = 10 + (uint32_t)u;
    r.status = ZT_OK;
    r.stop_idx = u + 1 < n ? (int32_t)u : -1;
    T.res.push_back(r);
    T.tok_off.push_back(1000 * u);
  }
  T.restart.assign(n ? n - 1 : 0, 0);
  return T;
}

static void check_unit(const ChainPlan &p, size_t k, uint32_t unit, uint64_t out_off, uint64_t seg_off,
                       uint64_t desc_off, uint32_t ntok, uint32_t out_len, int line) {
  const bool ok = k < p.chain.size() && p.on_chain[k] == unit && p.chain[k].tok_off == 1000ull * unit &&
                  p.chain[k].out_off == out_off && p.chain[k].seg_off == seg_off && p.chain[k].desc_off == desc_off &&
                  p.chain[k].ntok == ntok && p.chain[k].out_len == out_len;
  if (!ok) {
    fprintf(stderr, "line %d: chain unit %zu differs\n", line, k);
    ++fails;
  }
}
#define UNIT(...) check_unit(__VA_ARGS__, __LINE__)

static void one_unit() {
  Tables T = chain_of({77});
  const ChainPlan p = T.run();
  CHECK(p.outcome == ChainPlan::kBuilt && p.why.empty());
  CHECK(p.chain.size() == 1 && p.segs.size() == 1 && p.last == 0);
  CHECK(p.total == 77 && p.desc_total == 77);
  UNIT(p, 0, 0, 0, 0, 0, 10, 77);
  CHECK(p.segs[0].first == 0 && p.segs[0].count == 1);
  // an empty stream: one empty unit is a direct segment
  T = chain_of({0});
  const ChainPlan e = T.run();
  CHECK(e.outcome == ChainPlan::kBuilt && e.total == 0 && e.desc_total == 0);
  CHECK(e.segs.size() == 1 && e.segs[0].count == (1u | 0x80000000u));
}

static void skips_false_candidates() {
  // units 1, 2 and 4 are false candidates: 0 -> 3 -> 5
  Tables T = chain_of({100, 5, 6, 200, 7, 300});
  T.res[0].stop_idx = 2;
  T.res[3].stop_idx = 4;
  T.res[1].status = ZT_E_INPUT_BROKEN;  // (off the chain: never looked at)
  T.restart[2] = 1;                     // unit 3 follows a restart point
  const ChainPlan p = T.run();
  CHECK(p.outcome == ChainPlan::kBuilt);
  CHECK(p.chain.size() == 3 && p.last == 5 && p.total == 600);
  UNIT(p, 0, 0, 0, 0, 0, 10, 100);
  UNIT(p, 1, 3, 100, 100, 512, 13, 200);
  UNIT(p, 2, 5, 300, 100, 712, 15, 300);
  CHECK(p.segs.size() == 2);
  CHECK(p.segs[0].first == 0 && p.segs[0].count == 1);
  CHECK(p.segs[1].first == 1 && p.segs[1].count == 2);
  CHECK(p.desc_total == 512 + 500);
}

static void restart_flags_and_empty_units() {
  // unit 0 is the stream start (a segment start whatever the flags say); a
  // restart point at unit 1 right behind an empty unit 0 merges: no empty segment
  Tables T = chain_of({0, 0, 40, 0, 0, 50, 60});
  T.restart[0] = 1;  // unit 1
  T.restart[1] = 1;  // unit 2: consecutive restart points, still nothing written
  T.restart[3] = 1;  // unit 4: 40 bytes since the segment start -> a new segment
  T.restart[4] = 1;  // unit 5: right behind it, unit 4 was empty -> merges
  const ChainPlan p = T.run();
  CHECK(p.outcome == ChainPlan::kBuilt);
  CHECK(p.chain.size() == 7 && p.total == 150);
  CHECK(p.segs.size() == 2);
  CHECK(p.segs[0].first == 0 && p.segs[0].count == 4);
  CHECK(p.segs[1].first == 4 && p.segs[1].count == 3);
  UNIT(p, 2, 2, 0, 0, 0, 12, 40);
  UNIT(p, 3, 3, 40, 0, 40, 13, 0);
  UNIT(p, 4, 4, 40, 40, 512, 14, 0);
  UNIT(p, 5, 5, 40, 40, 512, 15, 50);
  UNIT(p, 6, 6, 90, 40, 562, 16, 60);
  CHECK(p.desc_total == 512 + 110);
}

static void direct_and_mixed_segments() {
  // segment 0: stored runs and an empty unit -> direct; segment 1: one unit
  // of stored runs beside a Huffman unit -> mixed, bit 30 cleared
  Tables T = chain_of({1024, 0, 2048, 4096, 10});
  T.res[0].ntok = kDirect | 3;
  T.res[1].ntok = 0;
  T.res[2].ntok = kDirect | 3;
  T.res[3].ntok = kDirect | 6;
  T.res[4].ntok = (1u << 31) | 9;
  T.restart[2] = 1;  // unit 3
  const ChainPlan p = T.run();
  CHECK(p.outcome == ChainPlan::kBuilt && p.segs.size() == 2);
  CHECK(p.segs[0].first == 0 && p.segs[0].count == (3u | 0x80000000u));
  CHECK(p.segs[1].first == 3 && p.segs[1].count == 2);
  CHECK(p.chain[0].ntok == (kDirect | 3) && p.chain[1].ntok == 0 && p.chain[2].ntok == (kDirect | 3));
  CHECK(p.chain[3].ntok == ((kDirect | 6) & ~kRuns));
  CHECK(p.chain[4].ntok == ((1u << 31) | 9));
  UNIT(p, 3, 3, 3072, 3072, 3072, (1u << 31) | 6, 4096);
}

static void fallbacks() {
  // more than 4 GiB from one unit
  Tables T = chain_of({10, 0x100000000ull, 10});
  ChainPlan p = T.run();
  CHECK(p.outcome == ChainPlan::kFallback);
  CHECK(p.why == "unit 1 (chain 1): status 0 detail 0 ntok 11 out 4294967296\n");
  T.res[1].out_len = 0xFFFFFFFFull;  // (the largest one that stays)
  p = T.run();
  CHECK(p.outcome == ChainPlan::kBuilt && p.total == 0xFFFFFFFFull + 20);
  UNIT(p, 2, 2, 0xFFFFFFFFull + 10, 0, 0xFFFFFFFFull + 10, 12, 10);
  // a stop that does not move forward, and one past the tables
  T = chain_of({10, 20, 30});
  T.res[1].stop_idx = 0;  // next unit 1 <= 1
  p = T.run();
  CHECK(p.outcome == ChainPlan::kFallback && p.why == "unit 1: bad stop 0\n");
  T.res[1].stop_idx = 2;  // next unit 3 >= units
  p = T.run();
  CHECK(p.outcome == ChainPlan::kFallback && p.why == "unit 1: bad stop 2\n");
  // a status in the middle of the chain
  T = chain_of({10, 20, 30});
  T.res[1].status = ZT_E_INPUT_BROKEN;
  T.res[1].detail = 4;
  p = T.run();
  CHECK(p.outcome == ChainPlan::kFallback);
  char want[160];
  snprintf(want, sizeof want, "unit 1 (chain 1): status %d detail 4 ntok 11 out 20\n", ZT_E_INPUT_BROKEN);
  CHECK(p.why == want);
  // any other status in the last unit
  T = chain_of({10, 20, 30});
  T.res[2].status = ZT_E_INVALID_DISTANCE;
  p = T.run();
  CHECK(p.outcome == ChainPlan::kFallback && p.last == 2);
}

static void ran_out_of_input() {
  const int codes[2] = {ZT_E_INPUT_BROKEN, ZT_E_STORED_LEN};
  for (const int code : codes) {
    Tables T = chain_of({10, 20, 30});
    T.res[2].status = code;
    ChainPlan p = T.run();
    CHECK(p.outcome == ChainPlan::kTruncated && p.last == 2);
    CHECK(p.why == "chain ran out of input in its last unit 2\n");
    // the chain jumps over a false candidate into the last unit
    T.res[0].stop_idx = 1;
    p = T.run();
    CHECK(p.outcome == ChainPlan::kTruncated && p.last == 2);
    // a single unit has no chain to grow a window for: a fallback
    T = chain_of({10});
    T.res[0].status = code;
    p = T.run();
    CHECK(p.outcome == ChainPlan::kFallback);
    char want[160];
    snprintf(want, sizeof want, "unit 0 (chain 0): status %d detail 0 ntok 10 out 10\n", code);
    CHECK(p.why == want);
  }
}

static void batch_chain() {
  std::vector<TokResult> res;
  std::vector<uint64_t> tok_off;
  auto add = [&](uint64_t out_len, uint32_t ntok, int status, int stop_idx) {
    TokResult r{};
    r.out_len = out_len;
    r.end_bits = 100 * (res.size() + 1);
    r.ntok = ntok;
    r.status = status;
    r.stop_idx = stop_idx;
    res.push_back(r);
    tok_off.push_back(4096 * tok_off.size());
  };
  add(1000, 50, ZT_OK, -1);                  // 0
  add(0, 0, ZT_OK, -1);                      // 1: empty output, reserves 256 bytes
  add(5, 2, ZT_E_INVALID_SYMBOL, -1);        // 2: failed
  add(2048, kDirect | 3, ZT_OK, -1);         // 3: stored runs only
  add(10, 4, ZT_OK, 0);                      // 4: stopped at a sync point, not at BFINAL
  add(0x100000000ull, 9, ZT_OK, -1);         // 5: too long for one unit
  add(257, (1u << 31) | 7, ZT_OK, -1);       // 6
  TokResult *r = new TokResult[res.size()];
  uint64_t *t = new uint64_t[res.size()];
  std::copy(res.begin(), res.end(), r);
  std::copy(tok_off.begin(), tok_off.end(), t);
  const BatchChain b = batch_chain_host(r, t, res.size());
  delete[] r;
  delete[] t;
  CHECK(b.failed == (std::vector<size_t>{2, 4, 5}));
  CHECK(b.who == (std::vector<size_t>{0, 1, 3, 6}));
  CHECK(b.chain.size() == 4 && b.segs.size() == 4);
  const uint64_t out_off[4] = {0, 1024, 1280, 3328}, desc_off[4] = {0, 1024, 1024, 3072};
  const uint32_t count[4] = {1, 1, 0x80000001u, 1};
  for (size_t j = 0; j < b.chain.size() && j < 4; ++j) {
    const ChainUnit &cu = b.chain[j];
    const TokResult &s = res[b.who[j]];
    CHECK(cu.tok_off == 4096 * b.who[j] && cu.ntok == s.ntok && cu.out_len == s.out_len);
    CHECK(cu.out_off == out_off[j] && cu.seg_off == out_off[j] && cu.desc_off == desc_off[j]);
    CHECK(b.segs[j].first == j && b.segs[j].count == count[j]);
  }
  CHECK(b.out_total == 3328 + 512);
  CHECK(b.desc_total == 3072 + 257);
  // nothing decodable: empty chain, everything failed
  TokResult bad{};
  bad.status = ZT_E_UNKNOWN_BTYPE;
  uint64_t zero = 0;
  const BatchChain none = batch_chain_host(&bad, &zero, 1);
  CHECK(none.chain.empty() && none.segs.empty() && none.failed.size() == 1 && none.out_total == 0);
}

int main() {
  one_unit();
  skips_false_candidates();
  restart_flags_and_empty_units();
  direct_and_mixed_segments();
  fallbacks();
  ran_out_of_input();
  batch_chain();
  if (fails) return fprintf(stderr, "inflate_chain_check: %d checks failed\n", fails), 1;
  printf("inflate_chain_check ok\n");
  return 0;
}
