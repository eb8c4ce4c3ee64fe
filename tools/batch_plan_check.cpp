// tools/batch_plan_check.cpp -- drives the host batch layer's arithmetic
// (zlib.ts_amd/csrc/batch_plan.h) without a device: every function against a
// slow re-statement written here, and the fan-out's collection of codes and
// messages against stub shares.  Meant to be built with a sanitizer and run
// on its own (tests/test_container_batch_host.py):
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o batch_plan_check tools/batch_plan_check.cpp
//   ./batch_plan_check
//
// Size tables are heap allocations of exactly their entries, so a read
// outside one stops the run.  Prints "batch_plan_check ok"; exit 1 on a
// broken invariant.
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../zlib.ts_amd/csrc/batch_plan.h"

using namespace zt;

static int fails = 0;
#define CHECK(c)                                      \
  do {                                                \
    if (!(c)) {                                       \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
      ++fails;                                        \
    }                                                 \
  } while (0)

// an exact-size copy (a vector may have spare capacity the sanitizer does not guard)
static std::unique_ptr<size_t[]> exact(const std::vector<size_t> &v) {
  std::unique_ptr<size_t[]> p(new size_t[v.size()]);
  std::copy(v.begin(), v.end(), p.get());
  return p;
}

// ---- LPT ------------------------------------------------------------------------
// slow re-statement: repeatedly take the largest item not yet placed (the
// lowest index among equals) and give it to the device with the least load
// (the lowest index among equals)
static std::vector<std::vector<size_t>> lpt_slow(const std::vector<size_t> &n, size_t nd) {
  std::vector<std::vector<size_t>> share(nd);
  if (nd == 1) {
    for (size_t i = 0; i < n.size(); ++i) share[0].push_back(i);
    return share;
  }
  std::vector<bool> placed(n.size(), false);
  std::vector<uint64_t> load(nd, 0);
  for (size_t round = 0; round < n.size(); ++round) {
    size_t best = n.size();
    for (size_t i = 0; i < n.size(); ++i)
      if (!placed[i] && (best == n.size() || n[i] > n[best])) best = i;
    size_t d = 0;
    for (size_t e = 1; e < nd; ++e)
      if (load[e] < load[d]) d = e;
    placed[best] = true;
    load[d] += n[best] + 4096;
    // ascending insert
    auto &v = share[d];
    v.insert(std::lower_bound(v.begin(), v.end(), best), best);
  }
  return share;
}

static void check_lpt(const std::vector<size_t> &n, size_t nd) {
  const auto p = exact(n);
  const auto got = lpt_shares(p.get(), n.size(), nd);
  CHECK(got == lpt_slow(n, nd));
  CHECK(got.size() == nd);
  std::vector<int> seen(n.size(), 0);
  for (const auto &v : got) {
    for (size_t k = 0; k < v.size(); ++k) {
      CHECK(v[k] < n.size());
      if (v[k] < n.size()) seen[v[k]]++;
      if (k) CHECK(v[k - 1] < v[k]);
    }
  }
  for (int s : seen) CHECK(s == 1);
}

static void test_lpt() {
  for (size_t nd : {size_t(1), size_t(3), size_t(8)}) {
    check_lpt({}, nd);
    check_lpt({7}, nd);
    check_lpt({1024, 70000}, nd);                 // fewer items than devices (nd 3, 8)
    check_lpt(std::vector<size_t>(20, 4096), nd);  // all equal: ties by index
    std::vector<size_t> giant(17, 1000);
    giant[5] = size_t(1) << 30;
    check_lpt(giant, nd);
    std::vector<size_t> mix;
    uint32_t x = 12345;
    for (int i = 0; i < 97; ++i) {
      x = x * 1664525u + 1013904223u;
      mix.push_back((x >> 8) % 300000 * (i % 7 == 0 ? 0 : 1));
    }
    check_lpt(mix, nd);
  }
  // equal sizes on 3 devices: round robin in index order
  const auto p = exact(std::vector<size_t>(7, 100));
  const auto s = lpt_shares(p.get(), 7, 3);
  CHECK((s[0] == std::vector<size_t>{0, 3, 6}));
  CHECK((s[1] == std::vector<size_t>{1, 4}));
  CHECK((s[2] == std::vector<size_t>{2, 5}));
  // one giant: alone on its device
  std::vector<size_t> g{10, 10, 1u << 30, 10, 10};
  const auto pg = exact(g);
  const auto sg = lpt_shares(pg.get(), 5, 3);
  CHECK((sg[0] == std::vector<size_t>{2}));
  CHECK(sg[1].size() == 2 && sg[2].size() == 2);
}

// ---- contiguous cuts --------------------------------------------------------------
static void check_cuts(const std::vector<size_t> &n, size_t nd) {
  const auto p = exact(n);
  const std::vector<size_t> cut = contiguous_cuts(p.get(), n.size(), nd);
  CHECK(cut.size() == nd + 1);
  CHECK(cut.front() == 0 && cut.back() == n.size());
  for (size_t d = 0; d < nd; ++d) CHECK(cut[d] <= cut[d + 1]);  // the shares tile [0, count)
  // slow re-statement: cut d lies behind the first item whose running cost
  // reaches d / nd of the whole (each item closes at most one share)
  uint64_t total = 0;
  for (size_t v : n) total += v + 256;
  std::vector<size_t> want(nd + 1, n.size());
  want[0] = 0;
  size_t d = 1;
  uint64_t acc = 0;
  for (size_t i = 0; i < n.size() && d < nd && nd > 1; ++i) {
    acc += n[i] + 256;
    if (acc * nd >= total * d) want[d++] = i + 1;
  }
  CHECK(cut == want);
}

static void test_cuts() {
  for (size_t nd : {size_t(1), size_t(2), size_t(3), size_t(8)}) {
    check_cuts({}, nd);
    check_cuts({5}, nd);
    check_cuts({1024, 0, 70000}, nd);  // a zero-length item among them
    check_cuts({0, 0, 0, 0}, nd);
    check_cuts(std::vector<size_t>(64, 4096), nd);
    check_cuts({1u << 30, 1, 1, 1, 1, 1, 1, 1, 1, 1}, nd);
  }
  const auto p = exact(std::vector<size_t>(8, 1000));
  CHECK((contiguous_cuts(p.get(), 8, 4) == std::vector<size_t>{0, 2, 4, 6, 8}));
}

// ---- layout, chunks, groups -----------------------------------------------------
static void test_layout() {
  const std::vector<size_t> n{0, 1, 255, 256, 32767, 32768, 32769};
  const auto p = exact(n);
  const std::vector<size_t> ids = iota_ids(n.size());
  struct Case {
    size_t align, min_len;
    std::vector<size_t> room;  // by hand
  };
  const Case cases[] = {
      {256, 1, {256, 256, 256, 256, 32768, 32768, 33024}},
      {256, 0, {0, 256, 256, 256, 32768, 32768, 33024}},
      {32768, 1, {32768, 32768, 32768, 32768, 32768, 32768, 65536}},
  };
  for (const Case &c : cases) {
    const PackLayout L = pack_layout(p.get(), ids, c.align, c.min_len);
    size_t at = 0;
    for (size_t k = 0; k < n.size(); ++k) {
      CHECK(L.off[k] == at);
      CHECK(L.off[k] % c.align == 0);
      at += c.room[k];
    }
    CHECK(L.total == at);
  }
  // a subset, out of order: offsets follow `ids`
  const PackLayout S = pack_layout(p.get(), {6, 2}, 256, 1);
  CHECK((S.off == std::vector<size_t>{0, 33024}) && S.total == 33280);
  CHECK(pack_layout(p.get(), {}, 256, 1).total == 0);
}

static void check_runs(const std::vector<size_t> &room, size_t chunk) {
  std::vector<size_t> off;
  size_t total = 0;
  for (size_t r : room) {
    off.push_back(total);
    total += r;
  }
  const std::vector<size_t> runs = chunk_runs(off, total, chunk);
  CHECK(runs.front() == 0 && runs.back() == room.size());
  for (size_t j = 0; j + 1 < runs.size(); ++j) {
    const size_t a = runs[j], b = runs[j + 1];
    CHECK(a < b);  // no empty run
    size_t bytes = 0;
    for (size_t k = a; k < b; ++k) bytes += room[k];
    // without its last item a run is below the chunk; with it, at or above
    // (but for the last run)
    CHECK(bytes - room[b - 1] < chunk || b == a + 1);
    if (b < room.size()) CHECK(bytes >= chunk);
  }
}

static void test_runs() {
  check_runs({}, 1024);
  CHECK((chunk_runs({}, 0, 1024) == std::vector<size_t>{0}));
  check_runs({256}, 1024);
  check_runs({4096, 256, 256}, 1024);             // an item larger than a chunk
  check_runs({512, 512, 512, 512, 256}, 1024);    // items that end exactly on a chunk
  check_runs({256, 256, 256, 256, 256, 256, 256}, 1024);
  check_runs({256, 8192, 256, 256, 256, 8192}, 1024);
  CHECK((chunk_runs({0, 512, 1024, 1536, 2048}, 2304, 1024) == std::vector<size_t>{0, 2, 4, 5}));
  CHECK((chunk_runs({0, 4096, 4352}, 4608, 1024) == std::vector<size_t>{0, 1, 3}));
}

static void check_groups(const std::vector<size_t> &room, uint64_t target) {
  std::vector<size_t> off;
  uint64_t padded = 0;
  for (size_t r : room) {
    off.push_back(padded);
    padded += r;
  }
  const size_t m = room.size();
  const std::vector<size_t> gk = group_cuts(off, m, padded, target);
  CHECK(gk.front() == 0 && gk.back() == m);
  for (size_t g = 0; g + 1 < gk.size(); ++g) {
    CHECK(gk[g] < gk[g + 1]);  // never empty
    uint64_t bytes = 0;
    for (size_t k = gk[g]; k < gk[g + 1]; ++k) bytes += room[k];
    if (g + 2 < gk.size()) {  // a closed group: at the target with its last item, below without
      CHECK(bytes >= target);
      CHECK(bytes - room[gk[g + 1] - 1] < target);
    }
  }
}

static void test_groups() {
  check_groups({32768, 32768}, 32768);  // m = 2: two groups
  CHECK((group_cuts({0, 32768}, 2, 65536, 32768) == std::vector<size_t>{0, 1, 2}));
  check_groups({32768, 32768}, 1u << 30);  // a target larger than the share: one group
  CHECK((group_cuts({0, 32768}, 2, 65536, 1u << 30) == std::vector<size_t>{0, 2}));
  check_groups({65536, 32768, 32768, 98304, 32768, 32768, 32768}, 98304);
  check_groups(std::vector<size_t>(40, 32768), 5 * 32768);
  check_groups(std::vector<size_t>(41, 32768), 5 * 32768 + 1);
  // the last item never closes a group of its own behind it
  CHECK((group_cuts({0, 32768, 65536}, 3, 98304, 32768) == std::vector<size_t>{0, 1, 2, 3}));
}

// ---- sizes ----------------------------------------------------------------------
static void test_sizes() {
  const size_t ns[] = {0, 1, 65535, 65536, 131070, 131071};
  // by hand: stored blocks of <= 65535 bytes (the empty input is one empty block)
  const size_t blocks[] = {1, 1, 1, 2, 2, 3};
  for (int k = 0; k < 6; ++k) {
    size_t slow = 0, left = ns[k];
    do {  // block by block
      const size_t l = std::min<size_t>(left, 65535);
      slow += 5 + l;
      left -= l;
    } while (left);
    CHECK(stored_len(ns[k]) == slow);
    CHECK(stored_len(ns[k]) == ns[k] + 5 * blocks[k]);
    CHECK(deflate_out_bound(0, ns[k], 999) == slow + 16);
    CHECK(deflate_out_bound(1, ns[k], 999) == 999 + ns[k] / 8 + 64);
    CHECK(deflate_out_bound(2, ns[k], 999) == 999);
  }
  for (uint64_t blk : {uint64_t(1), uint64_t(2), uint64_t(8192), uint64_t(100001)}) {
    const uint64_t p = blk * 32768;
    const uint64_t want = p + p / 8 + 1024 * (blk + 1) + 4096;
    CHECK(batch_out_bound(p) == want);
    CHECK(batch_out_bound(p, 256) == (want + 255) / 256 * 256);
    CHECK(batch_out_bound(p, 256) % 256 == 0 && batch_out_bound(p, 256) >= want);
  }
  for (size_t body : {size_t(0), size_t(1), size_t(45), size_t(46), size_t(63), size_t(64), size_t(100000)}) {
    const size_t s = slab_stride(10, body, 8);
    CHECK(s % 64 == 0 && s > 10 + body + 8 && s <= 10 + body + 8 + 64);
  }
  CHECK(slab_stride(0, 0, 0) == 64 && slab_stride(10, 46, 8) == 128 && slab_stride(10, 45, 8) == 64);
}

// ---- the resolver ---------------------------------------------------------------
static void test_resolver() {
  // by hand: level -> level used (out of 0..9: 6), for lazy = 0 and lazy = 1
  // (levels below 4 become 4; level 0 stays 0 with lazy = 0 and stores)
  const int lv_in[12] = {-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10};
  const int lv_lazy0[12] = {6, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 6};
  const int lv_lazy1[12] = {6, 4, 4, 4, 4, 4, 5, 6, 7, 8, 9, 6};
  for (int ct = -1; ct <= 3; ++ct)
    for (int k = 0; k < 12; ++k)
      for (int lazy = 0; lazy <= 1; ++lazy) {
        zt_deflate_opts o{};
        o.compression_type = ct;
        o.level = lv_in[k];
        o.lazy = lazy;
        int got_ct = -99, got_lv = -99;
        const int rc = resolve_deflate_opts(&o, &got_ct, &got_lv);
        if (ct < 0 || ct > 2) {
          CHECK(rc == ZT_E_INVALID_COMPRESSION_TYPE && got_ct == -99 && got_lv == -99);
          continue;
        }
        CHECK(rc == ZT_OK);
        CHECK(got_lv == (lazy ? lv_lazy1[k] : lv_lazy0[k]));
        // level 0 means stored blocks whatever the type (decided before `lazy` lifts the level)
        CHECK(got_ct == (lv_in[k] == 0 ? 0 : ct));
      }
  int ct = -99, lv = -99;
  CHECK(resolve_deflate_opts(nullptr, &ct, &lv) == ZT_OK && ct == 2 && lv == 6);
}

// ---- the fan-out ----------------------------------------------------------------
static thread_local std::string t_msg;
static const char *last_message() { return t_msg.c_str(); }

static void test_fan_out() {
  for (size_t nd : {size_t(1), size_t(3)}) {
    std::vector<std::vector<size_t>> shares(nd);
    for (size_t d = 0; d < nd; ++d) shares[d] = {d, d + nd};
    t_msg = "the caller's own text";
    // every share fails with its own code after setting its message on its thread
    std::vector<ShareResult> r = fan_out(shares, [&](size_t d) {
      t_msg = "share " + std::to_string(d) + " failed";
      return -100 - (int)d;
    }, last_message);
    CHECK(r.size() == nd);
    for (size_t d = 0; d < nd; ++d) {
      CHECK(r[d].code == -100 - (int)d);
      CHECK(r[d].msg == "share " + std::to_string(d) + " failed");
    }
    if (nd > 1) CHECK(t_msg == "the caller's own text");  // (the shares ran on threads of their own)
    // one share fails: the others report ZT_OK and no text, whatever their thread's message holds
    r = fan_out(shares, [&](size_t d) {
      t_msg = "text of share " + std::to_string(d);
      return d == nd - 1 ? -7 : 0;
    }, last_message);
    for (size_t d = 0; d < nd; ++d) {
      CHECK(r[d].code == (d == nd - 1 ? -7 : 0));
      CHECK(r[d].msg == (d == nd - 1 ? "text of share " + std::to_string(d) : std::string()));
    }
  }
  // an empty share among several is not run
  std::vector<std::vector<size_t>> shares{{0}, {}, {1}};
  std::vector<int> ran(3, 0);
  const std::vector<ShareResult> r = fan_out(shares, [&](size_t d) {
    ran[d] = 1;
    return 0;
  }, last_message);
  CHECK(ran[0] == 1 && ran[1] == 0 && ran[2] == 1 && r[1].code == 0);
}

int main() {
  test_lpt();
  test_cuts();
  test_layout();
  test_runs();
  test_groups();
  test_sizes();
  test_resolver();
  test_fan_out();
  if (fails) {
    fprintf(stderr, "batch_plan_check: %d failures\n", fails);
    return 1;
  }
  printf("batch_plan_check ok\n");
  return 0;
}
