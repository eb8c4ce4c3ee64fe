// Host model of the lane-parallel parse walk of csrc/deflate_post.hip
// (parse_block_lanes): lanes as arrays, the same lane_walk and the same
// entry-resolution loop, checked against the serial walk on random and
// adversarial length arrays.  Prints the distribution of resolution rounds
// per step.  No GPU:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -o parse_lanes_model parse_lanes_model.cpp && ./parse_lanes_model
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

constexpr uint32_t PL_LANE = 32, PL_STEP = 64 * PL_LANE;

// (as in deflate_post.hip; row[j]: the length at the lane's position j, 0 or 3..258)
static void lane_walk(const uint32_t *row, uint32_t mm, uint32_t e, uint32_t old, uint32_t &path, uint32_t &ex) {
  uint32_t p = 0, cur = e;
  bool merged = false;
  while (cur < PL_LANE) {
    const uint32_t from = ~0u << cur;
    const uint32_t rest = mm & from;
    const uint32_t m = rest ? (uint32_t)__builtin_ctz(rest) : 32u;
    const uint32_t below = m >= 32 ? ~0u : (1u << m) - 1;
    const uint32_t upto = m >= 31 ? ~0u : (2u << m) - 1;
    if (old & from & upto) {
      p |= (below | old) & from;
      merged = true;
      break;
    }
    p |= below & from;
    cur = m;
    if (m < 32) {
      p |= 1u << m;
      cur = m + row[m];
    }
  }
  path = p;
  if (!merged) ex = cur;
}

static std::map<int, uint64_t> g_rounds;

// the path positions of one sequence of lengths L[0..len), by steps of 64 lanes
static std::vector<uint8_t> lanes_walk(const std::vector<uint32_t> &L) {
  const uint32_t len = (uint32_t)L.size();
  std::vector<uint8_t> onpath(len, 0);
  uint32_t entry = 0;
  for (uint32_t t = 0; t * PL_STEP < len; ++t) {
    uint32_t row[64][PL_LANE], mm[64], vm[64], a[64], path[64], ex[64], nxt[64], ent[64] = {};
    bool on[64];
    const uint32_t rel = entry - t * PL_STEP, src = rel / PL_LANE, soff = rel % PL_LANE, send = (t + 1) * PL_STEP;
    if (rel >= PL_STEP) abort();
    for (uint32_t k = 0; k < 64; ++k) {
      const uint32_t pos0 = t * PL_STEP + k * PL_LANE;
      const uint32_t nvalid = pos0 < len ? (len - pos0 < PL_LANE ? len - pos0 : PL_LANE) : 0;
      vm[k] = nvalid >= 32 ? ~0u : (1u << nvalid) - 1;
      mm[k] = 0;
      for (uint32_t j = 0; j < PL_LANE; ++j) {
        row[k][j] = pos0 + j < len ? L[pos0 + j] : 0;
        mm[k] |= (row[k][j] >= 3 ? 1u : 0u) << j;
      }
      mm[k] &= vm[k];
      a[k] = k == src ? soff : 0;
      path[k] = 0;
      ex[k] = PL_LANE;
      lane_walk(row[k], mm[k], a[k], 0, path[k], ex[k]);
      path[k] &= vm[k];
    }
    int round = 0;
    for (;; ++round) {
      if (round > 64) abort();  // the bound the kernel's loop relies on
      uint32_t ptr[64];
      uint64_t reach[64];
      for (uint32_t k = 0; k < 64; ++k) {
        const uint32_t pos0 = t * PL_STEP + k * PL_LANE;
        nxt[k] = pos0 + ex[k] < send ? k + ex[k] / PL_LANE : 64;
        if (nxt[k] <= k) abort();
        ptr[k] = nxt[k];
        reach[k] = 1ull << k;
      }
      for (int rnd = 0; rnd < 6; ++rnd) {  // pointer jumping, all lanes at once
        uint32_t np[64];
        uint64_t nr[64];
        for (uint32_t k = 0; k < 64; ++k) {
          np[k] = ptr[k];
          nr[k] = reach[k];
          if (ptr[k] < 64) {
            nr[k] |= reach[ptr[k]];
            np[k] = ptr[ptr[k]];
          }
        }
        for (uint32_t k = 0; k < 64; ++k) ptr[k] = np[k], reach[k] = nr[k];
      }
      for (uint32_t k = 0; k < 64; ++k)
        if (ptr[k] < 64) abort();
      bool chain = true;  // every exit in the next lane: the kernel skips the pointer jumping
      for (uint32_t k = 0; k < 63; ++k) chain = chain && nxt[k] == k + 1;
      for (uint32_t k = 0; k < 64; ++k) {
        on[k] = (reach[src] >> k) & 1;
        if (chain && on[k] != (k >= src)) abort();
      }
      for (uint32_t k = 0; k < 64; ++k)
        if (on[k] && nxt[k] < 64) ent[nxt[k]] = ex[k] % PL_LANE;
      bool any = false, moved = false;
      for (uint32_t k = 0; k < 64; ++k) {
        const uint32_t te = k == src ? soff : ent[k];
        if (on[k] && te != a[k]) {
          any = true;
          const uint32_t ex0 = ex[k];
          lane_walk(row[k], mm[k], te, path[k], path[k], ex[k]);
          path[k] &= vm[k];
          a[k] = te;
          moved = moved || ex[k] != ex0;
        }
      }
      if (!any || !moved) break;  // no exit moved: the lists and the entries stay
    }
    g_rounds[round + 1]++;
    int nlast = 0;
    for (uint32_t k = 0; k < 64; ++k) {
      const uint32_t pos0 = t * PL_STEP + k * PL_LANE;
      if (!on[k]) continue;
      if (nxt[k] >= 64) {
        entry = pos0 + ex[k];
        ++nlast;
      }
      for (uint32_t j = 0; j < PL_LANE; ++j)
        if ((path[k] >> j) & 1) onpath[pos0 + j] = 1;
    }
    if (nlast != 1) abort();
  }
  return onpath;
}

static std::vector<uint8_t> serial_walk(const std::vector<uint32_t> &L) {
  std::vector<uint8_t> onpath(L.size(), 0);
  for (size_t i = 0; i < L.size(); i += L[i] >= 3 ? L[i] : 1) onpath[i] = 1;
  return onpath;
}

static int check(const std::string &name, const std::vector<uint32_t> &L) {
  g_rounds.clear();
  const bool ok = lanes_walk(L) == serial_walk(L);
  printf("%-28s len %6zu %s  rounds/step:", name.c_str(), L.size(), ok ? "ok  " : "FAIL");
  for (auto &kv : g_rounds) printf(" %d:%llu", kv.first, (unsigned long long)kv.second);
  printf("\n");
  return ok ? 0 : 1;
}

int main() {
  int bad = 0;
  std::mt19937 rng(1);
  const uint32_t lens[] = {1, 31, 32, 33, 2047, 2048, 2049, 4097, 32701, 32768};
  for (uint32_t len : lens) {
    std::vector<uint32_t> L(len);
    // text-like: a match at every third position or so, short lengths
    for (auto &l : L) l = rng() % 3 == 0 ? 3 + rng() % 10 : 0;
    bad += check("text-like", L);
    for (auto &l : L) l = rng() % 2 ? 3 + rng() % 256 : 0;
    bad += check("uniform lengths", L);
    for (auto &l : L) l = 3 + rng() % 3;
    bad += check("all short matches", L);
    for (auto &l : L) l = 0;
    bad += check("all literals", L);
    for (size_t i = 0; i < L.size(); ++i) L[i] = i & 1 ? 258 : 3;
    bad += check("alternating 3 / 258", L);
    for (auto &l : L) l = rng() % 50 == 0 ? 258 : 0;
    bad += check("sparse 258", L);
  }
  // all 258, the path at every phase: the first match after `ph` literals
  std::map<int, uint64_t> all;
  for (uint32_t ph = 0; ph < 258; ++ph) {
    std::vector<uint32_t> L(32768, 258);
    for (uint32_t i = 0; i < ph; ++i) L[i] = 0;
    g_rounds.clear();
    if (lanes_walk(L) != serial_walk(L)) {
      printf("all 258 at phase %u FAIL\n", ph);
      ++bad;
    }
    for (auto &kv : g_rounds) all[kv.first] += kv.second;
  }
  printf("%-28s len %6d %s  rounds/step:", "all 258, phases 0..257", 32768, "    ");
  for (auto &kv : all) printf(" %d:%llu", kv.first, (unsigned long long)kv.second);
  printf("\n%s\n", bad ? "FAILED" : "all ok");
  return bad ? 1 : 0;
}
