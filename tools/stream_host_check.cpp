// stream_host_check.cpp -- host-only check of the inflate sessions' arithmetic
// (zlib.ts_amd/csrc/stream_host.h), each function against a slow restatement:
// the pending-tail bookkeeping for every end_bits around a feed boundary, the
// decode limit, the pack offsets of a feed call, the output slots and the
// relaunch plan after an output-full stop, the trailing-byte count, the
// Adler-32 combination and the duplicate-session check.
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/stream_host_check.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "../zlib.ts_amd/csrc/batch_plan.h"
#include "../zlib.ts_amd/csrc/stream_host.h"

using namespace zt;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

static uint32_t rng_state = 12345;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

// ---- the pending tail: a model session that holds its bytes as a bit string ------
// A session of `total` fed bytes of which `consumed` bits are decoded keeps
// exactly the bytes that hold an undecoded bit.
static void check_tail() {
  for (size_t m = 0; m <= 40; ++m)
    for (uint64_t end_bits = 0; end_bits <= m * 8; ++end_bits) {
      const SessTail t = sess_tail(m, end_bits);
      // slow: walk the bytes, keep those with a bit at or behind end_bits
      size_t kept = 0, first = m;
      for (size_t b = 0; b < m; ++b)
        if ((uint64_t)(b + 1) * 8 > end_bits) {
          if (!kept) first = b;
          kept++;
        }
      CHECK(t.pending == kept);
      CHECK(t.drop == first);
      CHECK(t.drop + t.pending == m);
      CHECK(t.bit_off == (kept ? end_bits - first * 8 : 0));
      CHECK(t.bit_off < 8);
      // the next launch starts at the same stream bit
      CHECK(t.drop * 8 + t.bit_off == end_bits);
    }
  // a feed boundary: pending | new, consumed up to every bit around the boundary
  for (size_t pend = 0; pend <= 12; ++pend)
    for (size_t add = 0; add <= 12; ++add)
      for (uint64_t e = 0; e <= (pend + add) * 8; ++e) {
        const SessTail t = sess_tail(pend + add, e);
        const bool into_new = e >= pend * 8;
        CHECK((t.drop >= pend) == (into_new || pend == 0));
      }
}

static void check_limit() {
  for (size_t m = 0; m <= 64; ++m) {
    CHECK(sess_limit_bits(m, 1) == m * 8);
    // slow: the first bit of the last 8 bytes
    uint64_t lim = 0;
    for (size_t b = 0; b + kSessLag < m; ++b) lim = (b + 1) * 8;
    CHECK(sess_limit_bits(m, 0) == lim);
    // a token of at most 48 bits that starts below the limit lies inside the bytes
    if (lim) CHECK(lim - 1 + 48 <= m * 8);
    for (uint32_t bit = 0; bit < 8; ++bit) {
      CHECK(sess_has_work(m, bit, 1));
      CHECK(sess_has_work(m, bit, 0) == (lim > bit));
    }
  }
  CHECK(kSessHeaderMax * 8 > 17 + 19 * 3 + 320 * (7 + 7));  // the longest dynamic header, in bits
}

static void check_pack() {
  for (int trial = 0; trial < 200; ++trial) {
    const size_t k = rnd() % 20 + 1;
    std::vector<size_t> m(k);
    for (auto &v : m) v = rnd() % 3 ? rnd() % 5000 : rnd() % 3;
    const PackLayout L = pack_layout(m.data(), iota_ids(k), 256, 1);
    size_t at = 0;
    for (size_t i = 0; i < k; ++i) {
      CHECK(L.off[i] == at && L.off[i] % 256 == 0);
      size_t room = m[i] ? m[i] : 1;
      while (room % 256) ++room;
      at += room;
      // the reader's 16-byte loads of the slot's last bytes stay inside the slot
      CHECK(((m[i] + 15) & ~size_t(15)) <= room);
    }
    CHECK(L.total == at);
  }
}

static void check_slots() {
  for (size_t m : {size_t(0), size_t(1), size_t(9), size_t(1023), size_t(1024), size_t(1025), size_t(4080),
                   size_t(100000), size_t(1) << 20, size_t(5) << 20}) {
    size_t prev = 0;
    for (unsigned r = 0; r < 16; ++r) {
      const size_t c = sess_out_cap(m, r);
      // slow: doubling by hand
      size_t want = m * 8 < 4096 ? 4096 : m * 8;
      for (unsigned q = 0; q < r; ++q)
        if (want < kSessSlotMax) want *= 2;
      if (want > kSessSlotMax) want = kSessSlotMax;
      CHECK(c % 256 == 0 && c >= want + 258 && c < want + 258 + 256);
      CHECK(c >= prev);
      CHECK(c - 256 >= 258);  // the capacity the kernel sees always admits a token
      prev = c;
    }
  }
  // a round's plan and the relaunch plan after it
  for (int trial = 0; trial < 100; ++trial) {
    const size_t k = rnd() % 30 + 1;
    std::vector<size_t> m(k);
    std::vector<unsigned> rl(k);
    std::vector<int32_t> stop(k);
    for (size_t i = 0; i < k; ++i) {
      m[i] = rnd() % 70000;
      rl[i] = rnd() % 4;
      stop[i] = (int32_t)(rnd() % 4);
    }
    const SessOutPlan P = sess_out_plan(m, rl);
    size_t at = 0;
    for (size_t i = 0; i < k; ++i) {
      CHECK(P.off[i] == at && P.off[i] % 256 == 0);
      CHECK(P.cap[i] == sess_out_cap(m[i], rl[i]));
      at += P.cap[i];
    }
    CHECK(P.total == at);
    const std::vector<size_t> again = sess_relaunch(stop);
    std::set<size_t> want;
    for (size_t i = 0; i < k; ++i)
      if (stop[i] == SS_OUT_FULL) want.insert(i);
    CHECK(std::set<size_t>(again.begin(), again.end()) == want && again.size() == want.size());
    CHECK(std::is_sorted(again.begin(), again.end()));
  }
}

static void check_unused() {
  for (uint64_t total = 0; total <= 40; ++total)
    for (uint64_t bits = 0; bits <= total * 8; ++bits) {
      uint64_t touched = 0;  // slow: bytes holding a consumed bit
      for (uint64_t b = 0; b < total; ++b)
        if (b * 8 < bits) touched++;
      CHECK(sess_unused(total, bits) == total - touched);
    }
}

static uint32_t adler_slow(const std::vector<uint8_t> &v, uint32_t adler = 1) {
  uint32_t s1 = adler & 0xFFFF, s2 = adler >> 16;
  for (uint8_t b : v) {
    s1 = (s1 + b) % 65521;
    s2 = (s2 + s1) % 65521;
  }
  return s1 | (s2 << 16);
}

static void check_adler() {
  for (int trial = 0; trial < 300; ++trial) {
    std::vector<uint8_t> a(rnd() % 7000), b(trial % 7 ? rnd() % 7000 : 0);
    const uint8_t fill = trial % 3 == 0 ? 0xFF : 0;
    for (auto &x : a) x = fill ? fill : (uint8_t)rnd();
    for (auto &x : b) x = fill ? fill : (uint8_t)rnd();
    std::vector<uint8_t> ab(a);
    ab.insert(ab.end(), b.begin(), b.end());
    CHECK(adler_combine(adler_slow(a), adler_slow(b), b.size()) == adler_slow(ab));
  }
  CHECK(adler_combine(1, 1, 0) == 1);
  // a long second part: the length only counts modulo 65521
  CHECK(adler_combine(0x12345678 % 0xFFF10000u, 1, 65521) == adler_combine(0x12345678 % 0xFFF10000u, 1, 0));
}

static void check_duplicates() {
  int obj[8];
  for (int trial = 0; trial < 200; ++trial) {
    const size_t k = rnd() % 8;
    std::vector<const void *> v(k);
    for (auto &p : v) p = &obj[rnd() % 8];
    bool dup = false;
    for (size_t i = 0; i < k; ++i)
      for (size_t j = i + 1; j < k; ++j) dup |= v[i] == v[j];
    CHECK(sess_has_duplicates(v.data(), k) == dup);
  }
  CHECK(!sess_has_duplicates(nullptr, 0));
}

int main() {
  static_assert(sizeof(SessRec) % 256 == 0 && offsetof(SessRec, lens) == kSessRing, "record layout");
  static_assert(offsetof(SessRec, op) % 8 == 0 && sizeof(SessJob) == 48 && sizeof(SessResult) == 40, "record layout");
  check_tail();
  check_limit();
  check_pack();
  check_slots();
  check_unused();
  check_adler();
  check_duplicates();
  printf("stream_host_check ok\n");
  return 0;
}
