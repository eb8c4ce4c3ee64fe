// Host model of the match kernel's chain heads in their two formats
// (csrc/deflate.hip: chain_link<0>, head_sweep, head_convert): the same link
// arithmetic, sweep and conversions in plain C++, over seeded bucket
// sequences.  Three runs per sequence -- u16 heads with sweeps throughout,
// u32 heads throughout, and format changes at arbitrary sub-chunk starts in
// both directions -- must give the link array of the plain definition (the
// distance to the newest earlier position of the bucket, 0 past DF_MAXDIST).
// The sequences include buckets hit again only after more than 2^16
// positions and sub-chunks linked up to DF_HEAD positions ahead of the next
// sub-chunk's start.  No GPU:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -o head_format_model head_format_model.cpp && ./head_format_model
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

// (as in deflate.hip)
constexpr uint32_t DF_SUB = 4096, DF_RING = 32768, DF_HIST = DF_RING - DF_SUB, DF_HEAD = 320;
constexpr uint32_t DF_MAXDIST = DF_HIST - 64 - (DF_HEAD - 64);  // 28352
constexpr uint32_t DF_HSIZE = 12240, HEAD_SWEEP = 4;
constexpr uint32_t kNoHead = 0x80000000u;
static_assert(DF_MAXDIST + (HEAD_SWEEP + 1) * DF_SUB + DF_HEAD < 65536 - 1024, "ages stay below 2^16");

struct Heads {
  bool fmt16;
  std::vector<uint32_t> h16;  // two buckets per word
  std::vector<uint32_t> h32;
};

static uint32_t link_of(uint32_t p, uint32_t old) {
  const uint32_t d = p - old;
  return d <= DF_MAXDIST ? d : 0u;
}

// chain_link<0, true>: the masked-OR exchange of one half-word
static uint32_t link16(Heads &H, uint32_t h, uint32_t p) {
  uint32_t &w = H.h16[h >> 1];
  const uint32_t sh = (h & 1) * 16;
  const uint32_t old = w;
  w = (w & ~(0xFFFFu << sh)) | ((p & 0xFFFFu) << sh);
  return link_of(p, p - ((p - (old >> sh)) & 0xFFFFu));
}
// chain_link<0, false>: the plain exchange
static uint32_t link32(Heads &H, uint32_t h, uint32_t p) {
  const uint32_t old = H.h32[h];
  H.h32[h] = p;
  return link_of(p, old);
}

static void head_sweep(Heads &H, uint32_t S) {
  const uint32_t stale = (S - 32768u) & 0xFFFFu;
  for (uint32_t i = 0; i < DF_HSIZE / 2; ++i) {
    const uint32_t w = H.h16[i];
    uint32_t r = w;
    for (int k = 0; k < 2; ++k) {
      const uint32_t age = (S - (w >> (16 * k))) & 0xFFFFu;
      if (age > DF_MAXDIST && age < 65536u - 1024u) r = (r & ~(0xFFFFu << (16 * k))) | (stale << (16 * k));
    }
    H.h16[i] = r;
  }
}

static uint32_t head_to32(uint32_t v, uint32_t S) {
  const uint32_t age = (S - v) & 0xFFFFu;
  return age <= DF_MAXDIST ? S - age : age >= 65536u - 1024u ? S + (65536u - age) : kNoHead;
}
static uint32_t head_to16(uint32_t r, uint32_t S) {
  return (S - r <= DF_MAXDIST || r - S <= 1024u) ? (r & 0xFFFFu) : ((S - 32768u) & 0xFFFFu);
}
static void head_convert(Heads &H, bool to16, uint32_t S) {
  if (to16) {
    for (uint32_t i = 0; i < DF_HSIZE / 2; ++i)
      H.h16[i] = head_to16(H.h32[2 * i], S) | head_to16(H.h32[2 * i + 1], S) << 16;
  } else {
    for (uint32_t i = 0; i < DF_HSIZE / 2; ++i) {
      const uint32_t w = H.h16[i];
      H.h32[2 * i] = head_to32(w & 0xFFFFu, S);
      H.h32[2 * i + 1] = head_to32(w >> 16, S);
    }
  }
  H.fmt16 = to16;
}

// mode 0: u16 throughout, 1: u32 throughout, 2: the format of sub-chunk k is
// want16[k] (decided at its start, as match_body does at a block's second
// sub-chunk).  ahead[k]: positions past sub-chunk k's end that are linked with it.
static std::vector<uint16_t> run(const std::vector<uint32_t> &bucket, int mode, const std::vector<uint8_t> &want16,
                                 const std::vector<uint32_t> &ahead, uint64_t conv[2]) {
  const uint32_t n = (uint32_t)bucket.size();
  Heads H;
  H.fmt16 = mode == 0;
  H.h16.assign(DF_HSIZE / 2, 0x80008000u);
  H.h32.assign(DF_HSIZE, kNoHead);
  std::vector<uint16_t> link(n, 0);
  uint32_t inserted = 0;
  for (uint32_t p0 = 0, k = 0; p0 < n; p0 += DF_SUB, ++k) {
    const uint32_t p1 = p0 + DF_SUB < n ? p0 + DF_SUB : n;
    uint32_t ih = p1 + ahead[k] < n ? p1 + ahead[k] : n;
    const bool lnk = ih > inserted;
    bool converted = false;
    if (mode == 2 && (want16[k] != 0) != H.fmt16) {
      head_convert(H, want16[k] != 0, p0);
      conv[want16[k] ? 0 : 1] += 1;
      converted = true;
    }
    if (H.fmt16 && !converted && k % HEAD_SWEEP == 0 && lnk) head_sweep(H, p0);
    if (lnk) {
      for (uint32_t p = inserted; p < ih; ++p)
        link[p] = (uint16_t)(H.fmt16 ? link16(H, bucket[p], p) : link32(H, bucket[p], p));
      inserted = ih;
    }
  }
  return link;
}

static std::vector<uint16_t> plain(const std::vector<uint32_t> &bucket) {
  std::vector<int64_t> last(DF_HSIZE, -1);
  std::vector<uint16_t> link(bucket.size(), 0);
  for (uint32_t p = 0; p < bucket.size(); ++p) {
    const int64_t q = last[bucket[p]];
    if (q >= 0 && p - q <= (int64_t)DF_MAXDIST) link[p] = (uint16_t)(p - q);
    last[bucket[p]] = p;
  }
  return link;
}

static int check(const char *what, const std::vector<uint16_t> &a, const std::vector<uint16_t> &b) {
  for (size_t i = 0; i < a.size(); ++i) {
    if (a[i] != b[i]) {
      printf("FAIL %s: position %zu link %u, expected %u\n", what, i, a[i], b[i]);
      return 1;
    }
  }
  return 0;
}

int main() {
  int bad = 0;
  uint64_t conv[2] = {0, 0}, far_hits = 0, links = 0, ahead_subs = 0;
  for (uint32_t seed = 1; seed <= 24; ++seed) {
    std::mt19937 rng(seed);
    // up to 24 blocks of 32 KiB after 28 KiB of history: positions pass 2^16 several times
    const uint32_t n = DF_HIST + (4 + rng() % 21) * 32768u - (seed % 3 ? rng() % DF_SUB : 0);
    // buckets: a few hot ones (short links), a band hit about every 2^13..2^15
    // positions (links near DF_MAXDIST, on both sides of it), and rare ones
    // that come back only after more than 2^16 positions
    const uint32_t hot = 1 + rng() % 64, band = 8 + rng() % 24, rare = 2 + rng() % 6;
    std::vector<uint32_t> bucket(n);
    std::vector<int64_t> last(DF_HSIZE, -1);
    for (uint32_t p = 0; p < n; ++p) {
      const uint32_t r = rng() % 100000;
      uint32_t h;
      if (r < rare)
        h = DF_HSIZE - 1 - rng() % rare;  // each about once per 10^5 positions
      else if (r < 400)
        h = 2000 + rng() % band;
      else if (r < 60000)
        h = rng() % hot;
      else
        h = 3000 + rng() % 9000;
      bucket[p] = h;
      if (last[h] >= 0 && p - last[h] > 65536) far_hits += 1;
      last[h] = p;
    }
    const uint32_t nsub = (n + DF_SUB - 1) / DF_SUB;
    std::vector<uint32_t> none(nsub, 0), ahead(nsub, 0);
    for (uint32_t k = 0; k < nsub; ++k) {
      if (rng() % 3 == 0) ahead[k] = 1 + rng() % DF_HEAD;
      ahead_subs += ahead[k] != 0;
    }
    const std::vector<uint16_t> ref = plain(bucket);
    for (uint16_t l : ref) links += l != 0;
    for (int a = 0; a < 2; ++a) {
      const std::vector<uint32_t> &ah = a ? ahead : none;
      uint64_t c0[2] = {0, 0};
      bad += check("u16 throughout", run(bucket, 0, {}, ah, c0), ref);
      bad += check("u32 throughout", run(bucket, 1, {}, ah, c0), ref);
      // format schedules: flips at random sub-chunks (often, seldom), and the
      // kernel's own pattern (a verdict per block at its second sub-chunk)
      for (int sched = 0; sched < 4; ++sched) {
        std::vector<uint8_t> want(nsub, 0);
        uint8_t cur = 0;
        for (uint32_t k = 0; k < nsub; ++k) {
          if (sched == 0 && rng() % 2 == 0) cur ^= 1;
          if (sched == 1 && rng() % 9 == 0) cur ^= 1;
          if (sched == 2 && k >= 7 && (k - 7) % 8 == 1) cur = rng() % 2;
          if (sched == 3 && k >= 7 && (k - 7) % 8 == 1) cur ^= 1;
          want[k] = cur;
        }
        bad += check("format changes", run(bucket, 2, want, ah, conv), ref);
      }
    }
  }
  printf("links %llu, bucket hits more than 2^16 positions apart %llu, sub-chunks linked ahead %llu\n",
         (unsigned long long)links, (unsigned long long)far_hits, (unsigned long long)ahead_subs);
  printf("conversions u32 -> u16 %llu, u16 -> u32 %llu\n", (unsigned long long)conv[0], (unsigned long long)conv[1]);
  if (far_hits == 0 || ahead_subs == 0 || conv[0] == 0 || conv[1] == 0) {
    printf("FAIL: the sequences miss a case\n");
    bad += 1;
  }
  printf(bad ? "FAILED\n" : "ok: u16, u32 and changing formats give the plain definition's links\n");
  return bad ? 1 : 0;
}
