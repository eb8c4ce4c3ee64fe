// Host model of the match kernel's serial link (csrc/deflate.hip: hash_keys'
// parked hashes, chain_link, chain_link_groups, link_range, head_sweep): the
// same loops in plain C++ over a model of the LDS arrays, a step's 64 lanes
// applied in lane order as the LDS applies them.  Every call links a range
// [lo, hi) whole groups first (no bounds selects, slot indices masked for the
// wrap only, hashes read one group ahead, the progress word after the group's
// link stores) and the ragged rest as before; after each call the links of its
// range, and at each published progress value the links below it, must be
// those of the plain definition: the distance to the newest earlier position
// of the bucket, 0 beyond DF_MAXDIST.  Runs T = 0 with u32 heads, T = 0 with
// u16 heads and sweeps, and T = 1, over seeded bucket sequences cut into calls
// at random places: lo and hi at every residue modulo 64 and 512, groups that
// straddle the ring's end, ranges shorter than a step, and the history linked
// in one call from a dictionary floor or from 0.  No GPU:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -o chain_link_model chain_link_model.cpp && ./chain_link_model
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

// (as in deflate.hip)
constexpr uint32_t DF_SUB = 4096, DF_RING = 32768, DF_HIST = DF_RING - DF_SUB, DF_HEAD = 320;
constexpr uint32_t DF_MAXDIST = DF_HIST - 64 - (DF_HEAD - 64);  // 28352
constexpr uint32_t DF_HSIZE = 12240, DF_H4SIZE = 4096, HEAD_SWEEP = 4;
constexpr uint32_t kNoHead = 0x80000000u;
constexpr int CL_U = 8;
constexpr uint32_t G = CL_U * 64;

struct Lds {
  std::vector<uint16_t> prev = std::vector<uint16_t>(DF_RING, 0xFFFF);
  std::vector<uint16_t> link4 = std::vector<uint16_t>(DF_SUB, 0);
  std::vector<uint32_t> head32 = std::vector<uint32_t>(DF_HSIZE, kNoHead);
  std::vector<uint32_t> head = std::vector<uint32_t>(DF_HSIZE / 2, 0x80008000u);
  std::vector<uint32_t> head4 = std::vector<uint32_t>(DF_H4SIZE, kNoHead);
  uint32_t dummy[4] = {0, 0, 0, 0};
  uint32_t linked = 0, linked4 = 0;
};

static uint32_t ridx(uint32_t rel) { return rel & (DF_RING - 1); }

// what the run checks against
struct Truth {
  const std::vector<uint16_t> *ref8, *ref4;
  uint32_t call_lo = 0;  // the running call's lo
  int bad = 0;
};

template <int T>
static uint16_t &slot(Lds &s, uint32_t q) {
  return T == 0 ? s.prev[ridx(q)] : s.link4[q & (DF_SUB - 1)];
}

// the progress word just took the value `done`: the links of the call below
// it are final (checked for the two groups below `done`; all of them when the
// call ends)
template <int T>
static void published(Lds &s, Truth &tr, uint32_t done, bool all = false) {
  const std::vector<uint16_t> &ref = T == 0 ? *tr.ref8 : *tr.ref4;
  const uint32_t from = all || done - tr.call_lo < 2 * G ? tr.call_lo : done - 2 * G;
  for (uint32_t p = from; p < done; ++p) {
    if (slot<T>(s, p) != ref[p]) {
      if (tr.bad < 10) printf("FAIL T=%d: progress %u published, position %u holds %u, link %u\n", T, done, p, slot<T>(s, p), ref[p]);
      tr.bad += 1;
      return;
    }
  }
}

// one exchange instruction: the lanes in lane order
template <int T, bool F16>
static void exchange(Lds &s, const uint32_t (&h)[64], const uint32_t (&q)[64], const bool (&live)[64], uint32_t (&old)[64]) {
  for (int l = 0; l < 64; ++l) {
    if (T == 0 && F16) {
      uint32_t &w = live[l] ? s.head[h[l] >> 1] : s.dummy[T];
      const uint32_t sh = (h[l] & 1) * 16;
      old[l] = w >> sh;  // (the low 16 bits count)
      w = (w & ~(0xFFFFu << sh)) | ((q[l] & 0xFFFFu) << sh);
    } else {
      uint32_t &w = live[l] ? (T == 0 ? s.head32[h[l]] : s.head4[h[l]]) : s.dummy[T];
      old[l] = w;
      w = q[l];
    }
  }
}

// chain_link as it was: every group with bounds selects and dummy targets
template <int T, bool F16>
static void chain_link(Lds &s, Truth &tr, uint32_t lo, uint32_t hi) {
  const uint32_t nsteps = (hi - lo + 63) / 64;
  uint32_t hq[CL_U][64];
  auto hashes = [&](uint32_t sb) {
    for (int j = 0; j < CL_U; ++j)
      for (uint32_t l = 0; l < 64; ++l) {
        const uint32_t p = lo + (sb + j) * 64 + l, pc = p < hi ? p : lo;
        hq[j][l] = slot<T>(s, pc);
      }
  };
  hashes(0);
  for (uint32_t sb = 0; sb < nsteps; sb += CL_U) {
    uint32_t old[CL_U][64], q[CL_U][64];
    bool live[CL_U][64];
    for (int j = 0; j < CL_U; ++j) {
      for (uint32_t l = 0; l < 64; ++l) {
        q[j][l] = lo + (sb + j) * 64 + l;
        live[j][l] = q[j][l] < hi;
      }
      exchange<T, F16>(s, hq[j], q[j], live[j], old[j]);
    }
    hashes(sb + CL_U);
    for (int j = 0; j < CL_U; ++j)
      for (uint32_t l = 0; l < 64; ++l) {
        const uint32_t p = q[j][l];
        const uint32_t o = (T == 0 && F16) ? p - ((p - old[j][l]) & 0xFFFFu) : old[j][l];
        const uint32_t d = p - o;
        const uint16_t v = (uint16_t)(d <= DF_MAXDIST ? d : 0u);
        if (live[j][l])
          slot<T>(s, p) = v;
        else
          s.dummy[2 + T] = v;
      }
    const uint32_t done = lo + (sb + CL_U) * 64;
    (T == 0 ? s.linked : s.linked4) = done < hi ? done : hi;
    published<T>(s, tr, done < hi ? done : hi);
  }
}

// chain_link_groups: ng whole groups from lo on
template <int T, bool F16>
static void chain_link_groups(Lds &s, Truth &tr, uint32_t lo, uint32_t ng) {
  uint32_t p[64], hq[CL_U][64];
  for (uint32_t l = 0; l < 64; ++l) p[l] = lo + l;
  for (int j = 0; j < CL_U; ++j)
    for (uint32_t l = 0; l < 64; ++l) hq[j][l] = slot<T>(s, p[l] + 64 * j);
  for (uint32_t g = 0; g < ng; ++g) {
    uint32_t d[CL_U][64], q[CL_U][64];
    bool live[64];
    for (uint32_t l = 0; l < 64; ++l) live[l] = true;
    for (int j = 0; j < CL_U; ++j) {
      for (uint32_t l = 0; l < 64; ++l) q[j][l] = p[l] + 64 * j;
      exchange<T, F16>(s, hq[j], q[j], live, d[j]);
    }
    for (int j = 0; j < CL_U; ++j)
      for (uint32_t l = 0; l < 64; ++l) hq[j][l] = slot<T>(s, p[l] + G + 64 * j);
    for (int j = 0; j < CL_U; ++j)
      for (uint32_t l = 0; l < 64; ++l)
        d[j][l] = (T == 0 && F16) ? ((q[j][l] - d[j][l]) & 0xFFFFu) : q[j][l] - d[j][l];
    for (int j = 0; j < CL_U; ++j)
      for (uint32_t l = 0; l < 64; ++l) slot<T>(s, q[j][l]) = (uint16_t)(d[j][l] <= DF_MAXDIST ? d[j][l] : 0u);
    (T == 0 ? s.linked : s.linked4) = p[0] + G;
    published<T>(s, tr, p[0] + G);
    for (uint32_t l = 0; l < 64; ++l) p[l] += G;
  }
}

template <int T, bool F16>
static void link_range(Lds &s, Truth &tr, uint32_t lo, uint32_t hi, bool lean) {
  tr.call_lo = lo;
  if (lean) {
    const uint32_t ng = (hi - lo) / G;
    if (ng) chain_link_groups<T, F16>(s, tr, lo, ng);
    lo += ng * G;
    if (lo == hi) return;
  }
  chain_link<T, F16>(s, tr, lo, hi);
}

static void head_sweep(Lds &s, uint32_t S) {
  const uint32_t stale = (S - 32768u) & 0xFFFFu;
  for (uint32_t i = 0; i < DF_HSIZE / 2; ++i) {
    const uint32_t w = s.head[i];
    uint32_t r = w;
    for (int k = 0; k < 2; ++k) {
      const uint32_t age = (S - (w >> (16 * k))) & 0xFFFFu;
      if (age > DF_MAXDIST && age < 65536u - 1024u) r = (r & ~(0xFFFFu << (16 * k))) | (stale << (16 * k));
    }
    s.head[i] = r;
  }
}

static std::vector<uint16_t> plain(const std::vector<uint32_t> &bucket, uint32_t floor, uint32_t nbuckets) {
  std::vector<int64_t> last(nbuckets, -1);
  std::vector<uint16_t> link(bucket.size(), 0);
  for (uint32_t p = floor; p < bucket.size(); ++p) {
    const int64_t q = last[bucket[p]];
    if (q >= 0 && p - q <= (int64_t)DF_MAXDIST) link[p] = (uint16_t)(p - q);
    last[bucket[p]] = p;
  }
  return link;
}

struct Coverage {
  bool lo64[64] = {}, hi64[64] = {}, lo512[512] = {}, hi512[512] = {};
  uint64_t straddle = 0, short_calls = 0, one_run = 0, one_run_floor = 0, calls = 0, lean_groups = 0;
};

// the u16 heads are swept every HEAD_SWEEP sub-chunks, here at the sub-chunk
// starts 2, 6, 10, ...: the ring's end (sub-chunk 8) and position 2^16 (16)
// then lie inside calls; no call crosses a sweep point
constexpr uint32_t SWEEP0 = 2 * DF_SUB, SWEEP_STEP = HEAD_SWEEP * DF_SUB;

// variant 0: T = 0 with u32 heads, 1: T = 0 with u16 heads, 2: T = 1.  Links
// positions [floor, n) in calls cut at `cuts` (ascending, from floor to n).
static int run(int variant, const std::vector<uint32_t> &b8, const std::vector<uint32_t> &b4, uint32_t floor,
               const std::vector<uint32_t> &cuts, bool lean, Coverage &cov) {
  const std::vector<uint16_t> ref8 = plain(b8, floor, DF_HSIZE), ref4 = plain(b4, floor, DF_H4SIZE);
  Lds s;
  Truth tr;
  tr.ref8 = &ref8;
  tr.ref4 = &ref4;
  for (size_t c = 0; c + 1 < cuts.size(); ++c) {
    const uint32_t lo = cuts[c], hi = cuts[c + 1];
    if (variant == 1 && lo >= SWEEP0 && (lo - SWEEP0) % SWEEP_STEP == 0) head_sweep(s, lo);
    // hash_keys: the hashes parked in the slots the links will fill
    for (uint32_t p = lo; p < hi; ++p) {
      if (variant == 2)
        s.link4[p & (DF_SUB - 1)] = (uint16_t)b4[p];
      else
        s.prev[ridx(p)] = (uint16_t)b8[p];
    }
    if (variant == 0)
      link_range<0, false>(s, tr, lo, hi, lean);
    else if (variant == 1)
      link_range<0, true>(s, tr, lo, hi, lean);
    else
      link_range<1, false>(s, tr, lo, hi, lean);
    const uint32_t pub = variant == 2 ? s.linked4 : s.linked;
    if (pub != hi) {
      if (tr.bad < 10) printf("FAIL variant %d: call [%u, %u) ended with progress %u\n", variant, lo, hi, pub);
      tr.bad += 1;
    }
    tr.call_lo = lo;
    if (variant == 2)
      published<1>(s, tr, hi, true);
    else
      published<0>(s, tr, hi, true);
    if (lean) {
      const uint32_t ng = (hi - lo) / G;
      cov.calls += 1;
      cov.lean_groups += ng;
      cov.lo64[lo % 64] = cov.hi64[hi % 64] = cov.lo512[lo % 512] = cov.hi512[hi % 512] = true;
      cov.short_calls += hi - lo < 64;
      // a whole group whose positions lie on both sides of the ring's end
      for (uint32_t g = 0; g < ng; ++g) cov.straddle += ridx(lo + g * G) + G > DF_RING;
    }
    if (tr.bad) break;
  }
  return tr.bad;
}

int main() {
  int bad = 0;
  Coverage cov;
  for (uint32_t seed = 1; seed <= 40 && !bad; ++seed) {
    std::mt19937 rng(seed);
    const uint32_t n = 2 * 32768 + 12000 + rng() % 9000;  // the ring wraps twice, positions pass 2^16
    // buckets: a few hot ones (every lane of a step in one bucket now and then),
    // runs of one bucket, and a wide rest; seed 1: one bucket throughout
    const uint32_t hot = 1 + rng() % 32;
    std::vector<uint32_t> b8(n), b4(n);
    for (uint32_t p = 0; p < n;) {
      const uint32_t r = rng() % 100;
      uint32_t len = 1, h8, h4;
      if (seed == 1) {
        h8 = h4 = 7, len = n;
      } else if (r < 3) {
        h8 = rng() % hot, h4 = rng() % hot, len = 1 + rng() % 300;  // a run: lane order decides
      } else if (r < 50) {
        h8 = rng() % hot, h4 = rng() % hot;
      } else {
        h8 = rng() % DF_HSIZE, h4 = rng() % DF_H4SIZE;
      }
      for (uint32_t k = 0; k < len && p < n; ++k, ++p) b8[p] = h8, b4[p] = h4;
    }
    // the history in one call (a workgroup's priming in one run), from 0 or
    // from a dictionary floor, then sub-chunk sized calls: T = 0, u32 heads
    for (uint32_t floor : {0u, 5u, 1000u + seed, 4097u}) {
      std::vector<uint32_t> cuts = {floor, DF_HIST};
      for (uint32_t c = DF_HIST + DF_SUB; c < n; c += DF_SUB) cuts.push_back(c);
      cuts.push_back(n);
      bad += run(0, b8, b4, floor, cuts, true, cov);
      (floor ? cov.one_run_floor : cov.one_run) += 1;
    }
    // calls cut at random places (at most DF_SUB long: link4 holds one
    // sub-chunk), and always at the sweep points
    for (int rep = 0; rep < 2 && !bad; ++rep) {
      const uint32_t floor = rep ? rng() % 3000 : 0;
      std::vector<uint32_t> cuts = {floor};
      uint32_t next_sweep = SWEEP0;
      while (cuts.back() < n) {
        const uint32_t r = rng() % 10;
        uint32_t len = r < 2 ? 1 + rng() % 63 : r < 4 ? 64 * (1 + rng() % 16) + (rng() % 3) - 1 : r < 7 ? 1 + rng() % 1500 : 1 + rng() % DF_SUB;
        uint32_t c = cuts.back() + len;
        if (c > n) c = n;
        if (c > next_sweep && cuts.back() < next_sweep) c = next_sweep;
        if (c >= next_sweep) next_sweep += SWEEP_STEP;
        cuts.push_back(c);
      }
      for (int variant = 0; variant < 3; ++variant) {
        bad += run(variant, b8, b4, floor, cuts, true, cov);
        Coverage unused;
        if (seed <= 4) bad += run(variant, b8, b4, floor, cuts, false, unused);  // (the model of the former link)
      }
    }
  }
  int missed = 0;
  for (int i = 0; i < 64; ++i) missed += !cov.lo64[i] + !cov.hi64[i];
  for (int i = 0; i < 512; ++i) missed += !cov.lo512[i] + !cov.hi512[i];
  printf("calls %llu, whole groups %llu, groups across the ring's end %llu, calls shorter than a step %llu, "
         "one-run histories %llu + %llu with a floor, residues missed %d\n",
         (unsigned long long)cov.calls, (unsigned long long)cov.lean_groups, (unsigned long long)cov.straddle,
         (unsigned long long)cov.short_calls, (unsigned long long)cov.one_run, (unsigned long long)cov.one_run_floor, missed);
  if (missed || !cov.straddle || !cov.short_calls || !cov.one_run || !cov.one_run_floor) {
    printf("FAIL: the sequences miss a case\n");
    bad += 1;
  }
  printf(bad ? "FAILED\n" : "chain_link_model ok\n");
  return bad ? 1 : 0;
}
