// tools/dev_batch_host_check.cpp -- drives the planner of the device-resident
// batch calls (zlib.ts_amd/csrc/dev_batch_plan.h) without a device: the copy
// jobs and their tile table, the patch jobs, the stored-block job list, the
// output bound, the groups, the capacity masking and the tile limit, each
// against a slow restatement.  The job tables are run by the host model of
// dev_copy_kernel / dev_patch_kernel in tools/dev_batch_model.h.  Meant to be built
// with a sanitizer and run on its own (tests/test_dev_batch_host.py):
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -pthread -o dev_batch_host_check tools/dev_batch_host_check.cpp
//   ./dev_batch_host_check
//
// Every buffer is a heap allocation of exactly its bytes.  Prints
// "dev_batch_host_check ok"; exit 1 on a broken invariant.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../zlib.ts_amd/csrc/deflate_index_host.h"  // restart_after
#include "dev_batch_model.h"

typedef std::vector<uint8_t> Bytes;

static uint32_t rng_state = 0x9E3779B9u;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

static Bytes filler(size_t n) {
  Bytes b(n);
  for (size_t i = 0; i < n; ++i) b[i] = (uint8_t)(rnd() >> 8);
  return b;
}

// ---- slow restatements ---------------------------------------------------------------
// stored blocks as the host batch call writes them (batch_api.cpp)
static Bytes slow_stored(const Bytes &in) {
  Bytes o;
  if (in.empty()) return Bytes{1, 0, 0, 0xFF, 0xFF};
  for (size_t p = 0; p < in.size(); p += 65535) {
    const uint32_t l = (uint32_t)std::min<size_t>(65535, in.size() - p);
    o.push_back(p + l == in.size() ? 1 : 0);
    o.push_back(l & 0xFF);
    o.push_back(l >> 8);
    o.push_back(~l & 0xFF);
    o.push_back((~l >> 8) & 0xFF);
    o.insert(o.end(), in.begin() + p, in.begin() + p + l);
  }
  return o;
}
static Bytes slow_frame(int fmt, int ctype_opt, const Bytes &body, uint32_t crc, uint32_t adler, uint32_t isize) {
  Bytes o;
  if (fmt == kFmtGzip) o = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 3};
  if (fmt == kFmtZlib) {
    const uint32_t cmf = 0x78, flg0 = (uint32_t)ctype_opt << 6;
    o = {(uint8_t)cmf, (uint8_t)(flg0 | (31 - ((cmf << 8) + flg0) % 31))};
  }
  o.insert(o.end(), body.begin(), body.end());
  if (fmt == kFmtGzip) {
    for (int k = 0; k < 4; ++k) o.push_back((crc >> (8 * k)) & 0xFF);
    for (int k = 0; k < 4; ++k) o.push_back((isize >> (8 * k)) & 0xFF);
  }
  if (fmt == kFmtZlib)
    for (int k = 0; k < 4; ++k) o.push_back((adler >> (24 - 8 * k)) & 0xFF);
  return o;
}
// the pipeline's worst case, block by block, with the markers where
// restart_after puts them in a batch stream at offset 0
static uint64_t slow_bound2(uint64_t n) {
  const uint64_t nb = (n + 32767) / 32768;
  const uint64_t span[2] = {0, n};
  uint64_t b = 0;
  for (uint64_t k = 0; k < nb; ++k) {
    const uint64_t blen = std::min<uint64_t>(32768, n - k * 32768);
    b += blen + 5 * ((blen + 65534) / 65535) + 5;
    // (restart_after reads span[2 b], span[2 b + 1]: one stream at block 0 .. nb - 1)
    const uint64_t nx = (k + 1) * 32768;
    const bool marker = nx < span[1] && ((nx - span[0]) / 32768) % 32 == 0;
    if (marker) b += 10;
  }
  return b;
}

static const size_t kSizes[] = {0,      1,      2,         15,        16,        17,         4095,       32767,
                                32768,  32769,  65534,     65535,     65536,     65537,      100001,     2 * 65535 - 1,
                                131070, 131071, 3 * 65535, 3 * 65535 + 1};

static void check_stored_and_frames() {
  for (const size_t n : kSizes)
    for (int fmt = kFmtRaw; fmt <= kFmtGzip; ++fmt)
      for (int mis = 0; mis < 3; ++mis) {
        const Bytes backing = filler(n + 3);
        // (the input as a view at an odd offset; its own allocation of n bytes for the bounds)
        Bytes in(backing.begin() + mis, backing.begin() + mis + n);
        const Bytes body = slow_stored(in);
        CHECK(body.size() == stored_len(n));
        const uint32_t sums[4] = {0xAABBCCDDu, 0x11223344u, 0xDEADBEEFu, 0x01020304u};
        const Bytes want = slow_frame(fmt, 0, body, sums[2], sums[3], (uint32_t)n);
        CHECK(want.size() == dev_batch_bound(n, 0, (MemberKind)fmt));
        Bytes out(want.size() + mis, 0x5A);  // exactly the room: ASan guards the rest
        const MemberFrame fr = frame_of((MemberKind)fmt, 0);
        const uint32_t plen = fr.prefix_len(), tl = fr.trailer_len();
        CHECK(plen == (fmt == kFmtGzip ? 10u : fmt == kFmtZlib ? 2u : 0u) && plen + body.size() + tl == want.size());
        DevCopyPlan cp;
        std::vector<DevPatchJob> pj;
        const uint64_t dst = addr(out.data()) + mis;
        dev_patch_bytes(pj, dst, fr.prefix.data(), plen);
        CHECK(dev_stored_jobs(addr(in.data()), n, dst + plen, cp, pj));
        dev_patch_trailer(pj, fr.kind, dst + plen + body.size(), n, 1);
        model_copy(cp);
        model_patch(pj, sums);
        CHECK(memcmp(out.data() + mis, want.data(), want.size()) == 0);
        for (int k = 0; k < mis; ++k) CHECK(out[k] == 0x5A);
      }
  // zlib's header for every compression type is a multiple of 31
  for (int ct = 0; ct <= 2; ++ct) {
    const std::vector<uint8_t> p = frame_of(kFmtZlib, ct).prefix;
    CHECK(p.size() == 2 && p[0] == 0x78 && ((p[0] << 8) + p[1]) % 31 == 0 && (p[1] >> 6) == ct);
  }
}

// gather: items at every source alignment into the packed layouts, against memcpy + memset
static void check_gather(size_t align, bool zero_pad) {
  std::vector<size_t> n;
  for (const size_t s : kSizes)
    for (int rep = 0; rep < 2; ++rep) n.push_back(s);
  const size_t count = n.size();
  std::vector<Bytes> store(count);
  std::vector<uint64_t> src(count);
  for (size_t i = 0; i < count; ++i) {
    // (an allocation of exactly n bytes at whatever alignment malloc gives,
    // moved through 0..15 by a prefix that is part of another item's bytes)
    store[i] = filler(n[i] + (i % 16));
    src[i] = addr(store[i].data()) + (i % 16);
  }
  std::vector<size_t> ids;
  for (size_t i = 0; i < count; ++i)
    if (!zero_pad || n[i]) ids.push_back(i);  // (deflate packs no empty item)
  const PackLayout L = pack_layout(n.data(), ids, align, 1);
  void *raw = aligned_alloc(256, L.total + 256);
  uint8_t *packed = static_cast<uint8_t *>(raw);
  memset(packed, 0xC3, L.total + 256);
  // the items' own allocations hold (i % 16) bytes in front: loads there are
  // outside the item and the model refuses to use their values
  DevCopyPlan cp;
  CHECK(dev_gather_plan(src.data(), n.data(), ids, L, addr(packed), zero_pad, cp) == ZT_OK);
  model_copy(cp);
  Bytes want(L.total + 256, 0xC3);
  for (size_t k = 0; k < ids.size(); ++k) {
    const size_t i = ids[k];
    if (n[i]) memcpy(want.data() + L.off[k], reinterpret_cast<const void *>(src[i]), n[i]);
    if (zero_pad) memset(want.data() + L.off[k] + n[i], 0, (k + 1 < ids.size() ? L.off[k + 1] : L.total) - L.off[k] - n[i]);
  }
  CHECK(memcmp(packed, want.data(), L.total + 256) == 0);
  // every tile belongs to the job the search gives
  for (uint64_t t = 0; t < cp.tiles; ++t) {
    const DevCopyJob &j = cp.jobs[dev_copy_find(cp.jobs, (uint32_t)t)];
    CHECK(j.tile0 <= t && (t - j.tile0) * kDevTile < j.len);
  }
  free(raw);
}

// scatter: from an aligned buffer to destinations at every alignment, each
// an allocation of exactly its bytes
static void check_scatter() {
  for (const size_t n : kSizes)
    for (int a = 0; a < 16; ++a)
      for (int sa = 0; sa < 16; sa += 5) {
        if (!n) continue;
        const Bytes in = filler(n + sa);
        // (the destination ends where ASan's redzone of `exact` starts)
        Bytes exact(n + a, 0x77);
        DevCopyPlan cp;
        CHECK(cp.add(addr(in.data()) + sa, addr(exact.data()) + a, n));
        model_copy(cp);
        CHECK(memcmp(exact.data() + a, in.data() + sa, n) == 0);
        for (int k = 0; k < a; ++k) CHECK(exact[k] == 0x77);
      }
}

static void check_bound() {
  for (uint64_t n = 0; n < (40u << 20); n = n < 70000 ? n + 1 : n + 999983) {
    const uint64_t b2 = dev_batch_bound(n, 2, kFmtRaw), b1 = dev_batch_bound(n, 1, kFmtRaw);
    if (n == 0) {
      CHECK(b2 == 5 && b1 == 5 && dev_batch_bound(0, 0, kFmtGzip) == 23 && dev_batch_bound(0, 0, kFmtZlib) == 11);
      continue;
    }
    CHECK(b2 == slow_bound2(n));
    // fixed codes: 9 bits a byte, 7 + 3 + 3 bits, padding, 4 sync bytes, per block
    const uint64_t nb = (n + 32767) / 32768;
    uint64_t f = 10 * ((nb - 1) / 32);
    for (uint64_t k = 0; k < nb; ++k) {
      const uint64_t blen = std::min<uint64_t>(32768, n - k * 32768);
      f += (9 * blen + 7 + 3 + 3 + 7) / 8 + 4;
    }
    CHECK(b1 >= f && b1 >= b2);
    CHECK(dev_batch_bound(n, 0, kFmtRaw) == n + 5 * ((n + 65534) / 65535));
    CHECK(dev_batch_bound(n, 2, kFmtGzip) == b2 + 18 && dev_batch_bound(n, 2, kFmtZlib) == b2 + 6);
  }
  // inside the room the pipeline's output buffer has (batch_out_bound of the padded item)
  for (const size_t n : kSizes)
    if (n) CHECK(dev_batch_bound(n, 1, kFmtRaw) <= batch_out_bound(align_up(n, 32768)) + n / 8 + 64);
}

static void check_groups() {
  std::vector<size_t> n;
  for (int i = 0; i < 3000; ++i) n.push_back(rnd() % 3 == 0 ? 0 : rnd() % 200000);
  n[17] = 5u << 20;  // larger than the budget: a group of its own
  const std::vector<size_t> ids = iota_ids(n.size());
  for (const size_t align : {(size_t)256, (size_t)32768}) {
    const uint64_t budget = 1u << 20;
    const std::vector<size_t> cut = dev_group_cuts(n.data(), ids, align, budget);
    CHECK(cut.front() == 0 && cut.back() == n.size());
    for (size_t g = 0; g + 1 < cut.size(); ++g) {
      CHECK(cut[g] < cut[g + 1]);
      uint64_t cost = 0;
      for (size_t k = cut[g]; k < cut[g + 1]; ++k) cost += align_up(std::max<size_t>(n[k], 1), align);
      CHECK(cost <= budget || cut[g + 1] - cut[g] == 1);
      // greedy: the next item would not have fitted
      if (g + 2 < cut.size()) CHECK(cost + align_up(std::max<size_t>(n[cut[g + 1]], 1), align) > budget);
    }
  }
  const std::vector<size_t> none;
  const std::vector<size_t> cut0 = dev_group_cuts(n.data(), none, 256, 1);
  CHECK(cut0.size() == 2 && cut0[0] == 0 && cut0[1] == 0);
}

// the launcher's limit: a plan never holds more than 0x7FFFFFFF tiles, the
// job that would pass it is refused and the gather plan answers ZT_E_ARG
static void check_tile_limit() {
  DevCopyPlan cp;
  const uint64_t big = 1ull << 40;  // 2^25 tiles
  size_t added = 0;
  while (cp.add(0x1000, 0x2000, big)) ++added;
  CHECK(added == 63 && cp.tiles == 63ull << 25 && cp.tiles <= kDevMaxTiles);
  CHECK(cp.add(0x1000, 0x2000, (kDevMaxTiles - cp.tiles) * kDevTile));  // exactly to the limit
  CHECK(cp.tiles == kDevMaxTiles);
  CHECK(!cp.add(0x1000, 0x2000, 1) && cp.tiles == kDevMaxTiles && cp.jobs.size() == 64);
  CHECK(cp.add(0x1000, 0x2000, 0) && cp.jobs.size() == 64);  // (an empty job takes no tile)
  // a count of one-tile items near the limit, sizes only (nothing is copied)
  std::vector<size_t> n(70, (size_t)big);
  std::vector<uint64_t> src(70, 0x1000);
  const std::vector<size_t> ids = iota_ids(70);
  const PackLayout L = pack_layout(n.data(), ids, 256, 1);
  DevCopyPlan g;
  CHECK(dev_gather_plan(src.data(), n.data(), ids, L, 0x100000, false, g) == ZT_E_ARG);
  DevCopyPlan g2;
  const std::vector<size_t> ids63(ids.begin(), ids.begin() + 63);
  CHECK(dev_gather_plan(src.data(), n.data(), ids63, pack_layout(n.data(), ids63, 256, 1), 0x100000, false, g2) ==
        ZT_OK);
  std::vector<DevPatchJob> pj;
  DevCopyPlan full;
  CHECK(full.add(0x1000, 0x2000, kDevMaxTiles * (uint64_t)kDevTile));
  CHECK(!dev_stored_jobs(0x1000, 10, 0x2000, full, pj));
}

static void check_capacity() {
  const size_t cap[3] = {0, 10, 11};
  CHECK(dev_fits(0, cap, 0) && !dev_fits(1, cap, 0));
  CHECK(dev_fits(10, cap, 1) && !dev_fits(11, cap, 1) && dev_fits(11, cap, 2));
  CHECK(!dev_fits(1ull << 40, cap, 2));
}

int main() {
  check_stored_and_frames();
  check_gather(32768, true);
  check_gather(256, false);
  check_scatter();
  check_bound();
  check_groups();
  check_tile_limit();
  check_capacity();
  if (fails) {
    fprintf(stderr, "dev_batch_host_check: %d failures\n", fails);
    return 1;
  }
  printf("dev_batch_host_check ok\n");
  return 0;
}
