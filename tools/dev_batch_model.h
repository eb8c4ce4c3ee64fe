// tools/dev_batch_model.h -- what the stand-alone host checks share: the CHECK
// counter and a host model of dev_copy_kernel (dev_batch.hip) and
// dev_patch_kernel (member_frame.hip) that runs the job tables of
// zlib.ts_amd/csrc/dev_batch_plan.h and follows the kernels' index arithmetic
// access by access: every 16-byte load must be aligned and hold at least one
// byte of the job's source, bytes of such a word outside the source read as
// garbage (so a result that depended on them would differ), and every store
// must lie inside the job's destination.  Used by dev_batch_host_check.cpp and
// member_frame_host_check.cpp.
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>

#include "../zlib.ts_amd/csrc/dev_batch_plan.h"

using namespace zt;

static int fails = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      if (fails < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

static uint64_t addr(const uint8_t *p) { return reinterpret_cast<uint64_t>(p); }

// ---- the kernels' host model ------------------------------------------------------
static uint8_t load_byte(const DevCopyJob &j, uint64_t addr) {
  CHECK(addr >= j.src && addr < j.src + j.len);
  return *reinterpret_cast<const uint8_t *>(addr);
}
static void store_byte(const DevCopyJob &j, uint64_t addr, uint8_t v) {
  CHECK(addr >= j.dst && addr < j.dst + j.len + j.zero);
  if (addr >= j.dst && addr < j.dst + j.len + j.zero) *reinterpret_cast<uint8_t *>(addr) = v;
}
// an aligned 16-byte load: must hold a byte of the source; the bytes outside
// the source are garbage
static void load16(const DevCopyJob &j, uint64_t addr, uint8_t w[16]) {
  CHECK((addr & 15) == 0);
  CHECK(addr + 16 > j.src && addr < j.src + j.len);
  for (int k = 0; k < 16; ++k) {
    const uint64_t a = addr + k;
    w[k] = (a >= j.src && a < j.src + j.len) ? *reinterpret_cast<const uint8_t *>(a) : (uint8_t)(0xE0 | k);
  }
}
// one workgroup of dev_copy_kernel (all its threads, in turn)
static void model_tile(const std::vector<DevCopyJob> &jobs, uint32_t tile) {
  const DevCopyJob j = jobs[dev_copy_find(jobs, tile)];
  const uint64_t o0 = (uint64_t)(tile - j.tile0) * kDevTile;
  if (o0 >= j.len) return;
  const bool last_tile = j.len - o0 <= kDevTile;
  uint32_t n = (uint32_t)(last_tile ? j.len - o0 : kDevTile);
  uint64_t s = j.src + o0, d = j.dst + o0;
  if (last_tile)
    for (uint32_t i = 0; i < j.zero; ++i) store_byte(j, d + n + i, 0);
  const uint32_t to16 = (uint32_t)((16 - (d & 15)) & 15);
  const uint32_t lead = to16 < n ? to16 : n;
  for (uint32_t i = 0; i < lead; ++i) store_byte(j, d + i, load_byte(j, s + i));
  s += lead;
  d += lead;
  n -= lead;
  const uint32_t body = n & ~15u;
  const uint32_t sh = (uint32_t)(s & 15);
  for (uint32_t i = 0; i < body; i += 16) {
    uint8_t w[32];
    load16(j, s - sh + i, w);
    if (sh)
      load16(j, s - sh + i + 16, w + 16);
    else
      memcpy(w + 16, w, 16);
    CHECK(((d + i) & 15) == 0);  // a 16-byte store
    for (uint32_t k = 0; k < 16; ++k) store_byte(j, d + i + k, w[sh + k]);
  }
  for (uint32_t i = body; i < n; ++i) store_byte(j, d + i, load_byte(j, s + i));
}
static void model_copy(const DevCopyPlan &cp) {
  uint64_t tiles = 0;
  for (const DevCopyJob &j : cp.jobs) {
    CHECK(j.len > 0 && j.tile0 == tiles);
    tiles += (j.len + kDevTile - 1) / kDevTile;
  }
  CHECK(tiles == cp.tiles);
  for (uint64_t t = 0; t < cp.tiles; ++t) model_tile(cp.jobs, (uint32_t)t);
}
static void model_patch(const std::vector<DevPatchJob> &pj, const uint32_t *sums) {
  for (const DevPatchJob &j : pj) {
    uint8_t *d = reinterpret_cast<uint8_t *>(j.dst);
    if (j.kind != kPatchBytes) {
      CHECK((j.kind == kFmtGzip || j.kind == kFmtZlib) && j.len == member_trailer_len((MemberKind)j.kind));
      put_trailer(d, (MemberKind)j.kind, sums[2 * j.sum], sums[2 * j.sum + 1], (uint32_t)j.value);
    } else {
      CHECK(j.len <= 8);
      for (uint32_t k = 0; k < j.len && k < 8; ++k) d[k] = (uint8_t)(j.value >> (8 * k));
    }
  }
}
