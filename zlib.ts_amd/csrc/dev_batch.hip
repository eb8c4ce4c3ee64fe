// dev_batch.hip -- the two ends of the device-resident batch calls
// (include/zt_dev_batch.h; the job tables: dev_batch_plan.h): dev_copy_kernel
// gathers the caller's buffers into the layout the batch pipelines read and
// scatters their results to the caller's pointers.  The few bytes around them
// (prefixes, trailers with the checksums, stored-block headers) are
// dev_patch_kernel's, in member_frame.hip.
#include "zt_internal.h"

namespace zt {

namespace {

typedef unsigned int u32x4d __attribute__((ext_vector_type(4)));

// One workgroup per (job, tile), the job found by binary search over tile0
// (range_gather_kernel's shape, with absolute addresses at both ends).
//
// Loads: byte loads of the job's own bytes, or aligned 16-byte words that hold
// at least one byte of [src, src + len) -- such a word lies in the page and
// in the allocation of that byte.  Stores: only into [dst, dst + len + zero).
// The bytes up to the destination's next 16-byte boundary and the last
// (len - lead) % 16 bytes of a tile go one by one; the body goes out as
// 16-byte stores, each from the two aligned 16-byte source words around it,
// shifted by the source's misalignment against the destination (uniform in
// the workgroup).  Tiles are kDevTile apart, so every tile of a job has the
// same lead.  No LDS, no waiting on another workgroup.
__global__ __launch_bounds__(256) void dev_copy_kernel(const DevCopyJob *__restrict__ jobs, uint32_t njobs) {
  uint32_t lo = 0, hi = njobs;  // the last job with tile0 <= blockIdx.x
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (jobs[mid].tile0 <= blockIdx.x)
      lo = mid;
    else
      hi = mid;
  }
  const DevCopyJob j = jobs[lo];
  const uint64_t o0 = (uint64_t)(blockIdx.x - j.tile0) * kDevTile;
  if (o0 >= j.len) return;
  const bool last_tile = j.len - o0 <= kDevTile;
  uint32_t n = (uint32_t)(last_tile ? j.len - o0 : kDevTile);
  const uint8_t *s = reinterpret_cast<const uint8_t *>(j.src) + o0;
  uint8_t *d = reinterpret_cast<uint8_t *>(j.dst) + o0;
  if (last_tile)  // the zeroed rest of the item's cell (gather for deflate)
    for (uint32_t i = threadIdx.x; i < j.zero; i += 256) d[n + i] = 0;
  const uint32_t to16 = (uint32_t)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15);
  const uint32_t lead = to16 < n ? to16 : n;
  for (uint32_t i = threadIdx.x; i < lead; i += 256) d[i] = s[i];
  s += lead;
  d += lead;
  n -= lead;
  const uint32_t body = n & ~15u;
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 15);
  const u32x4d *sa = reinterpret_cast<const u32x4d *>(s - sh);
  const uint32_t q = sh >> 2, r = sh & 3;
  for (uint32_t i = threadIdx.x * 16; i < body; i += 256 * 16) {
    // first word: holds s[i].  second (sh != 0 only): starts at s + i + 16 - sh
    // < s + i + 16 <= s + n, so it holds s[i + 16 - sh], a byte of the job
    const u32x4d a = sa[i / 16];
    const u32x4d b = sh ? sa[i / 16 + 1] : a;
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t v[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = q == 0 ? w[k] : q == 1 ? w[k + 1] : q == 2 ? w[k + 2] : w[k + 3];
    u32x4d o;
    o.x = __builtin_amdgcn_alignbyte(v[1], v[0], r);
    o.y = __builtin_amdgcn_alignbyte(v[2], v[1], r);
    o.z = __builtin_amdgcn_alignbyte(v[3], v[2], r);
    o.w = __builtin_amdgcn_alignbyte(v[4], v[3], r);
    *reinterpret_cast<u32x4d *>(d + i) = o;
  }
  for (uint32_t i = body + threadIdx.x; i < n; i += 256) d[i] = s[i];
}

}  // namespace

int dev_copy_dev(const DevCopyJob *d_jobs, uint32_t njobs, uint64_t tiles, hipStream_t s) {
  if (tiles == 0 || njobs == 0) return ZT_OK;
  if (tiles > kDevMaxTiles) return set_error(ZT_E_ARG, "batch too large for one launch");
  dev_copy_kernel<<<(uint32_t)tiles, 256, 0, s>>>(d_jobs, njobs);
  ZT_HIP(hipGetLastError());
  return ZT_OK;
}

}  // namespace zt
