// range_call.hip -- the gather every range call ends with (range_call.h: the
// index and the checkpoint formats; bgzf_api.hip): the requested sub-ranges of
// the decode buffer into one packed buffer, which then comes back with one
// download.
#include "zt_internal.h"

namespace zt {

namespace {

// (RangeJob, kGatherTile: zt_internal.h)
typedef unsigned int u32x4g __attribute__((ext_vector_type(4)));

// One workgroup per range and tile.  The destination is 16-byte aligned at
// every tile start, so the body goes out as 16-byte stores; each comes from
// the two aligned 16-byte source words around it, shifted by the range's
// source misalignment (uniform in the workgroup).  The last len % 16 bytes of
// a range go byte by byte.  (A job whose destination is not 16-byte aligned --
// the pieces of a BGZF range, packed back to back: bgzf_api.hip -- sends the
// bytes up to the next 16-byte boundary one by one first; `out` itself is
// aligned, so the ranges of the index calls have none.)
__global__ __launch_bounds__(256) void range_gather_kernel(const RangeJob *__restrict__ jobs, uint32_t njobs,
                                                           const uint8_t *__restrict__ dec, uint8_t *__restrict__ out,
                                                           const ChainInfo *__restrict__ info) {
  if (!info->ok) return;
  uint32_t lo = 0, hi = njobs;  // the last job with tile0 <= blockIdx.x
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (jobs[mid].tile0 <= blockIdx.x)
      lo = mid;
    else
      hi = mid;
  }
  const RangeJob j = jobs[lo];
  const uint64_t o0 = (uint64_t)(blockIdx.x - j.tile0) * kGatherTile;
  if (o0 >= j.len) return;
  uint32_t n = (uint32_t)(j.len - o0 < kGatherTile ? j.len - o0 : kGatherTile);
  const uint8_t *s = dec + j.src + o0;
  uint8_t *d = out + j.dst + o0;
  const uint32_t to16 = (uint32_t)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15);
  const uint32_t lead = to16 < n ? to16 : n;
  for (uint32_t i = threadIdx.x; i < lead; i += 256) d[i] = s[i];
  s += lead;
  d += lead;
  n -= lead;
  const uint32_t body = n & ~15u;
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 15);
  const u32x4g *sa = reinterpret_cast<const u32x4g *>(s - sh);
  const uint32_t q = sh >> 2, r = sh & 3;
  for (uint32_t i = threadIdx.x * 16; i < body; i += 256 * 16) {
    // (sh != 0: the second word starts before s + i + 16 <= s + n, inside the span)
    const u32x4g a = sa[i / 16];
    const u32x4g b = sh ? sa[i / 16 + 1] : a;
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t v[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = q == 0 ? w[k] : q == 1 ? w[k + 1] : q == 2 ? w[k + 2] : w[k + 3];
    u32x4g o;
    o.x = __builtin_amdgcn_alignbyte(v[1], v[0], r);
    o.y = __builtin_amdgcn_alignbyte(v[2], v[1], r);
    o.z = __builtin_amdgcn_alignbyte(v[3], v[2], r);
    o.w = __builtin_amdgcn_alignbyte(v[4], v[3], r);
    *reinterpret_cast<u32x4g *>(d + i) = o;
  }
  for (uint32_t i = body + threadIdx.x; i < n; i += 256) d[i] = s[i];
}

}  // namespace

int range_gather_dev(const RangeJob *d_jobs, uint32_t njobs, uint32_t tiles, const uint8_t *d_dec, uint8_t *d_out,
                     const ChainInfo *d_info, hipStream_t s) {
  if (tiles == 0) return ZT_OK;
  range_gather_kernel<<<tiles, 256, 0, s>>>(d_jobs, njobs, d_dec, d_out, d_info);
  ZT_HIP(hipGetLastError());
  return ZT_OK;
}

}  // namespace zt
