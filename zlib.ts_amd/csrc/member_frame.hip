// member_frame.hip -- the two kernels that write a member's frame on the device
// (the bytes: member_frame.h).  frame_members_kernel lays whole members out in
// one buffer, one FrameItem each (the host batch calls, BGZF);
// dev_patch_kernel writes the few bytes around bodies that dev_copy_kernel
// (dev_batch.hip) scattered to arbitrary pointers (the device-resident batch).
#include "zt_internal.h"

namespace zt {

namespace {

// one workgroup per member: prefix, body, trailer (put_trailer).  patch > 0
// (BGZF, bgzf_api.hip): prefix bytes [patch, patch + 2) are the member's own
// size - 1, little endian, in place of the shared prefix's
__global__ __launch_bounds__(256) void frame_members_kernel(const FrameItem *__restrict__ items,
                                                            const uint8_t *__restrict__ prefix, uint32_t plen,
                                                            MemberKind kind, const uint8_t *__restrict__ body,
                                                            const uint32_t *__restrict__ sums,
                                                            uint8_t *__restrict__ out, uint32_t patch) {
  const FrameItem it = items[blockIdx.x];
  uint8_t *o = out + it.out_off;
  const uint32_t bsize = plen + it.body_len + member_trailer_len(kind) - 1;
  for (uint32_t i = threadIdx.x; i < plen; i += 256)
    o[i] = (patch && i - patch < 2) ? (uint8_t)(bsize >> (8 * (i - patch))) : prefix[i];
  const uint8_t *b = body + it.body_off;
  uint8_t *ob = o + plen;
  // (body and destination offsets are arbitrary: dwords read unaligned by
  // byte aligns from the source's aligned words)
  const uint32_t n = it.body_len;
  const uint32_t lead = (uint32_t)((4 - ((uintptr_t)ob & 3)) & 3) < n ? (uint32_t)((4 - ((uintptr_t)ob & 3)) & 3) : n;
  for (uint32_t i = threadIdx.x; i < lead; i += 256) ob[i] = b[i];
  const uint8_t *bs = b + lead;
  uint32_t *od = reinterpret_cast<uint32_t *>(ob + lead);
  const uint32_t nw = (n - lead) / 4;
  const uint32_t sh = (uint32_t)((uintptr_t)bs & 3);
  const uint32_t *sw = reinterpret_cast<const uint32_t *>(bs - sh);
  for (uint32_t w = threadIdx.x; w < nw; w += 256) {
    const uint32_t lo = sw[w], hi = sh ? sw[w + 1] : 0u;
    od[w] = sh ? __builtin_amdgcn_alignbyte(hi, lo, sh) : lo;
  }
  for (uint32_t i = lead + 4 * nw + threadIdx.x; i < n; i += 256) ob[i] = b[i];
  // (a raw member has no sums to read)
  if (threadIdx.x == 0 && kind != kFmtRaw)
    put_trailer(ob + n, kind, sums[2 * blockIdx.x], sums[2 * blockIdx.x + 1], it.isize);
}

// one thread per patch job (DevPatchJob: dev_batch_plan.h)
__global__ __launch_bounds__(256) void dev_patch_kernel(const DevPatchJob *__restrict__ jobs, uint32_t njobs,
                                                        const uint32_t *__restrict__ sums) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= njobs) return;
  const DevPatchJob j = jobs[t];
  uint8_t *d = reinterpret_cast<uint8_t *>(j.dst);
  if (j.kind != kPatchBytes) {
    put_trailer(d, (MemberKind)j.kind, sums[2 * (size_t)j.sum], sums[2 * (size_t)j.sum + 1], (uint32_t)j.value);
  } else {
    for (uint32_t k = 0; k < j.len && k < 8; ++k) d[k] = (uint8_t)(j.value >> (8 * k));
  }
}

}  // namespace

int frame_members_dev(const FrameItem *d_items, uint32_t count, const uint8_t *d_prefix, uint32_t plen,
                      MemberKind kind, const uint8_t *d_body, const uint32_t *d_sums, uint8_t *d_out, hipStream_t s,
                      uint32_t patch) {
  if (!count) return ZT_OK;
  if (patch && patch + 2 > plen) return set_error(ZT_E_ARG, "size patch outside the prefix");
  frame_members_kernel<<<count, 256, 0, s>>>(d_items, d_prefix, plen, kind, d_body, d_sums, d_out, patch);
  ZT_HIP(hipGetLastError());
  return ZT_OK;
}

int dev_patch_dev(const DevPatchJob *d_jobs, uint32_t njobs, const uint32_t *d_sums, hipStream_t s) {
  if (njobs == 0) return ZT_OK;
  dev_patch_kernel<<<(njobs + 255) / 256, 256, 0, s>>>(d_jobs, njobs, d_sums);
  ZT_HIP(hipGetLastError());
  return ZT_OK;
}

}  // namespace zt
