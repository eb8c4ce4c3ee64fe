// container.hip -- find_members: candidate gzip member starts of a packed batch
// (include/zt_container_batch.h; host side: container_batch_api.cpp).
//
// The reference identifies a member by ID1, ID2 and CM alone
// (src/GUnzip.ts:77-82), so every byte position where 1F 8B 08 starts is a
// candidate and the set holds every true member start.  Candidates inside
// data, comments or FEXTRA are decoded speculatively and dropped by the
// host's chain walk (gunzip_chain.h), as find_syncs' false sync points are
// (inflate_seg.hip).
//
// One pass over the packed input: a workgroup takes a 4 KiB span, a lane one
// 16-byte aligned chunk as one 16-byte load; the two bytes past a chunk come
// from the next lane's chunk (a wave's last lane loads them).  Items start at
// 256-byte aligned offsets of the buffer, so a chunk lies in one item (or in
// padding); a position counts only when all three bytes lie inside its item,
// so nothing matches across two items or in padding, whatever the padding
// holds.  A workgroup gathers its candidates in LDS and takes its place in
// the list with one global atomic.  The list's capacity is proportional to
// the input; past it the kernel keeps counting and stops storing.
#include "zt_internal.h"

namespace zt {

namespace {

constexpr uint32_t kFmThreads = 256;
constexpr uint32_t kFmSpan = kFmThreads * 16;  // bytes per workgroup
// 1F 8B 08 cannot overlap itself: at most one candidate per 3 bytes of the
// span and the 2 after it
constexpr uint32_t kFmLocal = (kFmSpan + 2) / 3 + 2;

__global__ __launch_bounds__(kFmThreads) void find_members(const uint8_t *__restrict__ in, uint64_t total,
                                                           const uint64_t *__restrict__ item_off,
                                                           const uint64_t *__restrict__ item_len, uint32_t count,
                                                           MemberCand *__restrict__ list, uint32_t cap,
                                                           uint32_t *__restrict__ found) {
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  __shared__ uint32_t s_n, s_base, s_first;
  __shared__ MemberCand s_list[kFmLocal];
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t span = (uint64_t)blockIdx.x * kFmSpan;
  if (threadIdx.x == 0) {
    s_n = 0;
    // last item that starts at or before the span (item_off is ascending, item_off[0] = 0)
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (item_off[mid] <= span)
        lo = mid;
      else
        hi = mid;
    }
    s_first = lo;
  }
  __syncthreads();
  const uint64_t base = span + (uint64_t)threadIdx.x * 16;
  const bool live = base < total;  // (total is a multiple of 256: a live chunk is whole)
  u32x4 v = {0u, 0u, 0u, 0u};
  if (live) v = *reinterpret_cast<const u32x4 *>(in + base);
  // the 4 bytes after the chunk: the next lane's first word
  uint32_t nx = (uint32_t)__shfl_down((int)v.x, 1, 64);
  if (lane == 63) nx = base + 16 < total ? *reinterpret_cast<const uint32_t *>(in + base + 16) : 0u;
  if (live) {
    // the chunk's item: walk on from the span's first
    uint32_t it = s_first;
    while (it + 1 < count && item_off[it + 1] <= base) ++it;
    const uint64_t ioff = item_off[it], iend = ioff + item_len[it];
    const uint32_t w[5] = {v.x, v.y, v.z, v.w, nx};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t x = (j & 3) ? __builtin_amdgcn_alignbyte(w[(j >> 2) + 1], w[j >> 2], j & 3) : w[j >> 2];
      if ((x & 0xFFFFFFu) == 0x088B1Fu) {
        const uint64_t p = base + j;
        // (offset 0 is a start of every item whatever it holds: the host adds it)
        if (p > ioff && p + 3 <= iend) {
          const uint32_t k = atomicAdd(&s_n, 1u);
          if (k < kFmLocal) s_list[k] = MemberCand{p - ioff, it, 0u};
        }
      }
    }
  }
  __syncthreads();
  const uint32_t m = s_n < kFmLocal ? s_n : kFmLocal;
  if (threadIdx.x == 0 && m) s_base = atomicAdd(found, m);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < m; i += kFmThreads)
    if ((uint64_t)s_base + i < cap) list[s_base + i] = s_list[i];
}

}  // namespace

// d_in: `total` packed bytes (a multiple of 256, 16-byte aligned), item i at
// d_item_off[i] (ascending, 256-aligned, [0] = 0) with d_item_len[i] bytes.
// *d_found (zeroed here) = the candidates seen; the first min(*d_found, cap)
// are stored in d_list, in any order.
int find_members_dev(const uint8_t *d_in, uint64_t total, const uint64_t *d_item_off, const uint64_t *d_item_len,
                     uint32_t count, MemberCand *d_list, uint32_t cap, uint32_t *d_found, hipStream_t s) {
  ZT_HIP(hipMemsetAsync(d_found, 0, sizeof(uint32_t), s));
  if (!total || !count) return ZT_OK;
  if ((total & 255) || (reinterpret_cast<uintptr_t>(d_in) & 15))
    return set_error(ZT_E_INTERNAL, "find_members: unaligned packed input");
  const uint64_t grid = (total + kFmSpan - 1) / kFmSpan;
  if (grid > 0x7FFFFFFFull) return set_error(ZT_E_ARG, "batch too large");
  find_members<<<(unsigned)grid, kFmThreads, 0, s>>>(d_in, total, d_item_off, d_item_len, count, d_list, cap, d_found);
  ZT_HIP(hipGetLastError());
  return ZT_OK;
}

}  // namespace zt
