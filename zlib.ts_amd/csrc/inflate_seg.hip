// inflate_seg.hip -- parallel inflate of one large stream (host orchestration).
//
// This engine's deflate ends every 32 KiB block on a byte-aligned empty stored
// block (00 00 FF FF: a *sync point* after it) and starts an independent
// 1 MiB segment with two more (the 10-byte restart marker
// 00 00 00 FF FF 00 00 00 FF FF; no match reaches behind it).  Streams that
// carry sync points are decoded in two phases (inflate_tok.hip):
//   1. find_syncs: every byte position is tested for the pattern (one 16-byte
//      window per thread, HBM-bound); sync points are appended, flagged when
//      the full restart marker precedes them;
//   2. tokenize_kernel: one wave per unit (stream start, or a sync point)
//      decodes blocks to tokens until it reaches another sync point;
//      (the candidate list is sorted and deduplicated, and the units' jobs
//      written, on the device: rocPRIM radix sort + scans; each unit's token
//      slot is bounded by the input bits up to the next candidate);
//   3. the host follows the chain from the stream start (unit -> the sync
//      point it stopped on -> the unit starting there ...), so sync points
//      that lie inside data are never used, and cuts the chain into segments
//      at restart markers; output offsets are the prefix sums of the units'
//      output lengths;
//   4. resolve_kernel: one wave per segment writes the bytes to their final
//      place.
// Any error on the chain, a unit that outgrew its token slot, or a match
// reaching behind a segment start returns 1: the caller then decodes the
// stream with one wave (inflate.hip), which also yields the reference's
// exact error.  Results are identical to the sequential decode by
// construction.  Replaces src/RawInflate.ts:127-143 for such streams.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/warp/warp_scan.hpp>

#include "index_host.h"
#include "zt_internal.h"

namespace zt {

namespace {

constexpr uint32_t kMaxSync = 1u << 22;

// ZT_INF_DEBUG=1: report why a stream left the two-phase path
bool inf_debug() {
  static const bool on = getenv("ZT_INF_DEBUG") != nullptr;
  return on;
}
#define FALLBACK(...)                                   \
  do {                                                  \
    if (inf_debug()) fprintf(stderr, "[zt inflate] " __VA_ARGS__); \
    return 1;                                           \
  } while (0)
// this engine's units are one DEFLATE block of DF_GROUP parse blocks
// (zt_internal.h): <= 1 token per byte
constexpr uint32_t kUnitTokCap = DF_BLOCK * DF_GROUP + 64;
static_assert(kUnitTokCap < (1u << 30), "token counts stay below TokResult::ntok's flag bits");
static_assert(kUnitTokCap == kIdxUnitTokCap, "the index validation's bound is the unit token capacity");

// sync point = byte after an aligned 00 00 FF FF; list entry = pos << 1 | restart
// One 16-byte aligned chunk per lane, loaded as one 16-byte word; the 8 bytes
// before it and the 12 after come from the neighbouring lanes (lanes at a
// wave's edge load them).  A sync point is 00 00 FF FF (u32 0xFFFF0000 at the
// candidate) ending at p; a restart point is the double marker
// 00 00 00 FF FF 00 | 00 00 FF FF before it.
__device__ __forceinline__ uint32_t fs_word(const uint8_t *in, uint64_t n, int64_t q) {
  // 4 bytes at q (bytes outside [0, n) read as 1: never part of a pattern)
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t x = q + k;
    v |= (uint32_t)((x >= 0 && (uint64_t)x < n) ? in[x] : 1) << (8 * k);
  }
  return v;
}
#ifndef ZT_FS_ITER
#define ZT_FS_ITER 8  // 4 / 8 / 16: 0.305 / 0.256 / 0.337 ms per GiB (each workgroup's one atomic on the shared counter; gpurun_out/r05ay)
#endif
constexpr uint32_t FS_ITER = ZT_FS_ITER;  // 4 KiB spans per workgroup (fewer, longer workgroups)
constexpr uint32_t kFsLocal = 64;  // sync candidates a workgroup gathers before its one global atomic
// Workgroup k appends to list region k % FS_SPLIT (its own counter, in its own
// 128-byte line): one counter took every workgroup's atomic, serialised where
// device-scope atomics execute; fs_gather then packs the regions
#ifndef ZT_FS_SPLIT
#define ZT_FS_SPLIT 64
#endif
constexpr uint32_t FS_SPLIT = ZT_FS_SPLIT;
constexpr uint32_t kFsRegion = kMaxSync / FS_SPLIT;  // candidates per region (more: the stream leaves this path)
constexpr uint32_t kFsCountStride = 32;             // u32 counters 128 bytes apart
#ifndef ZT_FS_NT
#define ZT_FS_NT 1
#endif
__global__ __launch_bounds__(256) void find_syncs(const uint8_t *__restrict__ in, uint64_t lo, uint64_t n,
                                                  uint64_t *__restrict__ list, uint32_t *__restrict__ count) {
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63;
  uint32_t *rcount = count + (blockIdx.x % FS_SPLIT) * kFsCountStride;
  uint64_t *rlist = list + (uint64_t)(blockIdx.x % FS_SPLIT) * kFsRegion;
  __shared__ uint32_t s_n, s_base;
  __shared__ uint64_t s_list[kFsLocal];
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  // A wave scans FS_ITER contiguous KiB (1 KiB per step, 16 bytes per lane):
  // the bytes around a lane's chunk come from its neighbours, across steps
  // from the previous step's lane 63 / the next step's lane 0, and only the
  // wave's two ends are loaded apart -- with the chunks, all in flight at once
  const uint32_t wv = threadIdx.x >> 6;
  const uint64_t wbase = (lo & ~uint64_t(15)) + ((uint64_t)blockIdx.x * FS_ITER * 256 + (uint64_t)wv * FS_ITER * 64) * 16;
  const bool in16 = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
  const bool aligned = (reinterpret_cast<uintptr_t>(in) & 3) == 0;
  const uint32_t *in32 = reinterpret_cast<const uint32_t *>(in);
  auto edge = [&](int64_t q) -> uint32_t {  // 4 bytes at q, as fs_word
    return aligned && q >= 0 && (uint64_t)q + 4 <= n ? in32[q / 4] : fs_word(in, n, q);
  };
  u32x4 pre[FS_ITER];
#pragma unroll
  for (uint32_t it = 0; it < FS_ITER; ++it) {
    const uint64_t base = wbase + ((uint64_t)it * 64 + lane) * 16;
    pre[it] = base + 16 <= n && in16
                  ? (ZT_FS_NT ? __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(in + base))
                             : *reinterpret_cast<const u32x4 *>(in + base))
                  : u32x4{0u, 0u, 0u, 0u};
  }
  // lane 0: the 8 bytes before the wave's span; lane 63: the 12 after it
  uint32_t e0 = 0, e1 = 0, e2 = 0;
  if (lane == 0) {
    e0 = edge((int64_t)wbase - 8);
    e1 = edge((int64_t)wbase - 4);
  }
  if (lane == 63) {
    const int64_t q = (int64_t)(wbase + (uint64_t)FS_ITER * 1024);
    e0 = edge(q);
    e1 = edge(q + 4);
    e2 = edge(q + 8);
  }
  uint32_t c0 = e0, c1 = e1;  // lane 0: the 8 bytes before this step's chunk
#pragma unroll
  for (uint32_t it = 0; it < FS_ITER; ++it) {
  const uint64_t base = wbase + ((uint64_t)it * 64 + lane) * 16;
  // words: w[0..1] = bytes [base - 8, base), w[2..5] = [base, base + 16), w[6..8] = [base + 16, base + 28)
  uint32_t w[9];
  const bool whole = base + 16 <= n && in16;
  if (whole) {
    const u32x4 v = pre[it];
    w[2] = v.x;
    w[3] = v.y;
    w[4] = v.z;
    w[5] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) w[2 + k] = fs_word(in, n, (int64_t)base + 4 * k);
  }
  w[0] = (uint32_t)__shfl_up((int)w[4], 1, 64);
  w[1] = (uint32_t)__shfl_up((int)w[5], 1, 64);
  w[6] = (uint32_t)__shfl_down((int)w[2], 1, 64);
  w[7] = (uint32_t)__shfl_down((int)w[3], 1, 64);
  w[8] = (uint32_t)__shfl_down((int)w[4], 1, 64);
  if (lane == 0) {
    w[0] = c0;
    w[1] = c1;
  }
  c0 = (uint32_t)__builtin_amdgcn_readlane((int)w[4], 63);
  c1 = (uint32_t)__builtin_amdgcn_readlane((int)w[5], 63);
  if (it + 1 < FS_ITER) {
    // the next step's first 12 bytes: lane 0's chunk there when it is whole
    const uint64_t nb = wbase + (uint64_t)(it + 1) * 1024;
    const bool nwhole = nb + 16 <= n && in16;
    const uint32_t x0 = (uint32_t)__builtin_amdgcn_readlane((int)pre[it + 1].x, 0);
    const uint32_t x1 = (uint32_t)__builtin_amdgcn_readlane((int)pre[it + 1].y, 0);
    const uint32_t x2 = (uint32_t)__builtin_amdgcn_readlane((int)pre[it + 1].z, 0);
    if (lane == 63) {
      w[6] = nwhole ? x0 : fs_word(in, n, (int64_t)nb);
      w[7] = nwhole ? x1 : fs_word(in, n, (int64_t)nb + 4);
      w[8] = nwhole ? x2 : fs_word(in, n, (int64_t)nb + 8);
    }
  } else if (lane == 63) {
    w[6] = e0;
    w[7] = e1;
    w[8] = e2;
  }
  if (base >= n) continue;
  auto at = [&](int x) -> uint32_t {  // 4 bytes at base - 8 + x (0 <= x <= 32)
    return (x & 3) ? __builtin_amdgcn_alignbyte(w[(x >> 2) + 1], w[x >> 2], x & 3) : w[x >> 2];
  };
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (at(8 + j) == 0xFFFF0000u) {
      const uint64_t p = base + j + 4;
      if (p > lo && p < n) {
        // bytes base + j - 6 .. base + j - 1: 00 00 00 FF FF 00
        const bool restart = base + j >= 6 && at(2 + j) == 0xFF000000u && (at(6 + j) & 0xFFFFu) == 0x00FFu;
        // gathered per workgroup (one global atomic per workgroup)
        const uint64_t v = (p << 1) | (restart ? 1 : 0);
        const uint32_t k = atomicAdd(&s_n, 1u);
        if (k < kFsLocal) {
          s_list[k] = v;
        } else {
          const uint32_t g = atomicAdd(rcount, 1u);
          if (g < kFsRegion) rlist[g] = v;
        }
      }
    }
  }
  }
  __syncthreads();
  const uint32_t m = s_n < kFsLocal ? s_n : kFsLocal;
  if (threadIdx.x == 0 && m) s_base = atomicAdd(rcount, m);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < m; i += 256)
    if (s_base + i < kFsRegion) rlist[s_base + i] = s_list[i];
}

// the FS_SPLIT regions of find_syncs packed into `out` (region order; the
// sort that follows makes the order irrelevant), one workgroup per region;
// *total = the candidates, or kMaxSync + 1 when a region overflowed
__global__ __launch_bounds__(256) void fs_gather(const uint64_t *__restrict__ list, const uint32_t *__restrict__ count,
                                                 uint64_t *__restrict__ out, uint32_t *__restrict__ total) {
  const uint32_t r = blockIdx.x;
  __shared__ uint32_t s_off, s_over;
  if (threadIdx.x < 64) {
    uint32_t below = 0, all = 0, over = 0;
    for (uint32_t q = threadIdx.x; q < FS_SPLIT; q += 64) {
      const uint32_t c = count[q * kFsCountStride];
      over |= c > kFsRegion ? 1u : 0u;
      all += c;
      below += q < r ? c : 0u;
    }
    for (int o = 32; o; o >>= 1) {
      below += (uint32_t)__shfl_xor((int)below, o, 64);
      all += (uint32_t)__shfl_xor((int)all, o, 64);
      over |= (uint32_t)__shfl_xor((int)over, o, 64);
    }
    if (threadIdx.x == 0) {
      s_off = below;
      s_over = over;
      if (r == 0) *total = over ? kMaxSync + 1 : all;
    }
  }
  __syncthreads();
  if (s_over) return;
  const uint32_t c = count[r * kFsCountStride];
  const uint64_t *src = list + (uint64_t)r * kFsRegion;
  for (uint32_t i = threadIdx.x; i < c; i += 256) out[s_off + i] = src[i];
}

// sorted candidates (pos << 1 | restart) -> first of each position
__global__ __launch_bounds__(256) void unit_flags(const uint64_t *__restrict__ key, uint32_t cnt,
                                                  uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i > cnt) return;
  flag[i] = i < cnt && (i == 0 || (key[i] >> 1) != (key[i - 1] >> 1)) ? 1u : 0u;
}

// unit k + 1 starts at the k-th distinct sync point (unit 0 at `index`);
// pos[cnt] = the number of distinct sync points.  Token slot of a unit: every
// token takes at least one input bit, and a real unit ends at the next real
// sync point, so min(cap, 8 x the bytes up to the next candidate + 64)
// holds it (a false candidate inside a real unit's block can only make that
// unit overflow its slot: the stream then leaves this path).  Without the
// bound, every one of a crafted input's dense false candidates took a whole
// block's slot (~128 KiB each).
__global__ __launch_bounds__(256) void unit_jobs(const uint64_t *__restrict__ key, const uint32_t *__restrict__ flag,
                                                 const uint32_t *__restrict__ pos, uint32_t cnt, uint64_t n,
                                                 uint64_t index, uint32_t cap, uint64_t *__restrict__ sync,
                                                 uint8_t *__restrict__ restart, TokJob *__restrict__ jobs,
                                                 uint64_t *__restrict__ slot, uint32_t *__restrict__ nrestart,
                                                 uint32_t *__restrict__ span_key, uint32_t *__restrict__ unit_id) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  auto job = [&](uint32_t u, uint64_t start, uint64_t next) {
    // (launch order: the longest input span first -- sorted on a 20-bit
    // key, spans of 1 MiB and more tied first)
    const uint64_t span = next > start ? next - start : 0;
    if (span_key) {
      span_key[u] = 0xFFFFFu - (uint32_t)(span < 0xFFFFFull ? span : 0xFFFFFull);
      unit_id[u] = u;
    }
    TokJob j;
    j.start = start;
    j.tok_off = 0;  // unit_slots
    const uint64_t room = (next > start ? next - start : 0) * 8 + 64;
    j.tok_cap = (uint32_t)(room < cap ? room : cap);
    j.stop_first = u;  // sync[u] is the first sync point after start
    j.end = 0;
    jobs[u] = j;
    slot[u] = (j.tok_cap + 63) & ~63u;
  };
  if (i == 0) job(0, index, cnt ? key[0] >> 1 : n);
  if (i >= cnt || !flag[i]) return;
  const uint32_t k = pos[i];
  const uint64_t p = key[i] >> 1;
  uint32_t j = i + 1;
  while (j < cnt && (key[j] >> 1) == p) ++j;
  sync[k] = p;
  restart[k] = (uint8_t)(key[i] & 1);
  if (key[i] & 1) atomicAdd(nrestart, 1u);
  job(k + 1, p, j < cnt ? key[j] >> 1 : n);
}

// token offsets = exclusive scan of the slots; total[0] = all slots
__global__ __launch_bounds__(256) void unit_slots(const uint64_t *__restrict__ off, const uint64_t *__restrict__ slot,
                                                  const uint32_t *__restrict__ nunits_m1, TokJob *__restrict__ jobs,
                                                  uint64_t *__restrict__ total) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  const uint32_t units = *nunits_m1 + 1;
  if (u >= units) return;
  jobs[u].tok_off = off[u];
  if (u + 1 == units) total[0] = off[u] + slot[u];
}

}  // namespace

// ---- the chain on the device (the common case) --------------------------------
// When every unit is on the chain in order -- unit u stops at sync point u and
// the last one at BFINAL, i.e. no false sync-point candidate -- the chain, its
// copy segments and their descriptor offsets are prefix sums, and one
// workgroup builds them where the host walk needed every unit's result back
// over PCIe and the chain sent down again (a host round trip between tokenize
// and expand).  Anything else (a false candidate, a unit error, an output past
// the capacity, more segments than the bound) leaves info->ok = 0: expand and
// copy return at once and the host walks the chain as before.  Segment rules
// as the host walk's: a segment starts at unit 0 and at the first unit after
// a restart point that has output bytes since the previous restart point
// (empty segments merge into the next); its descriptors start 512-aligned; a
// segment of stored runs only is copied by expand_kernel (SegJob count bit 31).
constexpr int CH_T = 1024;
constexpr uint32_t CH_MAXU = 40960;  // units (LDS: 2 B each): 1.25 GiB of 32 KiB blocks
constexpr int CH_B = 8;              // rounds whose loads are in flight together
constexpr uint32_t CH_MAXS = 2048;   // segments (LDS)

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64);
  const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}
struct AddU64 {
  __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
};
struct MaxU64 {
  __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; }
};
// exclusive scan over the workgroup's CH_T threads (identity 0); *total = the reduction
template <typename Op>
__device__ uint64_t block_excl_scan(uint64_t v, Op op, uint64_t *wsum, uint64_t *total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t x = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t y = shfl_up64(x, d);
    if (lane >= d) x = op(x, y);
  }
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  if (w == 0) {
    uint64_t sw = lane < CH_T / 64 ? wsum[lane] : 0;
    for (int d = 1; d < CH_T / 64; d <<= 1) {
      const uint64_t y = shfl_up64(sw, d);
      if (lane >= d) sw = op(sw, y);
    }
    if (lane < CH_T / 64) wsum[lane] = sw;
  }
  __syncthreads();
  uint64_t ex = shfl_up64(x, 1);
  if (lane == 0) ex = 0;
  const uint64_t r = op(w ? wsum[w - 1] : 0, ex);
  if (total) *total = wsum[CH_T / 64 - 1];
  __syncthreads();
  return r;
}

// wave w owns units [w * wu, (w + 1) * wu), taken 64 at a time (lane = unit:
// every global access coalesced); running values cross rounds in registers
// and waves through one workgroup scan
__global__ __launch_bounds__(CH_T) void chain_kernel(const TokResult *__restrict__ res, const uint8_t *__restrict__ restart,
                                                     const uint64_t *__restrict__ tok_off, uint32_t units,
                                                     uint64_t out_cap, uint64_t desc_cap, uint32_t max_seg,
                                                     ChainUnit *__restrict__ cu, SegJob *__restrict__ sj,
                                                     ChainInfo *__restrict__ info, uint32_t *__restrict__ ekey,
                                                     uint32_t *__restrict__ eid) {
  __shared__ uint16_t ol[CH_MAXU];              // unit output bytes (<= 65535 here)
  __shared__ uint32_t candb[CH_MAXU / 32];      // unit follows a restart point (or is unit 0)
  __shared__ uint32_t dirb[CH_MAXU / 32];       // unit is stored runs only, or empty
  __shared__ uint64_t seg_off[CH_MAXS + 1];     // output offset of segment k's first unit; [nseg] = total
  __shared__ uint64_t seg_desc[CH_MAXS];
  __shared__ uint32_t seg_first[CH_MAXS + 1];
  __shared__ uint32_t seg_direct[CH_MAXS];
  __shared__ uint64_t wsum[CH_T / 64];
  __shared__ int bad;
  const uint32_t t = threadIdx.x;
  const int lane = t & 63;
  const uint32_t w = t >> 6, nw = CH_T / 64;
  const uint32_t wu = ((units + nw - 1) / nw + 63) & ~63u;  // units per wave, whole rounds
  const uint32_t w0 = w * wu < units ? w * wu : units, w1 = w0 + wu < units ? w0 + wu : units;
  if (t == 0) bad = 0;
  for (uint32_t i = t; i < CH_MAXU / 32; i += CH_T) candb[i] = dirb[i] = 0;
  for (uint32_t i = t; i < CH_MAXS; i += CH_T) seg_direct[i] = 1;
  __syncthreads();
  // A: the unit results into LDS (CH_B rounds' loads in flight); every unit
  // on the chain in order; the wave's bytes
  bool ok = true;
  uint64_t wlen = 0;
  for (uint32_t r0 = w0; r0 < w1; r0 += 64 * CH_B) {
    uint64_t olen[CH_B];
    int32_t st[CH_B], stop[CH_B];
    uint32_t ntok[CH_B];
    uint8_t rs[CH_B];
#pragma unroll
    for (int j = 0; j < CH_B; ++j) {
      const uint32_t v = r0 + 64 * j + lane, u = v < w1 ? v : w0;
      olen[j] = res[u].out_len;
      st[j] = res[u].status;
      stop[j] = res[u].stop_idx;
      ntok[j] = res[u].ntok;
      rs[j] = restart[u ? u - 1 : 0];
    }
#pragma unroll
    for (int j = 0; j < CH_B; ++j) {
      const uint32_t u = r0 + 64 * j + lane;
      if (u >= w1) continue;
      ok = ok && st[j] == ZT_OK && olen[j] <= 0xFFFFull && (u + 1 < units ? stop[j] == (int32_t)u : stop[j] < 0);
      ol[u] = (uint16_t)olen[j];
      wlen += olen[j];
      if (u == 0 || rs[j] != 0) atomicOr(&candb[u >> 5], 1u << (u & 31));
      if ((ntok[j] >> 30) == 3u || olen[j] == 0) atomicOr(&dirb[u >> 5], 1u << (u & 31));
    }
  }
  if (!ok) bad = 1;
  for (int o = 32; o; o >>= 1) wlen += ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(wlen >> 32), o, 64) << 32) |
                                       (uint32_t)__shfl_xor((int)(uint32_t)wlen, o, 64);
  uint64_t total;
  const uint64_t wbase = block_excl_scan(lane == 0 ? wlen : 0, AddU64(), wsum, &total);  // (one lane per wave)
  const uint64_t base = __shfl((int)(uint32_t)wbase, 0, 64) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(wbase >> 32), 0, 64) << 32);
  auto cand = [&](uint32_t u) { return u < w1 && ((candb[u >> 5] >> (u & 31)) & 1u); };
  // One round of 64 units: u's output offset o (the round's sums are 32-bit:
  // units <= 65535 bytes), whether u starts a segment (a restart point with
  // output since the previous one: pcr = that one's offset before the round),
  // and the running values for the next round (wave scans by DPP, rocPRIM).
  using WScan = rocprim::warp_scan<uint32_t, 64>;
  __shared__ typename WScan::storage_type wst[CH_T / 64];
  struct Round {
    uint64_t o;
    bool start;
  };
  auto round = [&](uint32_t u, uint32_t l, uint64_t &off, uint64_t &pcr) -> Round {
    uint32_t inc;
    WScan().inclusive_scan(l, inc, wst[w], rocprim::plus<uint32_t>());
    const uint64_t o = off + inc - l;
    const bool c = cand(u);
    const uint32_t cv = c ? inc - l + 1 : 0u;  // 1 + the round-local offset of a restart point
    uint32_t ex;
    WScan().exclusive_scan(cv, ex, 0u, wst[w], rocprim::maximum<uint32_t>());
    const uint64_t before = ex ? off + ex - 1 : pcr;
    const uint32_t rmax = (uint32_t)__shfl((int)(ex > cv ? ex : cv), 63, 64);
    const bool start = u < w1 && (u == 0 || (c && o > before));
    if (rmax) pcr = off + rmax - 1;
    off += (uint32_t)__shfl((int)inc, 63, 64);
    return Round{o, start};
  };
  // B: output offset of the wave's last restart point (non-decreasing: a max-scan)
  uint64_t off = base, last = 0;
  for (uint32_t r0 = w0; r0 < w1; r0 += 64) {
    const uint32_t u = r0 + lane;
    (void)round(u, u < w1 ? ol[u] : 0u, off, last);
  }
  const uint64_t prevw = block_excl_scan(lane == 0 ? last : 0, MaxU64(), wsum, nullptr);
  const uint64_t prev = __shfl((int)(uint32_t)prevw, 0, 64) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(prevw >> 32), 0, 64) << 32);
  // C: segment starts per wave
  uint64_t nstart = 0, pc = prev;
  off = base;
  for (uint32_t r0 = w0; r0 < w1; r0 += 64) {
    const uint32_t u = r0 + lane;
    const Round r = round(u, u < w1 ? ol[u] : 0u, off, pc);
    nstart += __popcll(__ballot(r.start));
  }
  uint64_t nseg64;
  const uint64_t sbw = block_excl_scan(lane == 0 ? nstart : 0, AddU64(), wsum, &nseg64);
  const uint32_t sbase = (uint32_t)__shfl((int)(uint32_t)sbw, 0, 64);
  const uint32_t nseg = (uint32_t)nseg64;
  if (bad || total > out_cap || nseg > max_seg || nseg > CH_MAXS) {
    if (t == 0) info->ok = 0;
    return;  // (uniform: bad was set before the scans' barriers)
  }
  // D: the segment table; a segment is direct when all its units are stored runs (or empty)
  uint32_t k = sbase;  // segments started before this round
  pc = prev;
  off = base;
  for (uint32_t r0 = w0; r0 < w1; r0 += 64) {
    const uint32_t u = r0 + lane;
    const Round r = round(u, u < w1 ? ol[u] : 0u, off, pc);
    const uint64_t sm = __ballot(r.start);
    const uint32_t g = k + (uint32_t)__popcll(sm & ((2ull << lane) - 1)) - 1;  // this unit's segment
    if (r.start) {
      seg_first[g] = u;
      seg_off[g] = r.o;
    }
    if (u < w1 && !((dirb[u >> 5] >> (u & 31)) & 1)) seg_direct[g] = 0;
    k += (uint32_t)__popcll(sm);
  }
  if (t == 0) {
    seg_first[nseg] = units;
    seg_off[nseg] = total;
  }
  __syncthreads();
  // E: descriptor offsets, each segment 512-aligned
  const uint32_t sper = (nseg + CH_T - 1) / CH_T;
  const uint32_t s0 = t * sper < nseg ? t * sper : nseg, s1 = s0 + sper < nseg ? s0 + sper : nseg;
  uint64_t dl = 0;
  for (uint32_t q = s0; q < s1; ++q) dl += (seg_off[q + 1] - seg_off[q] + 511) & ~uint64_t(511);
  uint64_t db = block_excl_scan(dl, AddU64(), wsum, nullptr);
  for (uint32_t q = s0; q < s1; ++q) {
    seg_desc[q] = db;
    db += (seg_off[q + 1] - seg_off[q] + 511) & ~uint64_t(511);
  }
  __syncthreads();
  const uint64_t desc_total = seg_desc[nseg - 1] + (total - seg_off[nseg - 1]);
  if (desc_total + 1024 > desc_cap) {
    if (t == 0) info->ok = 0;
    return;  // (uniform)
  }
  // F: chain units (coalesced) and segment jobs
  k = sbase;
  pc = prev;
  off = base;
  for (uint32_t b0 = w0; b0 < w1; b0 += 64 * CH_B) {
    uint64_t to[CH_B];
    uint32_t nt[CH_B];
#pragma unroll
    for (int j = 0; j < CH_B; ++j) {  // CH_B rounds' loads in flight (each round waited alone: 0.1 ms)
      const uint32_t v = b0 + 64 * j + lane, uu = v < w1 ? v : w0;
      to[j] = tok_off[uu];
      nt[j] = res[uu].ntok;
    }
#pragma unroll
    for (int j = 0; j < CH_B; ++j) {
      const uint32_t r0 = b0 + 64 * j;
      if (r0 >= w1) break;  // (wave-uniform)
      const uint32_t u = r0 + lane;
      const uint32_t l = u < w1 ? ol[u] : 0u;
      const Round r = round(u, l, off, pc);
      const uint64_t sm = __ballot(r.start);
      const uint32_t g = k + (uint32_t)__popcll(sm & ((2ull << lane) - 1)) - 1;
      if (u < w1) {
        ChainUnit x;
        x.tok_off = to[j];
        x.out_off = r.o;
        x.seg_off = seg_off[g];
        x.desc_off = seg_desc[g] + (r.o - seg_off[g]);
        x.ntok = seg_direct[g] ? nt[j] : (nt[j] & ~0x40000000u);
        x.out_len = l;
        cu[u] = x;
        if (ekey) {  // expand's launch order: most tokens first (17-bit key)
          const uint32_t nt = x.ntok & 0x3FFFFFFFu;
          ekey[u] = 0x1FFFFu - (nt < 0x1FFFFu ? nt : 0x1FFFFu);
          eid[u] = u;
        }
      }
      k += (uint32_t)__popcll(sm);
    }
  }
  for (uint32_t q = t; q < nseg; q += CH_T)
    sj[q] = SegJob{seg_first[q], (seg_first[q + 1] - seg_first[q]) | (seg_direct[q] ? 0x80000000u : 0u)};
  if (t == 0) {
    info->ok = 1;
    info->nseg = nseg;
    info->total = total;
    info->end_bits = res[units - 1].end_bits;
    info->desc_total = desc_total;
  }
}

// ZT_INF_TIMING=1: host wall time of inflate_segments_dev's stages on stderr (measurement only)
#define IT(label) ZT_STAMP("ZT_INF_TIMING", "inflate", label)

// a unit of the chain starts at byte `pos` (the device chain: every unit is
// on it); flag[0] |= 1 then
__global__ void unit_starts_at(const TokJob *__restrict__ jobs, uint32_t units, uint64_t pos, uint32_t *flag) {
  for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x)
    if (jobs[u].start == pos) atomicOr(flag, 1u);
}

// The index entries (index_host.h: IdxEntry) of a proven chain, one lane per
// unit: chain unit k is unit on_chain[k] of the tables (null: unit k, the
// device-built chain, which holds every unit); entry nchain is the sentinel.
__global__ __launch_bounds__(256) void index_pack_kernel(const TokJob *__restrict__ jobs,
                                                         const TokResult *__restrict__ res,
                                                         const uint8_t *__restrict__ restart,
                                                         const ChainUnit *__restrict__ cu,
                                                         const uint32_t *__restrict__ on_chain, uint32_t nchain,
                                                         uint64_t end_ip, uint64_t total, IdxEntry *__restrict__ out) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k > nchain) return;
  IdxEntry e;
  if (k == nchain) {
    e = IdxEntry{end_ip, total, 0u, 0u};
  } else {
    const uint32_t u = on_chain ? on_chain[k] : k;
    e.in_off = jobs[u].start;
    e.out_off = cu[k].out_off;
    e.ntok = res[u].ntok & 0x3FFFFFFFu;
    e.flags = (u == 0 || restart[u - 1] != 0) ? 1u : 0u;
  }
  out[k] = e;
}

namespace {

// room behind a device chain's statuses: its ChainInfo and the boundary flag
constexpr size_t kChainTail = 512;
static_assert(sizeof(ChainInfo) + 4 <= kChainTail, "tail holds the chain summary and the flag");

// ZT_TOK_DUMP=u: unit whose first SIMT block dumps its lane state (with ZT_TOK_CHECK)
uint32_t tok_dump_unit() { return getenv("ZT_TOK_DUMP") ? (uint32_t)atoi(getenv("ZT_TOK_DUMP")) : 0xFFFFFFFFu; }

// ---- inflate_segments_dev's stages -----------------------------------------------
// steps 1-2: the sync points found, sorted, deduplicated and turned into units
struct SegUnits {
  size_t units_max;   // candidates + 1: what the tables are sized for
  size_t units;       // distinct sync points + 1
  uint32_t nsync;     // distinct sync points
  uint32_t nrestart;  // of them, restart points
  uint64_t tok_total; // token slots of all units
  uint64_t *d_off;    // [units] token offsets (kSyncSort)
  // kTokMeta
  uint64_t *d_stops;
  uint8_t *d_restart;
  TokJob *d_jobs;
  TokResult *d_res;
  // kTokOrder: [span keys | unit ids | sorted keys | sorted ids | sort storage]
  bool lpt;  // launch order: longest first
  uint32_t *d_skey, *d_uid, *d_skey2, *d_order;
  void *d_ordtmp;
  size_t t_ord;
  int sort_order(hipStream_t s) const {  // d_order = unit ids by d_skey
    size_t t = t_ord;
    if (lpt && units > 1)
      ZT_HIP(rocprim::radix_sort_pairs(d_ordtmp, t, d_skey, d_skey2, d_uid, d_order, units, 0u, 20u, s));
    return ZT_OK;
  }
  const uint32_t *order() const { return lpt && units > 1 ? d_order : nullptr; }
};

int seg_find_units(DeviceCtx *c, const uint8_t *d_in, size_t n, size_t index, hipStream_t s, SegUnits *U) {
  // 1. sync points
  // [counters: FS_SPLIT lines | total][regions: kMaxSync][packed: kMaxSync]
  struct {
    uint32_t *rcount, *count;
    uint64_t *regions, *list;
  } C = {};
  ZT_TRY(scratch_carved(c, kSyncCand, [&](void *base) {
    Carve cv(base);
    C.rcount = cv.take<uint32_t>((size_t)FS_SPLIT * kFsCountStride + 64);  // (+ the total's own 256 bytes)
    C.regions = cv.take<uint64_t>(kMaxSync);
    C.list = cv.take<uint64_t>(kMaxSync);
    return cv.bytes();
  }));
  C.count = C.rcount + (size_t)FS_SPLIT * kFsCountStride;
  ZT_HIP(hipMemsetAsync(C.rcount, 0, (size_t)FS_SPLIT * kFsCountStride * 4, s));
  const uint64_t span = n - (index & ~size_t(15));
  const uint32_t grid = (uint32_t)((span + 16 * 256 * FS_ITER - 1) / (16 * 256 * FS_ITER));
  ZT_TRY(timing_begin(c, s, 2));
  find_syncs<<<grid, 256, 0, s>>>(d_in, index, n, C.regions, C.rcount);
  ZT_HIP(hipGetLastError());
  fs_gather<<<FS_SPLIT, 256, 0, s>>>(C.regions, C.rcount, C.list, C.count);
  ZT_HIP(hipGetLastError());
  uint32_t cnt = 0;
  ZT_TRY(readback(c, &cnt, C.count, 4, s));
  IT("sync points counted");
  if (cnt == 0 || cnt > kMaxSync) FALLBACK("%u sync points\n", cnt);
  // 2. the candidates sorted, deduplicated and turned into units on the
  // device (rocPRIM radix sort + scan): unit 0 starts at `index`, unit k + 1
  // at the k-th sync point
  int end_bit = 1;
  while (end_bit < 64 && ((uint64_t)n << 1 | 1) >> end_bit) ++end_bit;
  const size_t units_max = U->units_max = (size_t)cnt + 1;
  size_t t_sort = 0, t_scan = 0, t_scan64 = 0;
  ZT_HIP(rocprim::radix_sort_keys(nullptr, t_sort, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)cnt, 0u,
                                  (unsigned)end_bit, s));
  ZT_HIP(rocprim::exclusive_scan(nullptr, t_scan, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, units_max,
                                 rocprim::plus<uint32_t>(), s));
  ZT_HIP(rocprim::exclusive_scan(nullptr, t_scan64, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0,
                                 units_max, rocprim::plus<uint64_t>(), s));
  // kSyncSort: [rocPRIM storage | sorted keys | first-of-position flags |
  // their scan | slot sizes | token offsets | totals]
  uint8_t *sb = nullptr;
  uint64_t *d_key = nullptr, *d_slot = nullptr, *d_ttot = nullptr;
  uint32_t *d_flag = nullptr, *d_pos = nullptr;
  ZT_TRY(scratch_carved(c, kSyncSort, [&](void *base) {
    Carve cv(base);
    sb = cv.take<uint8_t>(std::max(t_sort, std::max(t_scan, t_scan64)));
    d_key = cv.take<uint64_t>(cnt);
    d_flag = cv.take<uint32_t>(units_max);
    d_pos = cv.take<uint32_t>(units_max);
    d_slot = cv.take<uint64_t>(units_max);
    U->d_off = cv.take<uint64_t>(units_max);
    d_ttot = cv.take<uint64_t>(3);  // [0] token slots in all, [1] (unused), [2] restart points (u32)
    return cv.bytes();
  }));
  ZT_HIP(rocprim::radix_sort_keys(sb, t_sort, C.list, d_key, (size_t)cnt, 0u, (unsigned)end_bit, s));
  const uint32_t g = (cnt + 1 + 255) / 256;
  unit_flags<<<g, 256, 0, s>>>(d_key, cnt, d_flag);
  ZT_HIP(hipGetLastError());
  ZT_HIP(rocprim::exclusive_scan(sb, t_scan, d_flag, d_pos, 0u, units_max, rocprim::plus<uint32_t>(), s));
  ZT_TRY(scratch_carved(c, kTokMeta, [&](void *base) {
    Carve cv(base);
    U->d_stops = cv.take<uint64_t>(cnt);
    U->d_restart = cv.take<uint8_t>(units_max);
    U->d_jobs = cv.take<TokJob>(units_max);
    U->d_res = cv.take<TokResult>(units_max);
    return cv.bytes();
  }));
  ZT_HIP(hipMemsetAsync(d_slot, 0, units_max * 8, s));
  ZT_HIP(hipMemsetAsync(d_ttot + 2, 0, 8, s));
  // tokenize launch order (kTokOrder)
  // (up to 128 K candidates: 4 GiB of 32 KiB blocks; a crafted stream of
  // dense false candidates keeps the position order and no order buffers)
  static const bool lpt_env = getenv("ZT_TOK_ORDER") ? atoi(getenv("ZT_TOK_ORDER")) != 0 : true;
  U->lpt = lpt_env && units_max <= (1u << 17);
  U->t_ord = 0;
  if (U->lpt)
    ZT_HIP(rocprim::radix_sort_pairs(nullptr, U->t_ord, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                     (const uint32_t *)nullptr, (uint32_t *)nullptr, units_max, 0u, 20u, s));
  ZT_TRY(scratch_carved(c, kTokOrder, [&](void *base) {
    Carve cv(base);
    const size_t k = U->lpt ? units_max : 1;
    U->d_skey = cv.take<uint32_t>(k);
    U->d_uid = cv.take<uint32_t>(k);
    U->d_skey2 = cv.take<uint32_t>(k);
    U->d_order = cv.take<uint32_t>(k);
    U->d_ordtmp = cv.take<uint8_t>(U->t_ord);
    return cv.bytes();
  }));
  unit_jobs<<<g, 256, 0, s>>>(d_key, d_flag, d_pos, cnt, n, index, kUnitTokCap, U->d_stops, U->d_restart, U->d_jobs,
                              d_slot, reinterpret_cast<uint32_t *>(d_ttot + 2), U->lpt ? U->d_skey : nullptr, U->d_uid);
  ZT_HIP(hipGetLastError());
  ZT_HIP(rocprim::exclusive_scan(sb, t_scan64, d_slot, U->d_off, (uint64_t)0, units_max, rocprim::plus<uint64_t>(), s));
  unit_slots<<<g, 256, 0, s>>>(U->d_off, d_slot, d_pos + cnt, U->d_jobs, d_ttot);
  ZT_HIP(hipGetLastError());
  void *mb;
  ZT_TRY(mailbox(c, 24, &mb));
  uint64_t *m64 = static_cast<uint64_t *>(mb);
  m64[1] = m64[2] = 0;
  ZT_TRY(x_copy(&m64[0], d_ttot, 8, s));
  ZT_TRY(x_copy(&m64[1], d_pos + cnt, 4, s));
  ZT_TRY(x_copy(&m64[2], d_ttot + 2, 4, s));
  ZT_HIP(hipStreamSynchronize(s));
  IT("units counted");
  U->tok_total = m64[0];
  U->nsync = (uint32_t)m64[1];
  U->nrestart = (uint32_t)m64[2];
  U->units = (size_t)U->nsync + 1;
  return ZT_OK;
}

// the unit tables in pinned staging (kPinInflateMeta), sized for the chain
// buffer's mirror behind them (chain_upload, the device chain's readback)
struct SegPinned {
  uint8_t *restart;
  TokResult *res;
  uint64_t *tok_off;
  size_t front;  // bytes of the three tables
  size_t bytes;
};
SegPinned seg_pinned(void *base, size_t units_max) {
  Carve cv(base);
  SegPinned P;
  P.restart = cv.take<uint8_t>(units_max);
  P.res = cv.take<TokResult>(units_max);
  P.tok_off = cv.take<uint64_t>(units_max);
  P.front = cv.bytes();
  P.bytes = P.front + chain_buf(nullptr, units_max, units_max, 0, kChainTail).bytes;
  return P;
}

// tokenize: the token slots, the launch order, the kernel
int seg_tokenize(DeviceCtx *c, const uint8_t *d_in, size_t n, const SegUnits &U, hipStream_t s, uint32_t **d_tok_out,
                 SegPinned *pin, uint64_t **dbg) {
  // Every candidate sync point gets a token slot before the chain shows which
  // are real block boundaries; the slots are bounded by the input bits up to
  // the next candidate (unit_jobs), so all of them together stay below 8
  // tokens per input byte + 64 per candidate.  Past the device's free memory,
  // or when the slots cannot be allocated, the stream takes the general path.
  const size_t tok_bytes = ((size_t)U.tok_total + 256) * 4;  // + slack: chunked token reads
  // (only asked when the cached slots are too small: hipMemGetInfo is a
  // driver round trip on every call otherwise)
  if (tok_bytes > c->buf_size[kTokens]) {
    size_t mem_free = 0, mem_total = 0;
    ZT_HIP(hipMemGetInfo(&mem_free, &mem_total));
    if (tok_bytes > c->buf_size[kTokens] + mem_free / 2)
      FALLBACK("%zu sync candidates: token slots over budget\n", U.units);
  }
  void *d_tok, *hp;
  if (scratch(c, kTokens, tok_bytes, &d_tok) != ZT_OK) FALLBACK("token slots (%zu B) not allocated\n", tok_bytes);
  // metadata comes back through pinned staging
  ZT_TRY(pinned(c, seg_pinned(nullptr, U.units_max).bytes, &hp, kPinInflateMeta));
  *pin = seg_pinned(hp, U.units_max);
  // longest units first: the kernel's last units are short ones, so its tail
  // (SIMDs idle while the last units finish) is short
  ZT_TRY(U.sort_order(s));
  TokParams tp;
  tp.in = d_in;
  tp.n = n;
  tp.order = U.order();
  tp.stops = U.d_stops;
  tp.nstops = U.nsync;
  tp.jobs = U.d_jobs;
  tp.res = U.d_res;
  tp.tokens = *d_tok_out = static_cast<uint32_t *>(d_tok);
  tp.count = (uint32_t)U.units;
  tp.simt = tok_simt_env();
  tp.dbg = nullptr;
  if (getenv("ZT_TOK_CHECK")) {
    void *d_dbg;
    ZT_TRY(scratch(c, kSmall, U.units * 64 + 8 * 64 * 32, &d_dbg));
    ZT_HIP(hipMemsetAsync(d_dbg, 0, U.units * 64 + 8 * 64 * 32, s));
    tp.dbg = static_cast<uint64_t *>(d_dbg);
  }
  *dbg = tp.dbg;
  tp.dump_unit = tok_dump_unit();
  tp.dump_once = 0;
  tp.run_tokens = 1;
  ZT_TRY(timing_begin(c, s, 3));
  ZT_TRY(tokenize_units_dev(tp, s));
  return timing_end(c, s, 3);
}

// ZT_TOK_CHECK / ZT_TOK_DUMP: what the tokenizer's debug words say (after the stream is synchronized)
int tok_check_print(const uint64_t *d_dbg, size_t units) {
  std::vector<uint64_t> dbg(units * 8);
  ZT_HIP(hipMemcpy(dbg.data(), d_dbg, units * 64, hipMemcpyDeviceToHost));
  size_t bad = 0;
  for (size_t i = 0; i < units; ++i)
    if (dbg[i * 8]) {
      if (bad++ < 8)
        fprintf(stderr, "[zt tok check] unit %zu body@%llu: end simt %llu scalar %llu, tokens %llu/%llu, bytes %llu/%llu\n",
                i, (unsigned long long)dbg[i * 8 + 1], (unsigned long long)dbg[i * 8 + 2],
                (unsigned long long)dbg[i * 8 + 3], (unsigned long long)dbg[i * 8 + 4],
                (unsigned long long)dbg[i * 8 + 5], (unsigned long long)dbg[i * 8 + 6],
                (unsigned long long)dbg[i * 8 + 7]);
    }
  fprintf(stderr, "[zt tok check] %zu of %zu units differ\n", bad, units);
  if (tok_dump_unit() < units) {
    std::vector<uint32_t> dd(8 * 64 * 8);
    ZT_HIP(hipMemcpy(dd.data(), d_dbg + units * 8, dd.size() * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < 8; ++r) {
      if (r > 0 && dd[(r * 64) * 8] == 0) break;
      fprintf(stderr, "round %d R=%u last=%d\n", r, dd[(r * 64) * 8], (int)dd[(r * 64) * 8 + 6]);
      for (int l = 0; l < 64; ++l) {
        const uint32_t *d = &dd[(r * 64 + l) * 8];
        fprintf(stderr, "  l%02d t=%u end=%u tok=%u e=%d fl=%u ev=%u\n", l, d[1], d[2], d[3], (int)d[4], d[5], d[7]);
      }
    }
  }
  return ZT_OK;
}

// what every stage from the chain on needs
struct SegCall {
  DeviceCtx *c;
  const uint8_t *d_in;
  size_t n;
  uint8_t **d_out_io;
  size_t out_cap;
  size_t *out_len, *end_ip;
  hipStream_t s;
  uint64_t boundary;
  std::vector<uint8_t> *index_blob = nullptr;  // the index build: receives the blob once the chain is proven
};

int seg_done(const SegCall &a, const ChainRun &run, const char *tag) {
  DeviceCtx *c = a.c;
  ZT_TRY(timing_collect(c, &c->times.inflate_ms, &c->times.inflate_launches, 2));
  ZT_TRY(timing_collect(c, &c->times.inflate_tok_ms, &c->times.inflate_toks, 3));
  for (uint32_t i = 0; i < run.nunits; ++i)
    if (run.host.unit_status[i] != ZT_OK)
      FALLBACK("unit %u of %u (%s): status %d\n", i, run.nunits, tag, run.host.unit_status[i]);
  for (uint32_t i = 0; i < run.nseg; ++i)
    if (run.host.seg_status[i] != ZT_OK) FALLBACK("segment %u of %u: status %d\n", i, run.nseg, run.host.seg_status[i]);
  c->times.inflate_paths[0]++;
  return ZT_OK;
}

// 3a. the common case: chain, segments and the resolve kernels straight on
// the device (a caller-owned output: its capacity bounds the descriptors).
// *resolved: the stream is done (ZT_OK) or left this path (1); otherwise the
// kernels did nothing and the host walks the chain.
int seg_chain_device(const SegCall &a, const SegUnits &U, const uint32_t *d_tok, const SegPinned &pin, bool plain,
                     bool *resolved) {
  DeviceCtx *c = a.c;
  hipStream_t s = a.s;
  *resolved = false;
  // ZT_INF_HOST_CHAIN=1 forces the host walk (measurement)
  static const bool host_chain = getenv("ZT_INF_HOST_CHAIN") != nullptr;
  const size_t units = U.units;
  const uint32_t max_seg = (uint32_t)std::min<uint64_t>((uint64_t)U.nrestart + 1, units);
  const uint64_t desc_cap = (uint64_t)a.out_cap + 512ull * max_seg + 2048;
  // The descriptors are sized from the caller's capacity here (the decoded
  // size is known only after the chain), and the scratch cache only grows: a
  // generous capacity takes the device chain only when its descriptors fit
  // what the descriptor slot already holds or 8 bytes per input byte (output
  // up to 4x the input); otherwise, and when the slot cannot grow, the host
  // walks the chain and sizes them from the real total.
  const bool desc_fits = desc_cap * 2 <= c->buf_size[kDeflateOrDesc] ||
                         desc_cap * 2 <= 8ull * a.n + 4ull * (512ull * max_seg + 2048);
  if (!*a.d_out_io || !plain || host_chain || max_seg > CH_MAXS || units > CH_MAXU || a.out_cap > (64ull << 30) ||
      !desc_fits)
    return ZT_OK;
  void *d_chain, *d_desc;
  ZT_TRY(scratch(c, kChain, chain_buf(nullptr, units, max_seg, 0, kChainTail).bytes, &d_chain));
  if (scratch(c, kDeflateOrDesc, desc_cap * 2, &d_desc) != ZT_OK) {
    (void)hipGetLastError();  // (the failed allocation's sticky error)
    return ZT_OK;
  }
  ChainRun run;
  run.dev = chain_buf(d_chain, units, max_seg, 0, kChainTail);
  run.host = chain_buf(pin.restart + pin.front, units, max_seg, 0, kChainTail);
  run.nunits = (uint32_t)units;
  run.nseg = max_seg;  // (grid; copy waves past info->nseg return at once)
  ChainInfo *d_info = reinterpret_cast<ChainInfo *>(run.dev.tail);
  uint32_t *d_bflag = reinterpret_cast<uint32_t *>(d_info + 1);
  if (a.boundary != ~0ull) {
    ZT_HIP(hipMemsetAsync(d_bflag, 0, 4, s));
    unit_starts_at<<<(uint32_t)std::min<size_t>(64, (units + 255) / 256), 256, 0, s>>>(U.d_jobs, (uint32_t)units,
                                                                                      a.boundary, d_bflag);
    ZT_HIP(hipGetLastError());
  }
  // (the tokenize order's buffers, free again, hold expand's: most tokens first)
  chain_kernel<<<1, CH_T, 0, s>>>(U.d_res, U.d_restart, U.d_off, (uint32_t)units, a.out_cap, desc_cap, max_seg,
                                  run.dev.units, run.dev.segs, d_info, U.lpt ? U.d_skey : nullptr, U.d_uid);
  ZT_HIP(hipGetLastError());
  ZT_TRY(U.sort_order(s));
  ResolveParams rp = resolve_params(run, d_tok, static_cast<uint16_t *>(d_desc), *a.d_out_io, 0, a.d_in);
  rp.info = d_info;
  rp.order = U.order();
  IT("device chain launched");
  ZT_TRY(resolve_segments_dev(rp, s));
  ZT_TRY(timing_end(c, s, 2));
  // back in one copy: every status, the chain summary and the boundary flag
  ZT_TRY(x_copy(run.host.unit_status, run.dev.unit_status,
                (size_t)(run.dev.tail - reinterpret_cast<uint8_t *>(run.dev.unit_status)) + sizeof(ChainInfo) + 4, s));
  ZT_HIP(hipStreamSynchronize(s));
  IT("resolved (device chain)");
  const ChainInfo info = *reinterpret_cast<const ChainInfo *>(run.host.tail);
  if (!info.ok)  // not the common case: the host walks the chain (the kernels above did nothing)
    return timing_begin(c, s, 2);
  *resolved = true;
  if (a.boundary != ~0ull && !*reinterpret_cast<const uint32_t *>(run.host.tail + sizeof(ChainInfo)))
    FALLBACK("no unit of the chain starts at the boundary %llu\n", (unsigned long long)a.boundary);
  run.nseg = info.nseg;
  ZT_TRY(seg_done(a, run, "device chain"));
  *a.out_len = info.total;
  *a.end_ip = (info.end_bits + 7) >> 3;
  return ZT_OK;
}

// the index of a chain that expand and copy have proved (no error, no match
// behind a segment start): packed on the device from the unit tables and the
// chain, one table back
int seg_index_pack(const SegCall &a, const SegUnits &U, const ChainPlan &plan, const ChainRun &run) {
  DeviceCtx *c = a.c;
  hipStream_t s = a.s;
  const size_t nchain = plan.chain.size();
  uint32_t *d_on = nullptr;
  IdxEntry *d_ent = nullptr;
  ZT_TRY(scratch_carved(c, kIndexPack, [&](void *base) {
    Carve cv(base);
    d_on = cv.take<uint32_t>(nchain);
    d_ent = cv.take<IdxEntry>(nchain + 1);
    return cv.bytes();
  }));
  ZT_HIP(hipMemcpyAsync(d_on, plan.on_chain.data(), nchain * 4, hipMemcpyHostToDevice, s));
  index_pack_kernel<<<(uint32_t)((nchain + 1 + 255) / 256), 256, 0, s>>>(U.d_jobs, U.d_res, U.d_restart, run.dev.units,
                                                                        d_on, (uint32_t)nchain, *a.end_ip, *a.out_len,
                                                                        d_ent);
  ZT_HIP(hipGetLastError());
  std::vector<uint8_t> &blob = *a.index_blob;
  blob.assign(index_blob_bytes(nchain), 0);
  ZT_TRY(readback(c, blob.data() + kIdxHeader, d_ent, (nchain + 1) * sizeof(IdxEntry), s));
  uint32_t nseg = 0;
  for (size_t k = 0; k < nchain; ++k) nseg += idx_get32(blob.data() + kIdxHeader + k * kIdxEntry + 20) & 1u;
  index_write_header(blob.data(), (uint32_t)nchain, nseg, idx_get64(blob.data() + kIdxHeader), *a.end_ip, *a.out_len);
  IT("index packed");
  return ZT_OK;
}

// 3b-4. the unit tables back to the host, the chain walked there
// (seg_chain_host), then expand (one wave per unit) and copy (one wave per
// segment)
int seg_chain_on_host(const SegCall &a, const SegUnits &U, const uint32_t *d_tok, const SegPinned &pin,
                      const uint64_t *d_dbg) {
  DeviceCtx *c = a.c;
  hipStream_t s = a.s;
  const size_t units = U.units;
  ZT_TRY(x_copy(pin.restart, U.d_restart, U.nsync, s));
  ZT_TRY(x_copy(pin.res, U.d_res, units * sizeof(TokResult), s));
  ZT_TRY(x_copy(pin.tok_off, U.d_off, units * 8, s));
  ZT_HIP(hipStreamSynchronize(s));
  IT("tokenized");
  if (d_dbg) ZT_TRY(tok_check_print(d_dbg, units));
  const ChainPlan plan = seg_chain_host(pin.res, pin.restart, pin.tok_off, units);
  if (plan.outcome != ChainPlan::kBuilt) {
    if (inf_debug()) fprintf(stderr, "[zt inflate] %s", plan.why.c_str());
    return plan.outcome == ChainPlan::kTruncated ? 2 : 1;
  }
  if (a.boundary != ~0ull) {
    std::vector<TokJob> hj(units);
    ZT_TRY(readback(c, hj.data(), U.d_jobs, units * sizeof(TokJob), s));
    bool at = false;
    for (uint32_t k : plan.on_chain) at = at || hj[k].start == a.boundary;
    if (!at) FALLBACK("no unit of the chain starts at the boundary %llu\n", (unsigned long long)a.boundary);
  }
  *a.out_len = plan.total;
  *a.end_ip = (pin.res[plan.last].end_bits + 7) >> 3;
  if (inf_debug()) {
    // segment sizes (copy_kernel: one wave per segment)
    uint64_t mn = ~0ull, mx = 0;
    size_t small = 0;
    for (const SegJob &sj : plan.segs) {
      const ChainUnit &f = plan.chain[sj.first], &b = plan.chain[sj.first + (sj.count & 0x7FFFFFFFu) - 1];
      const uint64_t len = b.out_off + b.out_len - f.out_off;
      mn = len < mn ? len : mn;
      mx = len > mx ? len : mx;
      small += len < (512u << 10);
    }
    fprintf(stderr, "[zt inflate] %zu units, %zu segments, %llu bytes: segment min %llu max %llu, %zu under 512 KiB\n",
            plan.chain.size(), plan.segs.size(), (unsigned long long)plan.total, (unsigned long long)mn,
            (unsigned long long)mx, small);
  }
  uint8_t *d_out = *a.d_out_io;
  if (!d_out) {  // caller wants a library-owned buffer
    void *p;
    ZT_TRY(scratch(c, kOut, plan.total ? plan.total : 1, &p));
    *a.d_out_io = d_out = static_cast<uint8_t *>(p);
  } else if (plan.total > a.out_cap) {  // (*out_len: the bytes needed)
    return set_error(ZT_E_ARG, "output capacity too small");
  }
  ChainRun run;
  IT("chain built");
  ZT_TRY(resolve_chain_dev(c, plan.chain, plan.segs, plan.desc_total, d_tok, d_out, 0, a.d_in, pin.front, &run, s));
  ZT_TRY(timing_end(c, s, 2));
  ZT_TRY(chain_statuses(run, s));
  IT("resolved");
  const int done = seg_done(a, run, "chain");
  if (done != ZT_OK || !a.index_blob) return done;
  return seg_index_pack(a, U, plan, run);
}

}  // namespace

int inflate_segments_dev(DeviceCtx *c, const uint8_t *d_in, size_t n, size_t index, uint8_t **d_out_io,
                         size_t out_cap, size_t *out_len, size_t *end_ip, hipStream_t s, uint64_t boundary) {
  IT("start");
  if (n < index + (1u << 14)) return 1;  // small: one wave is as fast
  SegUnits U;
  ZT_TRY(seg_find_units(c, d_in, n, index, s, &U));
  uint32_t *d_tok;
  SegPinned pin;
  uint64_t *d_dbg;
  ZT_TRY(seg_tokenize(c, d_in, n, U, s, &d_tok, &pin, &d_dbg));
  const SegCall a{c, d_in, n, d_out_io, out_cap, out_len, end_ip, s, boundary};
  bool resolved;
  const int rc = seg_chain_device(a, U, d_tok, pin, /*plain=*/!d_dbg && !inf_debug(), &resolved);
  if (rc || resolved) return rc;
  return seg_chain_on_host(a, U, d_tok, pin, d_dbg);
}

int inflate_index_build_dev(DeviceCtx *c, const uint8_t *d_in, size_t n, size_t index, uint8_t **d_out,
                            size_t *out_len, size_t *end_ip, std::vector<uint8_t> *blob, hipStream_t s) {
  IT("index build start");
  if (n <= index) return 1;
  SegUnits U;
  ZT_TRY(seg_find_units(c, d_in, n, index, s, &U));
  uint32_t *d_tok;
  SegPinned pin;
  uint64_t *d_dbg;
  ZT_TRY(seg_tokenize(c, d_in, n, U, s, &d_tok, &pin, &d_dbg));
  *d_out = nullptr;  // library-owned
  const SegCall a{c, d_in, n, d_out, 0, out_len, end_ip, s, ~0ull, blob};
  return seg_chain_on_host(a, U, d_tok, pin, d_dbg);
}

// chain_kernel on host tables (zt_internal.h)
extern "C" int zt_debug_chain(const TokResult *res, const uint8_t *restart, const uint64_t *tok_off, uint32_t units,
                              uint64_t out_cap, uint64_t desc_cap, uint32_t max_seg, ChainInfo *info, ChainUnit *cu,
                              SegJob *sj) {
  if (!res || !restart || !tok_off || !info || !cu || !sj || units == 0 || units > CH_MAXU || max_seg == 0)
    return set_error(ZT_E_ARG, "zt_debug_chain: bad argument");
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  hipStream_t s = c->stream;
  void *d_chain;
  TokResult *d_res = nullptr;
  uint8_t *d_restart = nullptr;
  uint64_t *d_off = nullptr;
  ZT_TRY(scratch_carved(c, kTokMeta, [&](void *base) {
    Carve cv(base);
    d_res = cv.take<TokResult>(units);
    d_restart = cv.take<uint8_t>(units);
    d_off = cv.take<uint64_t>(units);
    return cv.bytes();
  }));
  ZT_TRY(scratch(c, kChain, chain_buf(nullptr, units, max_seg, 0, kChainTail).bytes, &d_chain));
  const ChainBuf dev = chain_buf(d_chain, units, max_seg, 0, kChainTail);
  ZT_HIP(hipMemcpyAsync(d_res, res, units * sizeof(TokResult), hipMemcpyHostToDevice, s));
  ZT_HIP(hipMemsetAsync(d_restart, 0, 1, s));  // (the kernel reads restart[0] for a single unit too)
  if (units > 1) ZT_HIP(hipMemcpyAsync(d_restart, restart, units - 1, hipMemcpyHostToDevice, s));
  ZT_HIP(hipMemcpyAsync(d_off, tok_off, units * 8, hipMemcpyHostToDevice, s));
  ChainInfo *d_info = reinterpret_cast<ChainInfo *>(dev.tail);
  ZT_HIP(hipMemsetAsync(d_info, 0, sizeof(ChainInfo), s));
  chain_kernel<<<1, CH_T, 0, s>>>(d_res, d_restart, d_off, units, out_cap, desc_cap, max_seg, dev.units, dev.segs,
                                  d_info, nullptr, nullptr);
  ZT_HIP(hipGetLastError());
  ZT_HIP(hipMemcpyAsync(info, d_info, sizeof(ChainInfo), hipMemcpyDeviceToHost, s));
  ZT_HIP(hipStreamSynchronize(s));
  if (!info->ok) return ZT_OK;
  if (info->nseg > max_seg) return set_error(ZT_E_INTERNAL, "zt_debug_chain: more segments than the bound");
  ZT_HIP(hipMemcpyAsync(cu, dev.units, (size_t)units * sizeof(ChainUnit), hipMemcpyDeviceToHost, s));
  ZT_HIP(hipMemcpyAsync(sj, dev.segs, (size_t)info->nseg * sizeof(SegJob), hipMemcpyDeviceToHost, s));
  ZT_HIP(hipStreamSynchronize(s));
  return ZT_OK;
}

}  // namespace zt
