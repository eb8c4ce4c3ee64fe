// deflate.hip -- raw DEFLATE (RFC 1951) encoder on the GPU: the stages before
// the parse and the host driver of the whole pipeline.
// Replaces src/LZ77.ts (with deflate_post.hip: src/RawDeflate.ts, src/Heap.ts
// and src/Bitstream.ts).
//
//   0. classify_kernel -- one 256-thread workgroup per 32 KiB block: blocks
//      whose bytes cannot beat a stored block skip the search and the parse.
//   1. match_kernel -- one 1024-thread workgroup per super-chunk (4
//      consecutive 32 KiB blocks; a 1 MiB segment starts without history,
//      later super-chunks index the 28 KiB before them first).  4 KiB
//      sub-chunks stream through a 32 KiB LDS ring (28 608-byte window).
//      Wave 0 links 8-byte-key hash chains (u16 relative links; u32 heads,
//      u16 heads while a block measures through the queues below)
//      and wave 1 a 4-byte-key table (the newest earlier position per
//      bucket), each by lane-ordered LDS exchanges head[h] <-> p, 64
//      positions per exchange, publishing their progress; all waves search
//      256-position super-steps as soon as they are linked: per thread 4
//      positions, two chain walks interleaved (two LDS loads per hop: the
//      link and one filter word), candidates measured against 16 bytes held
//      in registers -- at once, or, in blocks whose first sub-chunk measured
//      many, 64 at a time through a per-wave LDS queue (the same matches);
//      matches shorter than the key come from near probes
//      (distances 1..16, register window) and the 4-byte table.  The
//      longest match of every position goes to HBM: res[i] = len << 16 |
//      dist.
//   2. price, optparse, parse, block, scan_sizes and encode turn res into the
//      stream: deflate_post.hip, launched by its deflate_post_run.
//
// The host driver (the end of this file): the level table, the work split
// over workgroups, the scratch layout and the deflate_* entry points, which
// launch classify -> match -> deflate_post_run and read the sizes back.
// stored_blocks writes compressionType NONE.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zt_internal.h"

namespace zt {

#ifdef ZT_DF_TIME
__device__ unsigned long long g_df_time[8];  // debug: cycles (thread 0 of each workgroup) in phases
#endif
#ifdef ZT_DF_COUNT
__device__ unsigned long long g_df_count[8];  // debug: pair steps (per wave), lane hops, extends (lanes), extends (waves),
                                              // measured lanes that improve / measure < 8 bytes / do not improve
                                              // (at once only), candidates queued (of the extends)
#endif
// blocks whose later sub-chunks measured through the queues / at once (zt_debug_match_modes)
__device__ unsigned long long g_match_modes[2];
// chain-head format changes of the match workgroups: u32 -> u16 / u16 -> u32 (zt_debug_head_formats)
__device__ unsigned long long g_head_formats[2];

constexpr int DF_SUB = 4096;
constexpr int DF_RING = 32768;  // power of two: ring index = rel & (DF_RING - 1)
// hash buckets of the 8-byte-key chains and of the 4-byte-key table (u32
// heads, no chains): with the ring, the chain links and the sub-chunk's
// 4-byte links they fill the 160 KiB of LDS.  The chain heads are u32 while a
// workgroup's blocks measure at once, and u16 -- two per word -- while they
// measure through the waves' queues, which then take the room of the upper
// halves (MatchShared); both formats give the same links and streams.
#ifndef ZT_DF_HSIZE
#define ZT_DF_HSIZE 12240  // (even: two u16 heads per word)
#endif
#ifndef ZT_DF_H4SIZE
#define ZT_DF_H4SIZE 2048
#endif
#ifndef ZT_DF_P4FAR
#define ZT_DF_P4FAR 1024  // 4-byte (not longer) matches from the 4-byte-key table reach at most this far
#endif
constexpr uint32_t DF_HSIZE = ZT_DF_HSIZE;
constexpr uint32_t DF_H4SIZE = ZT_DF_H4SIZE;
static_assert(DF_HSIZE <= 65536 && DF_H4SIZE <= 65536, "bucket indices are parked in u16 slots (hash_keys)");
static_assert(DF_HSIZE % 2 == 0, "two u16 heads per word");
constexpr int DF_THREADS = 1024;
// the ring holds [p1 - DF_RING, p1) while sub-chunk [p0, p1) is searched;
// a super-chunk loads DF_HIST bytes of history first (whole sub-chunks)
constexpr int DF_HIST = DF_RING - DF_SUB;     // 28672
// The first DF_HEAD bytes of the next sub-chunk are in the ring while a
// sub-chunk is searched, so matches run on past its end (to the block's);
// they take the ring slots of the window's oldest DF_HEAD - 64 bytes.
#ifndef ZT_DF_HEAD
#define ZT_DF_HEAD 320
#endif
constexpr int DF_HEAD = ZT_DF_HEAD;
static_assert(DF_HEAD == 0 || DF_HEAD >= 258 + 8 + 54, "a head covers a whole match past the sub-chunk end");
constexpr int DF_MAXDIST = DF_HIST - 64 - (DF_HEAD ? DF_HEAD - 64 : 0);  // 28352 (28608 without heads)
// empty head entry: p - kNoHead exceeds DF_MAXDIST for every rel position p
constexpr uint32_t kNoHead = 0x80000000u;

// Preset dictionary of a batch (second argument of classify_dict_kernel and
// match_dict_kernel; launches without a dictionary run classify_kernel and
// match_kernel, which take DeflateParams alone and hold no dictionary code).
// The first workgroup of every stream loads `hist` bytes of history from
// `dict` instead of from the bytes before the stream.  dict holds the usable
// tail of the dictionary (its last DF_MAXDIST bytes at most) right-aligned in
// hist = round_up(tail, DF_SUB) bytes; the floor = hist - tail bytes in front
// are padding: rel positions below the floor are never linked into the
// chains, never probed and never a match source.
struct DictView {
  const uint8_t *dict;
  uint32_t hist;
  uint32_t floor;
};

namespace {

// ================================ 0. classify_kernel ================================
// Blocks that cannot beat a stored block skip the match search and the parse
// (src/RawDeflate.ts:122-153 is the stored form).  Decided
// from the block's bytes alone, one 256-thread workgroup per 32 KiB block:
//  A. order-0 entropy of a 4 KiB sample (1 KiB at each quarter): below
//     CL_ENTROPY bits per byte the literals alone would compress -> search;
//  B. high-entropy blocks are checked for repeats (random data that occurs
//     twice compresses although its bytes look random): the 8-byte keys of
//     every 16th position of the window (up to 28 KiB of history in the same
//     segment + the block) go into an LDS table (position + a 16-bit
//     fingerprint per bucket), every position of the block looks its key up
//     from registers (each thread 128 consecutive positions); a repeat of L
//     bytes gives ~L / 16 hits (the pair's other position, before or after,
//     within a match distance).  CL_HITS hits or more -> search.
//  C. the block's byte histogram (every 3rd byte, from the registers stage B
//     loaded): a block whose order-0 entropy would let an ideal literal coder
//     save more than CL_SAVE over the stored form is searched (a skewed
//     block -- 7.85..7.98 bits -- or compressible bytes outside the sample).
// Everything else is flagged: match / price / DP / parse skip the block and
// block_kernel plans it stored (the smallest form for such bytes: the
// reference's dynamic block of random data is 0.1 % larger).
constexpr float CL_ENTROPY = 7.85f;  // uniform bytes: ~7.955 from a 4096-byte sample
constexpr uint32_t CL_HITS = 8;
constexpr float CL_SAVE = 0.002f;  // C: largest saving an ideal literal coder may forgo
constexpr int CL_STRIDE = 3;       // C: every 3rd byte counted
constexpr uint32_t CL_TABLE = 8192;
constexpr uint32_t CL_EMPTY = 0xFFFFFFFFu;
struct ClassifyShared {
  uint32_t table[CL_TABLE];  // window position << 16 | fingerprint
  uint32_t hist[256];
  float part[4];
  uint32_t hits[4];
  float cnt[4][2];  // stage C: bytes counted, bins used (per wave)
};

// 4 stream bytes at g + off (off >= 0 relative to a possibly unaligned g);
// bytes at or past `end`, and bytes before `begin`, read as 0 (begin: the
// window's first byte where off may lie below it -- the inserts' words start
// at a multiple of 4 at or below a window that starts 1..3 bytes into a halo,
// and nothing in front of the halo belongs to the caller's buffer)
__device__ __forceinline__ uint32_t cl_gword(const uint8_t *g, int64_t off, uint64_t end, int64_t begin = 0) {
  const uint8_t *a = g + off;
  if ((reinterpret_cast<uintptr_t>(a) & 3) == 0 && off >= begin && off + 4 <= (int64_t)end)
    return *reinterpret_cast<const uint32_t *>(a);
  uint32_t v = 0;
  for (int k = 0; k < 4; ++k)
    if (off + k >= begin && off + k < (int64_t)end) v |= (uint32_t)a[k] << (8 * k);
  return v;
}
// 4 bytes at offset wo of the window [dictionary tail dt[0 .. dlen) | stream
// bytes from g + lo on] of a stream's first block (bytes past `end` read as 0)
__device__ __forceinline__ uint32_t cl_dword(const uint8_t *dt, uint32_t dlen, const uint8_t *g, uint64_t lo,
                                             uint64_t end, uint32_t wo) {
  if (wo >= dlen) return cl_gword(g, (int64_t)(lo + (wo - dlen)), end);
  uint32_t v = 0;
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t o = wo + k;
    uint32_t b = 0;
    if (o < dlen)
      b = dt[o];
    else if (lo + (o - dlen) < end)
      b = g[lo + (o - dlen)];
    v |= b << (8 * k);
  }
  return v;
}
// 13-bit bucket and 16-bit fingerprint of an 8-byte key
__device__ __forceinline__ uint32_t cl_hash(uint32_t a, uint32_t b) {
  uint32_t h = a * 0x9E3779B1u ^ b * 0x85EBCA77u;
  h ^= h >> 15;
  return h * 0x2C1B3C6Du;
}

template <bool DICT>
__device__ __forceinline__ void classify_body(const DeflateParams P, const DictView D) {
  __shared__ ClassifyShared sh;
  ClassifyShared *s = &sh;
  const uint32_t t = threadIdx.x, blk = blockIdx.x;
  const uint64_t lo = (uint64_t)blk * DF_BLOCK;
  const uint64_t n = stream_end(P, blk);
  const uint32_t blen = (uint32_t)((n - lo) < DF_BLOCK ? (n - lo) : DF_BLOCK);
  const uint8_t *g = P.base + P.halo;  // stream byte 0
  if (blen < 4096) {  // (small blocks: a search is cheap)
    if (t == 0) P.store[blk] = 0;
    return;
  }
  // A. entropy of the sample (4 words every `stride` bytes)
  s->hist[t] = 0;
  __syncthreads();
  // (four contiguous 1 KiB pieces, a quarter of the block apart: coalesced,
  // 4 KiB of lines per block instead of one line per sampled word)
  const uint32_t pstep = (blen / 4) & ~15u;
  {
    uint32_t v[4];
    const uint64_t a = lo + (uint64_t)(t >> 6) * pstep + (t & 63) * 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = cl_gword(g, (int64_t)(a + 4 * j), n);
#pragma unroll
    for (int j = 0; j < 16; ++j) atomicAdd(&s->hist[(v[j >> 2] >> (8 * (j & 3))) & 0xFF], 1u);
  }
  __syncthreads();
  const float c = (float)s->hist[t];
  float e = c > 0.f ? c * __log2f(c) : 0.f;
  for (int off = 32; off; off >>= 1) e += __shfl_xor(e, off, 64);
  if ((t & 63) == 0) s->part[t >> 6] = e;
  __syncthreads();
  const float h = 12.0f - (s->part[0] + s->part[1] + s->part[2] + s->part[3]) * (1.0f / 4096.0f);
  if (h < CL_ENTROPY) {
    if (t == 0) P.store[blk] = 0;
    return;
  }
  // B. repeats inside the window: history from the block's segment / stream
  const uint64_t f_lo = P.span ? P.span[2 * (uint64_t)blk] : 0;
  const uint64_t seg = ((lo - f_lo) / DF_BLOCK) / P.restart;
  const uint64_t w_lo = f_lo + seg * P.restart * DF_BLOCK;  // segment start (stream coordinates)
  const bool halo_hist = !P.span && seg == 0 && P.halo > 0;  // the first segment may look into the halo
  int64_t h0 = (int64_t)lo - DF_HIST;
  const int64_t floor_ = halo_hist ? -(int64_t)(P.halo < (uint64_t)DF_HIST ? P.halo : (uint64_t)DF_HIST) : (int64_t)w_lo;
  if (h0 < floor_) h0 = floor_;
  // a stream's first block counts its preset dictionary as history: the
  // window is the dictionary's usable tail, then the block
  const bool dfirst = DICT && lo == f_lo;
  const uint32_t dlen = dfirst ? D.hist - D.floor : 0u;
  const uint8_t *dtail = dfirst ? D.dict + D.floor : nullptr;
  const uint32_t wlen = (uint32_t)((int64_t)lo + blen - h0) + dlen;
  for (uint32_t i = t; i < CL_TABLE; i += 256) s->table[i] = CL_EMPTY;
  s->hist[t] = 0;  // (stage A's reads of it are behind the barrier above; B2 counts the whole block)
  // B1. inserts: every 16th position of the window (at most 15 per thread,
  // every load issued before the first is used); 8-byte loads when the
  // stream is 16-byte aligned and the window's reads stay inside it
  constexpr int NI = (DF_HIST + DF_BLOCK) / (16 * 256);
  const bool vecb = (reinterpret_cast<uintptr_t>(g) & 15) == 0 && (h0 & 15) == 0 && lo + DF_BLOCK + 8 <= n;
  const bool vec = vecb && !dfirst;  // (the inserts; the queries below read the block alone: vecb)
  typedef unsigned int cl_u32x2 __attribute__((ext_vector_type(2)));
  typedef unsigned int cl_u32x4 __attribute__((ext_vector_type(4)));
  {
    uint32_t w[NI][3];
    const int64_t a4 = h0 & ~int64_t(3);
    const uint32_t sh = (uint32_t)(h0 - a4);
    if (vec) {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const uint32_t r = 16 * (t + 256 * i);
        const cl_u32x2 v = r + 8 <= wlen ? *reinterpret_cast<const cl_u32x2 *>(g + h0 + r) : cl_u32x2{0, 0};
        w[i][0] = v.x;
        w[i][1] = v.y;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int64_t a = a4 + 16 * (int64_t)(t + 256 * i);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          w[i][j] = dfirst ? cl_dword(dtail, dlen, g, lo, n, 16 * (t + 256 * i) + 4 * j) : cl_gword(g, a + 4 * j, n, h0);
      }
    }
    __syncthreads();  // (the table's EMPTY stores before any insert)
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const uint32_t r = 16 * (t + 256 * i);
      const uint32_t x0 = vec ? w[i][0] : __builtin_amdgcn_alignbyte(w[i][1], w[i][0], sh);
      const uint32_t x1 = vec ? w[i][1] : __builtin_amdgcn_alignbyte(w[i][2], w[i][1], sh);
      const uint32_t hh = cl_hash(x0, x1);
      // (with a dictionary the oldest position of a bucket stays: a block
      // that repeats dictionary bytes a multiple of 16 back inserts the same
      // keys itself, and a query that finds only its own position is no hit)
      if (r + 8 <= wlen) {
        if (dfirst)
          atomicMin(&s->table[hh >> 19], (r << 16) | (hh & 0xFFFFu));
        else
          s->table[hh >> 19] = (r << 16) | (hh & 0xFFFFu);
      }
    }
  }
  __syncthreads();
  // B2. queries: thread t the 128 positions from lo + 128 t (block coordinates k)
  const uint32_t b0 = (uint32_t)((int64_t)lo - h0) + dlen;  // the block in window coordinates
  uint32_t hits = 0;
  const uint32_t k0 = 128 * t;
  if (k0 < blen) {
    uint32_t w[36];
    if (vecb) {
      const cl_u32x4 *v4 = reinterpret_cast<const cl_u32x4 *>(g + lo + k0);
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const cl_u32x4 v = v4[j];
        w[4 * j] = v.x;
        w[4 * j + 1] = v.y;
        w[4 * j + 2] = v.z;
        w[4 * j + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 34; ++j) w[j] = cl_gword(g, (int64_t)(lo + k0 + 4 * j), n);
    }
    // the block's byte histogram over every 3rd byte (stage A saw a 4 KiB
    // sample only; a stride prime to 2 sees every byte lane of 2-, 4- and
    // 8-byte records; all 32 KiB took 0.23 ms per GiB of LDS atomics)
#pragma unroll
    for (int k = 0; k < 128; k += CL_STRIDE)
      if (k0 + (uint32_t)k < blen) atomicAdd(&s->hist[(w[k >> 2] >> (8 * (k & 3))) & 0xFF], 1u);
#pragma unroll
    for (int k = 0; k < 128; ++k) {
      const uint32_t x0 = (k & 3) ? __builtin_amdgcn_alignbyte(w[(k >> 2) + 1], w[k >> 2], k & 3) : w[k >> 2];
      const uint32_t x1 =
          (k & 3) ? __builtin_amdgcn_alignbyte(w[(k >> 2) + 2], w[(k >> 2) + 1], k & 3) : w[(k >> 2) + 1];
      const uint32_t hh = cl_hash(x0, x1);
      const uint32_t ent = s->table[hh >> 19];
      const uint32_t r = b0 + k0 + (uint32_t)k, q = ent >> 16;
      const bool ok = k0 + (uint32_t)k + 8 <= blen && ent != CL_EMPTY && (ent & 0xFFFFu) == (hh & 0xFFFFu) &&
                      q != r && (q < r ? r - q : q - r) <= (uint32_t)DF_MAXDIST;
      hits += ok ? 1u : 0u;
    }
  }
  for (int off = 32; off; off >>= 1) hits += __shfl_xor(hits, off, 64);
  if ((t & 63) == 0) s->hits[t >> 6] = hits;
  __syncthreads();
  // C. the block's order-0 entropy (Miller-Madow: the sample's plug-in
  // estimate + (bins used - 1) / (2 N ln 2), its bias): an ideal literal
  // coder (which no Huffman code beats) + a 32-byte header must not save more
  // than CL_SAVE of the block over the stored form, or the block is searched
  // (uniform bytes: ~8.00 bits per byte, the cut ~7.98)
  const float cb = (float)s->hist[t];
  float eb = cb > 0.f ? cb * __log2f(cb) : 0.f, nb = cb, kb = cb > 0.f ? 1.f : 0.f;
  for (int off = 32; off; off >>= 1) {
    eb += __shfl_xor(eb, off, 64);
    nb += __shfl_xor(nb, off, 64);
    kb += __shfl_xor(kb, off, 64);
  }
  __syncthreads();  // (every hist read done before part[] is rewritten below)
  if ((t & 63) == 0) {
    s->part[t >> 6] = eb;
    s->cnt[t >> 6][0] = nb;
    s->cnt[t >> 6][1] = kb;
  }
  __syncthreads();
  if (t == 0) {
    const float n = s->cnt[0][0] + s->cnt[1][0] + s->cnt[2][0] + s->cnt[3][0];
    const float k = s->cnt[0][1] + s->cnt[1][1] + s->cnt[2][1] + s->cnt[3][1];
    const float hb = __log2f(n) - (s->part[0] + s->part[1] + s->part[2] + s->part[3]) / n +
                     (k - 1.f) / (2.f * n * 0.69314718f);
    const bool flat = hb * (float)blen * 0.125f + 32.f >= (1.0f - CL_SAVE) * (float)blen;
    const bool st = flat && (s->hits[0] + s->hits[1] + s->hits[2] + s->hits[3]) < CL_HITS;
    P.store[blk] = st ? 1 : 0;
    if (st) atomicAdd(P.nstore, 1u);
  }
}

__global__ __launch_bounds__(256) void classify_kernel(DeflateParams P) { classify_body<false>(P, DictView{}); }
__global__ __launch_bounds__(256) void classify_dict_kernel(DeflateParams P, DictView D) {
  classify_body<true>(P, D);
}

// ================================ 1. match_kernel ================================
constexpr uint32_t RING_ENT = DF_RING / 4;
constexpr uint32_t MQ_RING = 128;   // a wave's queue: two pushes of up to 64 between passes (walk_pair_hop_mq)
constexpr uint32_t MQ_SLOTS = 128;  // a wave's walks in flight: two per lane
#ifndef ZT_DF_MQ_FLUSH
#define ZT_DF_MQ_FLUSH 15
#endif
// 2^k - 1: a short queue is measured every 2^k steps all the same (every 4 /
// 8 / 16 steps at level 6: wordsalad 43.1 / 40.1 / 39.7, source text 44.5 /
// 43.1 / 42.0 ms of match per GiB)
constexpr int MQ_FLUSH = ZT_DF_MQ_FLUSH;
struct MatchShared {
  uint32_t ring[DF_RING / 4 + 16];  // data ring + 64-byte mirror of its start
  uint16_t prev[DF_RING];           // relative chain links (0 = none)
  // the chain heads in one of two formats (workgroup-uniform, match_body's
  // fmt16; head_convert changes it in place): the queues exist only beside
  // u16 heads
  union {
    uint32_t head32[DF_HSIZE];      // u32 format: newest position (rel) per hash bucket, kNoHead = none
    struct {
      uint32_t head[DF_HSIZE / 2];  // u16 format: newest position (rel mod 2^16) per hash bucket, two buckets per word
      uint32_t mq[DF_THREADS / 64][MQ_RING];   // per wave: candidates to measure (distance | walk slot << 16), a ring
      uint32_t mr[DF_THREADS / 64][MQ_SLOTS];  // per wave and walk slot: the best candidate's mq_key
    };
  };
  uint32_t head4[DF_H4SIZE];        // newest position (rel) per 4-byte-key bucket
  uint16_t link4[DF_SUB];           // position p of the sub-chunk: distance to the newest earlier
                                    // position of its 4-byte-key bucket (0 = none), at p % DF_SUB
  uint32_t dummy[4];                // exchange / link targets of lanes past the end (branch-free chain_link)
  uint32_t linked;                  // positions below are linked (chain_link -> searching waves)
  uint32_t linked4;                 // positions below have their 4-byte links
  uint32_t work;                    // next super-step of 256 positions to search
  uint32_t late, late2;             // probe sub-chunk: improvements at hop >= adapt_depth / adapt_depth2
  uint32_t nmeas;                   // probe sub-chunk: candidates measured
  int depth;                        // max_chain of the block's later sub-chunks
  int queued;                       // the block's later sub-chunks measure their candidates through the queues
};
static_assert(sizeof(MatchShared) <= 160 * 1024, "MatchShared fits the CU's LDS");
static_assert(offsetof(MatchShared, head32) % 8 == 0, "head_convert moves u32 heads in pairs");
// Workgroup barrier for LDS hand-offs only: waits for this wave's LDS
// operations, not for its global loads (the next sub-chunk's prefetch stays
// in flight) nor its global stores (res[] is read by later kernels only).
// __syncthreads() would drain vmcnt and expose HBM latency at every barrier.
__device__ __forceinline__ void lds_barrier() { __asm__ volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ uint32_t ridx(uint32_t rel) { return rel & (DF_RING - 1); }
// ---- ring storage: every access goes through these ----
// dword w (0 <= w < RING_ENT) of the ring := v (and its mirror copies)
__device__ __forceinline__ void ring_put32(MatchShared *s, uint32_t w, uint32_t v) {
  s->ring[w] = v;
  if (w < 16) s->ring[RING_ENT + w] = v;
}
// byte k (0 <= k < DF_RING) of the ring := v (and its copies)
__device__ __forceinline__ void ring_put8(MatchShared *s, uint32_t k, uint8_t v) {
  uint8_t *rb = reinterpret_cast<uint8_t *>(s->ring);
  rb[k] = v;
  if (k < 64) rb[DF_RING + k] = v;
}
// dwords w and w + 1 of the ring (w < RING_ENT + 15: the mirror covers the wrap)
__device__ __forceinline__ uint2 ring_pair(const MatchShared *s, uint32_t w) {
  return make_uint2(s->ring[w], s->ring[w + 1]);
}
// dwords w .. w + N of the ring (w < RING_ENT, N <= 15: the mirror covers the wrap)
template <int N>
__device__ __forceinline__ void ring_dwords(const MatchShared *s, uint32_t w, uint32_t (&d)[N + 1]) {
#pragma unroll
  for (int k = 0; k <= N; ++k) d[k] = s->ring[w + k];
}
__device__ __forceinline__ uint32_t ld8(const MatchShared *s, uint32_t rel) {
  const uint32_t i = ridx(rel);
  return reinterpret_cast<const uint8_t *>(s->ring)[i];
}
// 4 bytes at any byte offset: an aligned dword pair and a byte align (an
// unaligned ds_read_b32 is legal on gfx950 but measured 25-45 % slower here)
__device__ __forceinline__ uint32_t ld32(const MatchShared *s, uint32_t rel) {
  const uint2 v = ring_pair(s, ridx(rel) >> 2);
  return __builtin_amdgcn_alignbyte(v.y, v.x, rel);  // (v_alignbyte_b32 reads the shift's low 2 bits only)
}
// chain key at p: the first klen bytes (kmask: bytes 0-3, kmask2: bytes 4-7)
struct Key {
  uint32_t kmask, kmask2;
};

// bytes [rel0, rel0 + len) of the super-chunk into the ring (len <= DF_SUB, rel0 % DF_SUB == 0)
__device__ void load_sub(MatchShared *s, const uint8_t *g, uint32_t rel0, uint32_t len) {
  const uint32_t t = threadIdx.x;
  const uint32_t k0 = ridx(rel0);  // multiple of DF_SUB
  if (len == DF_SUB && (reinterpret_cast<uintptr_t>(g) & 3) == 0) {
    ring_put32(s, (k0 >> 2) + t, reinterpret_cast<const uint32_t *>(g)[t]);
    return;
  }
  // (the rare path of a short or unaligned sub-chunk: its start index is opaque
  // to the compiler, which would otherwise keep g + t in two registers across
  // the whole sub-chunk loop of match_body)
  uint32_t i0 = t;
  __asm__ volatile("" : "+v"(i0));
  for (uint32_t i = i0; i < len; i += DF_THREADS) ring_put8(s, k0 + i, g[i]);
}

// chain links for positions [lo, hi) (rel coords), by one wave, in position
// order: per step of 64 positions one LDS exchange head[h] <-> p.  The LDS
// applies the conflicting lanes of one exchange in lane order (checked on
// gfx950 by tools/micro/lds_xchg_order.hip), so each lane gets the newest
// earlier position of its bucket -- in its step or before -- and the head
// ends at the step's last one.  Exchanges of later steps are issued without
// waiting for earlier results (the wave's LDS operations stay in order); the
// progress is published for the searching waves (match_kernel).  T = 0: the
// 8-byte-key chains (head or head32 -> prev, s->linked; F16: the heads'
// format); T = 1, by a second wave at the same time: the 4-byte-key table
// (head4 -> link4, s->linked4).
// Hashes of the keys at positions [lo, hi), by all threads of the workgroup,
// parked in the slots their links will fill: prev[ridx(p)] (the ring slot of
// p held a position 32 KiB back, out of every walk's reach) and
// link4[p % DF_SUB] (the previous sub-chunk's, whose searches are done).  The
// serial link waves then only read them (chain_link).
// Four consecutive positions per thread: three aligned dword reads (lanes on
// consecutive words: no bank conflicts) give all four 8-byte keys by byte
// aligns, and a full quad's hashes go out as one 8-byte store per table
// (one position per thread took two unaligned reads -- two dwords each -- and
// two 2-byte stores per position).  Slots outside [lo, hi) keep their values:
// below lo are links already made, and link4's slots past hi are this
// sub-chunk's first positions.
__device__ __forceinline__ void hash_keys(MatchShared *s, uint32_t lo, uint32_t hi, Key key) {
  for (uint32_t p4 = (lo & ~3u) + 4 * threadIdx.x; p4 < hi; p4 += 4 * DF_THREADS) {
    const uint32_t w = ridx(p4) >> 2;  // (the mirror past the ring's end holds w + 1, w + 2 at the wrap)
    const uint2 d01 = ring_pair(s, w), d12 = ring_pair(s, w + 1);
    const uint32_t d0 = d01.x, d1 = d01.y, d2 = d12.y;
    uint32_t hk[4], h4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t x0 = k ? __builtin_amdgcn_alignbyte(d1, d0, k) : d0;
      const uint32_t x1 = k ? __builtin_amdgcn_alignbyte(d2, d1, k) : d1;
      const uint32_t v = (x0 & key.kmask) ^ ((x1 & key.kmask2) * 0x2545F491u);
      hk[k] = __umulhi(v * 0x9E3779B1u, DF_HSIZE);
      h4[k] = __umulhi(x0 * 0x9E3779B1u, DF_H4SIZE);
    }
    if (p4 >= lo && p4 + 4 <= hi) {
      *reinterpret_cast<uint2 *>(&s->prev[ridx(p4)]) = make_uint2(hk[0] | hk[1] << 16, hk[2] | hk[3] << 16);
      *reinterpret_cast<uint2 *>(&s->link4[p4 & (DF_SUB - 1)]) = make_uint2(h4[0] | h4[1] << 16, h4[2] | h4[3] << 16);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (p4 + k >= lo && p4 + k < hi) {
          s->prev[ridx(p4 + k)] = (uint16_t)hk[k];
          s->link4[(p4 + k) & (DF_SUB - 1)] = (uint16_t)h4[k];
        }
      }
    }
  }
}

#ifndef ZT_CL_U
#define ZT_CL_U 8
#endif
constexpr int CL_U = ZT_CL_U;  // steps per group: hashes, then exchanges, then links
template <int T, bool F16 = false>
__device__ void chain_link(MatchShared *s, uint32_t lo, uint32_t hi, Key key) {
  const int lane = threadIdx.x & 63;
  const uint32_t nsteps = (hi - lo + 63) / 64;
  uint32_t hq[CL_U];
  // the keys' hashes were computed by every thread beforehand (hash_keys)
  // and parked in the slots the links are about to fill
  auto hashes = [&](uint32_t sb, uint32_t (&h)[CL_U]) {
#pragma unroll
    for (int j = 0; j < CL_U; ++j) {
      const uint32_t p = lo + (sb + j) * 64 + lane;
      const uint32_t pc = p < hi ? p : lo;  // (lanes past hi: any bucket, they exchange with a dummy)
      h[j] = T == 0 ? (uint32_t)s->prev[ridx(pc)] : (uint32_t)s->link4[pc & (DF_SUB - 1)];
    }
  };
  hashes(0, hq);
  for (uint32_t sb = 0; sb < nsteps; sb += CL_U) {
    // branch-free: lanes past hi exchange with / link into a dummy word, so
    // the compiler keeps every load and exchange of the group in flight
    uint32_t old[CL_U];
    if (T == 0 && F16) {
      // u16 heads: a masked-OR exchange of one half-word (ds_mskor_rtn_b32
      // applies a wave's conflicting lanes in lane order, as the exchange
      // does: tools/micro/lds_mskor_order.hip); the waits come after all CL_U
      // are issued (the compiler does not see inline-asm LDS operations)
      uint32_t sh[CL_U];
#pragma unroll
      for (int j = 0; j < CL_U; ++j) {
        const uint32_t p = lo + (sb + j) * 64 + lane;
        uint32_t *hp = p < hi ? &s->head[hq[j] >> 1] : &s->dummy[T];
        sh[j] = (hq[j] & 1) * 16;
        const uint32_t a = (uint32_t)(uintptr_t)hp, clr = 0xFFFFu << sh[j], set = (p & 0xFFFFu) << sh[j];
        __asm__ volatile("ds_mskor_rtn_b32 %0, %1, %2, %3" : "=v"(old[j]) : "v"(a), "v"(clr), "v"(set) : "memory");
      }
      // (the next group's hashes load while the exchanges are in flight; the
      // wait below covers both)
      hashes(sb + CL_U, hq);
      static_assert(CL_U == 8, "the wait below names 8 results");
      __asm__ volatile("s_waitcnt lgkmcnt(0)"
                       : "+v"(old[0]), "+v"(old[1]), "+v"(old[2]), "+v"(old[3]), "+v"(old[4]), "+v"(old[5]),
                         "+v"(old[6]), "+v"(old[7])::"memory");
#pragma unroll
      for (int j = 0; j < CL_U; ++j) {
        const uint32_t p = lo + (sb + j) * 64 + lane;
        // (the distance modulo 2^16 is exact: stale heads are re-aged by head_sweep)
        old[j] = p - ((p - (old[j] >> sh[j])) & 0xFFFFu);
      }
    } else {
#pragma unroll
      for (int j = 0; j < CL_U; ++j) {
        const uint32_t p = lo + (sb + j) * 64 + lane;
        uint32_t *hp = p < hi ? (T == 0 ? &s->head32[hq[j]] : &s->head4[hq[j]]) : &s->dummy[T];
        old[j] = atomicExch(hp, p);
      }
      hashes(sb + CL_U, hq);
    }
#pragma unroll
    for (int j = 0; j < CL_U; ++j) {
      const uint32_t p = lo + (sb + j) * 64 + lane;
      const uint32_t d = p - old[j];
      uint16_t *pp = p < hi ? (T == 0 ? &s->prev[ridx(p)] : &s->link4[p & (DF_SUB - 1)])
                            : reinterpret_cast<uint16_t *>(&s->dummy[2 + T]);
      *pp = (uint16_t)(d <= (uint32_t)DF_MAXDIST ? d : 0u);
    }
    const uint32_t done = lo + (sb + CL_U) * 64;
    if (lane == 0)
      __hip_atomic_store(T == 0 ? &s->linked : &s->linked4, done < hi ? done : hi, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// The same links for ng whole groups of CL_U steps from lo on: every position
// of a whole group is in range, so no lane needs a dummy target or a clamped
// address -- positions advance by adds, and the slot index is masked for the
// wrap only (lo is any position: a group may straddle the ring's end).  The
// progress word goes out as a plain LDS store behind the group's link stores:
// the LDS applies one wave's operations in issue order (the exchanges above
// rely on it; stores and a flag store after them: tools/micro/
// lds_publish_order.hip), so no wait drains the link stores and the next
// group's hash reads before the next exchanges issue.  The store is inline
// assembly with a memory clobber: the compiler neither moves it nor puts a
// wait in front of it.  The hash reads run one group ahead and
// past the last group read slots that are not used (in bounds: the index is
// masked).
template <int T, bool F16>
__device__ __forceinline__ void chain_link_groups(MatchShared *s, uint32_t lo, uint32_t ng) {
  const uint32_t lane = threadIdx.x & 63;
  constexpr uint32_t G = CL_U * 64;
  auto slot = [&](uint32_t q) -> uint16_t * { return T == 0 ? &s->prev[ridx(q)] : &s->link4[q & (DF_SUB - 1)]; };
  uint32_t p = lo + lane;  // this lane's position in the group's first step
  uint32_t hq[CL_U];
#pragma unroll
  for (int j = 0; j < CL_U; ++j) hq[j] = *slot(p + 64 * j);
  // (the first hashes are waited for here, once per call: with loads pending
  // at the loop's entry the compiler's waits at its head, which must hold for
  // the entry and the back edge alike, would count the link stores of the
  // group before as done as well)
  static_assert(CL_U == 8, "the statement below names 8 hashes");
  __asm__ volatile("" : "+v"(hq[0]), "+v"(hq[1]), "+v"(hq[2]), "+v"(hq[3]), "+v"(hq[4]), "+v"(hq[5]), "+v"(hq[6]), "+v"(hq[7]));
  for (uint32_t g = 0; g < ng; ++g, p += G) {
    uint32_t d[CL_U];  // the exchanged heads, then the distances to them
    if (T == 0 && F16) {
      uint32_t sh[CL_U];
#pragma unroll
      for (int j = 0; j < CL_U; ++j) {
        const uint32_t q = p + 64 * j;
        sh[j] = (hq[j] & 1) * 16;
        const uint32_t a = (uint32_t)(uintptr_t)&s->head[hq[j] >> 1], clr = 0xFFFFu << sh[j], set = (q & 0xFFFFu) << sh[j];
        __asm__ volatile("ds_mskor_rtn_b32 %0, %1, %2, %3" : "=v"(d[j]) : "v"(a), "v"(clr), "v"(set) : "memory");
      }
#pragma unroll
      for (int j = 0; j < CL_U; ++j) hq[j] = *slot(p + G + 64 * j);
      // (the wait covers the hashes too, and names them: the compiler's own
      // counted waits for them at the next group's exchanges, which it cannot
      // see, would each wait for one more of this group's link stores)
      __asm__ volatile("s_waitcnt lgkmcnt(0)"
                       : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]), "+v"(d[4]), "+v"(d[5]), "+v"(d[6]),
                         "+v"(d[7]), "+v"(hq[0]), "+v"(hq[1]), "+v"(hq[2]), "+v"(hq[3]), "+v"(hq[4]), "+v"(hq[5]),
                         "+v"(hq[6]), "+v"(hq[7])::"memory");
#pragma unroll
      for (int j = 0; j < CL_U; ++j) d[j] = (p + 64 * j - (d[j] >> sh[j])) & 0xFFFFu;  // (exact: head_sweep)
    } else {
#pragma unroll
      for (int j = 0; j < CL_U; ++j) d[j] = atomicExch(T == 0 ? &s->head32[hq[j]] : &s->head4[hq[j]], p + 64 * j);
#pragma unroll
      for (int j = 0; j < CL_U; ++j) hq[j] = *slot(p + G + 64 * j);
#pragma unroll
      for (int j = 0; j < CL_U; ++j) d[j] = p + 64 * j - d[j];
    }
#pragma unroll
    for (int j = 0; j < CL_U; ++j) *slot(p + 64 * j) = (uint16_t)(d[j] <= (uint32_t)DF_MAXDIST ? d[j] : 0u);
    // (a store the compiler does not count only makes its counted waits
    // stronger; it has no result to wait for)
    if (lane == 0) {
      const uint32_t a = (uint32_t)(uintptr_t)(T == 0 ? &s->linked : &s->linked4), done = p + G;  // (lane 0: p = lo + g * G)
      __asm__ volatile("ds_write_b32 %0, %1" ::"v"(a), "v"(done) : "memory");
    }
  }
}

// chain_link, whole groups first and the ragged rest as before (lean = false,
// ZT_DF_LINK=0: all of it as before)
template <int T, bool F16 = false>
__device__ __forceinline__ void link_range(MatchShared *s, uint32_t lo, uint32_t hi, Key key, bool lean) {
  if (lean) {
    const uint32_t ng = (hi - lo) / (CL_U * 64);
    if (ng) chain_link_groups<T, F16>(s, lo, ng);
    lo += ng * (CL_U * 64);
    if (lo == hi) return;
  }
  chain_link<T, F16>(s, lo, hi, key);
}

// u16 heads hold rel positions modulo 2^16: every HEAD_SWEEP sub-chunks, at
// rel position S (before that sub-chunk is linked), a head that is out of
// reach (age > DF_MAXDIST, and not one of the <= DF_HEAD positions linked
// ahead of S) is re-aged to S - 32768: until the next sweep it reads as
// 32768..61440 back -- never a link -- and a head in reach stays below 2^16
// back until then, so every link the exchange computes is the true distance.
#ifndef ZT_DF_HEAD_SWEEP
#define ZT_DF_HEAD_SWEEP 4
#endif
constexpr uint32_t HEAD_SWEEP = ZT_DF_HEAD_SWEEP;
static_assert(DF_MAXDIST + (HEAD_SWEEP + 1) * DF_SUB + DF_HEAD < 65536 - 1024, "ages stay below 2^16");
__device__ __forceinline__ void head_sweep(MatchShared *s, uint32_t S) {
  const uint32_t stale = (S - 32768u) & 0xFFFFu;
  for (uint32_t i = threadIdx.x; i < DF_HSIZE / 2; i += DF_THREADS) {
    const uint32_t w = s->head[i];
    uint32_t r = w;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint32_t age = (S - (w >> (16 * k))) & 0xFFFFu;
      if (age > (uint32_t)DF_MAXDIST && age < 65536u - 1024u) r = (r & ~(0xFFFFu << (16 * k))) | (stale << (16 * k));
    }
    if (r != w) s->head[i] = r;
  }
}

// The workgroup's chain heads change their format in place, at rel position
// S (a sub-chunk start, before that sub-chunk is linked; all threads, between
// two barriers of match_body).  Every bucket gives the same link afterwards
// for every later position as without the change:
// u16 -> u32: a head in reach of S (or one of the <= DF_HEAD positions linked
// ahead of S, as in head_sweep) becomes its exact rel position, every other
// one kNoHead;
// u32 -> u16: a head in reach or ahead keeps its low half, every other one
// becomes S - 32768 -- the state a head_sweep at S leaves, so the sweep
// schedule's bound holds from here as from a sweep.
// The two arrays overlap: every thread reads its buckets, a barrier, then it
// writes (the caller's next barrier comes before the link waves read them).
__device__ __forceinline__ uint32_t head_to32(uint32_t v, uint32_t S) {
  const uint32_t age = (S - v) & 0xFFFFu;
  return age <= (uint32_t)DF_MAXDIST ? S - age : age >= 65536u - 1024u ? S + (65536u - age) : kNoHead;
}
__device__ __forceinline__ uint32_t head_to16(uint32_t r, uint32_t S) {
  return (S - r <= (uint32_t)DF_MAXDIST || r - S <= 1024u) ? (r & 0xFFFFu) : ((S - 32768u) & 0xFFFFu);
}
template <bool TO16>
__device__ __forceinline__ void head_convert(MatchShared *s, uint32_t S) {
  constexpr uint32_t NW = (DF_HSIZE / 2 + DF_THREADS - 1) / DF_THREADS;  // bucket pairs per thread
  uint32_t a[NW], b[NW];
  // (opaque to the compiler: it would otherwise compute every thread's 12
  // addresses ahead of the sub-chunk loop and spill them around the search)
  uint32_t tid = threadIdx.x;
  __asm__ volatile("" : "+v"(tid));
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k) {
    const uint32_t i = tid + k * DF_THREADS;
    a[k] = b[k] = 0;
    if (i < DF_HSIZE / 2) {
      if (TO16) {
        const uint2 v = *reinterpret_cast<const uint2 *>(&s->head32[2 * i]);
        a[k] = v.x;
        b[k] = v.y;
      } else {
        const uint32_t w = s->head[i];
        a[k] = w & 0xFFFFu;
        b[k] = w >> 16;
      }
    }
  }
  lds_barrier();
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k) {
    const uint32_t i = tid + k * DF_THREADS;
    if (i < DF_HSIZE / 2) {
      if (TO16)
        s->head[i] = head_to16(a[k], S) | head_to16(b[k], S) << 16;
      else
        *reinterpret_cast<uint2 *>(&s->head32[2 * i]) = make_uint2(head_to32(a[k], S), head_to32(b[k], S));
    }
  }
}

// 4 bytes at byte x of a register window (x a compile-time constant after unrolling)
template <int X>
__device__ __forceinline__ uint32_t win32(const uint32_t (&w)[9]) {
  return (X & 3) ? __builtin_amdgcn_alignbyte(w[(X >> 2) + 1], w[X >> 2], X & 3) : w[X >> 2];
}

constexpr int DF_NEAR = 16;  // near distances probed from registers

// matches shorter than the chain key at distances 1..probe, from a register
// window of bytes [pb - 16, pb + 16): longest wins, ties to the nearest
template <int K, int D>
__device__ __forceinline__ void near_probe(const uint32_t (&w)[9], uint32_t cur0, uint32_t cur1, uint32_t p,
                                           uint32_t max_len, int probe, uint32_t &best_len, uint32_t &best_dist) {
  if constexpr (D <= DF_NEAR) {
    if (D <= probe && (uint32_t)D <= p) {
      const uint32_t m0 = win32<16 + K - D>(w) ^ cur0;
      if ((m0 & 0xFFFFFFu) == 0) {
        uint32_t len;
        if (m0) {
          len = 3;
        } else {
          const uint32_t m1 = win32<20 + K - D>(w) ^ cur1;
          len = m1 ? 4 + ((uint32_t)(__ffs(m1) - 1) >> 3) : 8;
        }
        if (len > max_len) len = max_len;
        if (len > best_len) {
          best_len = len;
          best_dist = D;
        }
      }
    }
    near_probe<K, D + 1>(w, cur0, cur1, p, max_len, probe, best_len, best_dist);
  }
}

// Branch-free prefilter of the near probes of position pb + K: the minimum
// over distances 1..DF_NEAR of (3 bytes at p - D) XOR (3 bytes at p) is zero
// iff some distance has a 3-byte match (out-of-range distances only give
// false positives; near_probe re-checks).  One alignbyte + bitop3 + min per
// distance instead of a compare-and-branch per distance.
template <int K, int D>
__device__ __forceinline__ uint32_t near_any(const uint32_t (&w)[9], uint32_t cur0, uint32_t m) {
  if constexpr (D <= DF_NEAR) {
    const uint32_t x = (win32<16 + K - D>(w) ^ cur0) & 0xFFFFFFu;
    return near_any<K, D + 1>(w, cur0, m < x ? m : x);
  } else {
    return m;
  }
}

// One position's hash-chain walk (newest candidate first).  Two walks are
// interleaved per thread so that their dependent LDS loads overlap.
struct Walk {
  uint32_t p, q, link, max_len, best_len, best_dist, o, pw, omask, cur, cur2, cur3, cur4;
  uint32_t cl;  // carried match length (kept unless the walk finds one at least as long, nearer)
  int max_hops;  // (hops taken = the pair loop's step count while the walk is active)
  uint32_t late;  // ROLE_PROBE: improvements found at hop >= P.adapt_depth (low half) / adapt_depth2 (high half)
  uint32_t nmeas; // ROLE_PROBE: candidates measured
  bool active;
};

// What a sub-chunk's walks do besides finding matches, fixed at compile time
// (nothing is decided per hop).  The block's first sub-chunk is the probe: it
// measures each candidate at once, walks max_chain hops and counts (late
// improvements for the block's depth, measurements for the block's way of
// measuring).  The others carry no counts and measure at once (plain) or
// through the wave's queue (queued), as the probe's counts say.
enum Role { ROLE_PROBE, ROLE_PLAIN, ROLE_QUEUED };

// n words at byte rel of the ring, unaligned (the 64-byte mirror past the
// ring's end keeps up to 15 words contiguous): n + 1 dword loads, no wrap math
template <int N>
__device__ __forceinline__ void ld_run(const MatchShared *s, uint32_t rel, uint32_t (&o)[N]) {
  const uint32_t w = ridx(rel) >> 2, sh = rel;  // (v_alignbyte_b32 reads the shift's low 2 bits only)
  uint32_t d[N + 1];
  ring_dwords<N>(s, w, d);
#pragma unroll
  for (int k = 0; k < N; ++k) o[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
}

// start the walk of position p (carry: the previous position's match); cur..cur4
// are bytes 0..15 of p
__device__ __forceinline__ void walk_init(Walk &w, const MatchShared *s, const DeflateParams &P, uint32_t p, uint32_t p1,
                                          uint32_t cur, uint32_t cur2, uint32_t cur3, uint32_t cur4,
                                          uint32_t carry_len, uint32_t carry_dist, uint32_t link, int mc) {
  w.p = p;
  w.q = p;
  w.cur = cur;
  w.cur2 = cur2;
  w.cur3 = cur3;
  w.cur4 = cur4;
  w.max_len = p < p1 ? ((p1 - p) < 258 ? (p1 - p) : 258) : 0;
  w.best_len = 0;
  w.best_dist = 0;
  if (carry_len > 3 && w.max_len >= 3) {
    w.best_len = carry_len - 1 < w.max_len ? carry_len - 1 : w.max_len;
    w.best_dist = carry_dist;
  }
  w.max_hops = (int)w.best_len >= P.good ? (mc >> 2) : mc;
  w.active = w.max_len >= (uint32_t)P.klen && (int)w.best_len < P.skip_len;
  w.cl = w.best_len;
  // one word per hop filters the candidates: the word ending at best_len (a
  // candidate can only win if it matches there), or before any match the
  // first bytes of the key (the chains' hash buckets also hold collisions)
  w.o = w.best_len >= 4 ? w.best_len - 3 : 0;
  w.omask = w.best_len >= 4 || P.klen >= 4 ? 0xFFFFFFFFu : 0xFFFFFFu;
  w.pw = cur;
  w.link = 0;
  if (w.active) {
    if (w.best_len >= 4) w.pw = ld32(s, p + w.o);
    w.link = link;  // prev[ridx(p)], read by search_quad with its three neighbours
    w.active = w.link != 0;
  }
}

// equal leading bytes (0..16) of four XORed words: the first differing bit
// of each word (v_ffbl: ~0 for none), offset by the word's place with
// unsigned saturation (none stays ~0; the last word's by a min with 32, so
// that no constant needs a register), the least of them -- 11 VALU (round
// 4's per-word selects: 17, and the measurement is the walk's VALU-heaviest
// part: match 22.4 -> 20.4 ms per GiB, streams identical); inline asm because
// the compiler rewrites ffs of a possibly-zero word into compares and selects
__device__ __forceinline__ uint32_t ffbl_raw(uint32_t x) {
  uint32_t r;
  asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}
template <uint32_t B>
__device__ __forceinline__ uint32_t add_sat(uint32_t a) {
  uint32_t r;
  static_assert(B <= 64, "an inline constant (VOP3 takes no literal here)");
  asm("v_add_u32_e64 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "i"(B));
  return r;
}
__device__ __forceinline__ uint32_t min3_u32(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ uint32_t eq_len16(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
  const uint32_t m = min3_u32(ffbl_raw(x0), add_sat<32>(ffbl_raw(x1)), add_sat<64>(ffbl_raw(x2)));
  const uint32_t l3 = min(ffbl_raw(x3), 32u) + 96u;  // (<= 128: all 16 bytes equal)
  return min(m, l3) >> 3;
}

// a candidate q that passed the one-word filter: its length from byte 0
// (the filter checked at most 4 bytes) and keep the longest
template <Role R>
__device__ __forceinline__ void walk_extend(Walk &w, const MatchShared *s, const DeflateParams &P, uint32_t q,
                                            [[maybe_unused]] uint32_t late) {
#ifdef ZT_DF_COUNT
  atomicAdd(&g_df_count[2], 1ull);
  // (wave-level executions of the measurement: its first active lane counts)
  if ((int)(threadIdx.x & 63) == __ffsll((unsigned long long)__ballot(1)) - 1) atomicAdd(&g_df_count[3], 1ull);
#endif
  // the first 16 bytes: q's words in one run of loads, p's from registers;
  // lengths branch-free, so that every load of the run is in flight at once
  uint32_t qw[4];
  ld_run<4>(s, q, qw);
  uint32_t len = eq_len16(qw[0] ^ w.cur, qw[1] ^ w.cur2, qw[2] ^ w.cur3, qw[3] ^ w.cur4);
  // all 16 matched: 16 more bytes per round until a mismatch (or max_len)
  bool more = len == 16;
  while (more && len < w.max_len) {
    uint32_t qx[4], px[4];
    ld_run<4>(s, q + len, qx);
    ld_run<4>(s, w.p + len, px);
    const uint32_t l = eq_len16(qx[0] ^ px[0], qx[1] ^ px[1], qx[2] ^ px[2], qx[3] ^ px[3]);
    len += l;
    more = l == 16;
  }
  if (len > w.max_len) len = w.max_len;
  // branch-free update (selects instead of nested exec-mask branches: the
  // pass runs with a few lanes of the wave, and every branch of the nest is
  // taken by one of them: match 21.0 -> 20.3 ms per GiB, streams identical)
  const bool upd = len >= 3 && len > w.best_len;
#ifdef ZT_DF_COUNT
  atomicAdd(&g_df_count[upd ? 4 : 6], 1ull);
  if (len < 8) atomicAdd(&g_df_count[5], 1ull);
#endif
  const bool stop = upd && ((int)len >= P.nice_len || len >= w.max_len);
  const bool newo = upd && !stop && len >= 4;
  if constexpr (R == ROLE_PROBE) {
    w.late += upd ? late : 0u;
    w.nmeas += 1;
  }
  w.best_len = upd ? len : w.best_len;
  w.best_dist = upd ? w.p - q : w.best_dist;
  w.active = w.active && !stop;
  w.o = newo ? len - 3 : w.o;
  w.omask = newo ? 0xFFFFFFFFu : w.omask;
  const uint32_t npw = ld32(s, w.p + w.o);
  w.pw = newo ? npw : w.pw;
}



// one hop of two walks: every LDS load of both hops is issued before any is
// used (the walks are latency-bound pointer chases), then the checks.  Per
// hop two loads: the link and the filter word.
// `step`: the pair loop's count of steps before this one (wave-uniform): an
// active walk has taken exactly that many hops.  Inactive walks keep
// stepping through stale links: their loads stay inside the ring and are
// never used.
template <Role R>
__device__ __forceinline__ void walk_pair_step(Walk &a, Walk &b, const MatchShared *s, const DeflateParams &P,
                                               int step) {
  const uint32_t qa = a.q - a.link;
  const uint32_t qb = b.q - b.link;
  const bool ha = a.active && a.p - qa <= (uint32_t)DF_MAXDIST;
  const bool hb = b.active && b.p - qb <= (uint32_t)DF_MAXDIST;
  const uint32_t la = s->prev[ridx(qa)], lb = s->prev[ridx(qb)];
  const uint32_t oa = ld32(s, qa + a.o), ob = ld32(s, qb + b.o);
  a.q = qa;
  b.q = qb;
#ifdef ZT_DF_COUNT
  if ((threadIdx.x & 63) == 0) atomicAdd(&g_df_count[0], 1ull);
  atomicAdd(&g_df_count[1], (unsigned long long)(ha ? 1 : 0) + (hb ? 1 : 0));
#endif
  // (& not &&: a short-circuit lets the compiler sink a filter read into a
  // branch, behind the other walk's wait)
  const bool ca = ha & (((oa ^ a.pw) & a.omask) == 0);
  const bool cb = hb & (((ob ^ b.pw) & b.omask) == 0);
  a.link = la;
  b.link = lb;
  a.active = ha && la != 0 && step + 1 < a.max_hops;
  b.active = hb && lb != 0 && step + 1 < b.max_hops;
  uint32_t late = 0;
  if constexpr (R == ROLE_PROBE)
    late = (P.adapt_depth && step >= P.adapt_depth ? 1u : 0u) |
           (P.adapt_depth2 && step >= P.adapt_depth2 ? 0x10000u : 0u);
  if (ca) walk_extend<R>(a, s, P, qa, late);
  if (cb) walk_extend<R>(b, s, P, qb, late);
}

// ---- ROLE_QUEUED: candidate measurement through a per-wave queue ----
// Measured at once, the wave runs the measurement whenever any of its 128
// walks has a candidate: on text 1.5 passes per pair step with 4.7 lanes
// each, about as much time as the hops themselves.  Here a hop's candidate
// (it passed the filter) is appended to the wave's ring instead.  Whenever 64
// are queued, one pass measures 64 with every lane (p's bytes from the ring)
// and keeps the best per walk in the walk's result slot by an LDS atomicMax
// on mq_key: the longest, then the nearest -- the walk's own order (newest
// first, the first of equal length kept).  The walks then read their slots
// back and tighten their filters; until then a walk filters with an older
// best, which only lets through more candidates (measured, and never longer
// than the best).  Lengths enter the key clamped at nice_len: the walk at
// once stops at the first such candidate, and the nearest of them is that
// one; its owner measures its exact length again (mq_poll).  The ring is
// FIFO, so a slot always holds the best of a prefix of its walk's candidates.
// The streams are the ones of measuring at once.
struct MqState {
  uint32_t head, tail;  // wave-uniform: entries [head, tail) of the ring are queued
  uint32_t pbase;       // position of lane 0's first walk of the pair (slot 0)
  uint32_t pml;         // matches end here (wave-uniform)
  bool ready;           // a pass has run since the walks last read their slots
};
__device__ __forceinline__ uint32_t mq_key(uint32_t len, uint32_t dist) { return (len << 15) | (0x7FFFu - dist); }
static_assert(DF_MAXDIST < 0x7FFF, "a distance fits the key's low 15 bits and the ring entry's low 16");

// walk `slot` of each lane with c set queues its candidate at distance dist
__device__ __forceinline__ void mq_push(MatchShared *s, MqState &m, bool c, uint32_t dist, uint32_t slot) {
  const uint64_t b = __ballot(c);
  if (b) {
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (c) s->mq[threadIdx.x >> 6][(m.tail + below) & (MQ_RING - 1)] = dist | (slot << 16);
#ifdef ZT_DF_COUNT
    if (c) atomicAdd(&g_df_count[7], 1ull);
#endif
    m.tail += (uint32_t)__popcll(b);
  }
}

// equal leading bytes of q.. and p.., 16 per round, at most max_len
__device__ __forceinline__ uint32_t mq_measure(const MatchShared *s, uint32_t q, uint32_t p, uint32_t max_len) {
  uint32_t len = 0;
  bool more = true;
  while (more && len < max_len) {
    uint32_t qx[4], px[4];
    ld_run<4>(s, q + len, qx);
    ld_run<4>(s, p + len, px);
    const uint32_t l = eq_len16(qx[0] ^ px[0], qx[1] ^ px[1], qx[2] ^ px[2], qx[3] ^ px[3]);
    len += l;
    more = l == 16;
  }
  return len < max_len ? len : max_len;
}

// one pass: the next min(64, queued) candidates, one per lane
__device__ __forceinline__ void mq_process(MatchShared *s, const DeflateParams &P, MqState &m) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t n = (m.tail - m.head) < 64u ? (m.tail - m.head) : 64u;
  __builtin_amdgcn_wave_barrier();  // (the pushes are in the ring: the wave's LDS operations stay in order)
#ifdef ZT_DF_COUNT
  if (lane == 0) atomicAdd(&g_df_count[3], 1ull);
#endif
  if (lane < n) {
#ifdef ZT_DF_COUNT
    atomicAdd(&g_df_count[2], 1ull);
#endif
    const uint32_t e = s->mq[wv][(m.head + lane) & (MQ_RING - 1)];
    const uint32_t dist = e & 0xFFFFu, slot = e >> 16;
    // (slot 2 * l is the first walk of lane l's pair, 2 * l + 1 the second, two positions on)
    const uint32_t p = m.pbase + 4 * (slot >> 1) + 2 * (slot & 1);
    const uint32_t ml = p < m.pml ? ((m.pml - p) < 258u ? (m.pml - p) : 258u) : 0u;
    const uint32_t len = mq_measure(s, p - dist, p, ml);
    const uint32_t lk = len < (uint32_t)P.nice_len ? len : (uint32_t)P.nice_len;
    if (len >= 3) atomicMax(&s->mr[wv][slot & (MQ_SLOTS - 1)], mq_key(lk, dist));
  }
  __builtin_amdgcn_wave_barrier();
  m.head += n;
  m.ready = true;
}

// walk_pair_step with the candidates queued instead of measured
__device__ __forceinline__ void walk_pair_hop_mq(Walk &a, Walk &b, MatchShared *s, const DeflateParams &P, int step,
                                                 MqState &m) {
  const uint32_t qa = a.q - a.link;
  const uint32_t qb = b.q - b.link;
  const bool ha = a.active && a.p - qa <= (uint32_t)DF_MAXDIST;
  const bool hb = b.active && b.p - qb <= (uint32_t)DF_MAXDIST;
  const uint32_t la = s->prev[ridx(qa)], lb = s->prev[ridx(qb)];
  const uint32_t oa = ld32(s, qa + a.o), ob = ld32(s, qb + b.o);
  a.q = qa;
  b.q = qb;
#ifdef ZT_DF_COUNT
  if ((threadIdx.x & 63) == 0) atomicAdd(&g_df_count[0], 1ull);
  atomicAdd(&g_df_count[1], (unsigned long long)(ha ? 1 : 0) + (hb ? 1 : 0));
#endif
  const bool ca = ha & (((oa ^ a.pw) & a.omask) == 0);
  const bool cb = hb & (((ob ^ b.pw) & b.omask) == 0);
  a.link = la;
  b.link = lb;
  a.active = ha && la != 0 && step + 1 < a.max_hops;
  b.active = hb && lb != 0 && step + 1 < b.max_hops;
  // (a pass after either push whenever 64 are queued: fewer than 64 stay, so
  // a push of at most 64 never overruns the ring of 128)
  const uint32_t lane = threadIdx.x & 63;
  mq_push(s, m, ca, a.p - qa, 2 * lane);
  if (m.tail - m.head >= 64u) mq_process(s, P, m);
  mq_push(s, m, cb, b.p - qb, 2 * lane + 1);
  if (m.tail - m.head >= 64u) mq_process(s, P, m);
}

// the walk reads its result slot back (branch-free but for the exact length
// of a match that reached nice_len, as the measurement's own update)
__device__ __forceinline__ void mq_poll(Walk &w, const MatchShared *s, const DeflateParams &P, uint32_t slot) {
  const uint32_t k = s->mr[threadIdx.x >> 6][slot];
  uint32_t len = k >> 15;
  const uint32_t dist = 0x7FFFu - (k & 0x7FFFu);
  // (the slot's winner: longest key, then nearest; the carried match's own
  // entry never wins; a walk that stopped at nice_len holds its exact length,
  // which no key exceeds)
  const bool upd = len > w.best_len;
  if (upd && (int)len >= P.nice_len) len = mq_measure(s, w.p - dist, w.p, w.max_len);
  const bool stop = upd && ((int)len >= P.nice_len || len >= w.max_len);
  const bool newo = upd && !stop && len >= 4;
  w.best_len = upd ? len : w.best_len;
  w.best_dist = upd ? dist : w.best_dist;
  w.active = w.active && !stop;
  w.o = newo ? len - 3 : w.o;
  w.omask = newo ? 0xFFFFFFFFu : w.omask;
  const uint32_t npw = ld32(s, w.p + w.o);
  w.pw = newo ? npw : w.pw;
}

// one pair loop of search_quad with queued measurement.  A wave-uniform
// loop of at most mc steps (no walk takes more hops): the passes need every
// lane, so no lane leaves before the wave's last walk ends; an inactive
// walk's hops push nothing.  The slots start at the walks' carried matches
// with the largest distance field, so that no candidate of equal length
// replaces one (as the walk's strict > keeps it).
__device__ __forceinline__ void mq_pair_loop(Walk &wa, Walk &wb, MatchShared *s, const DeflateParams &P, MqState &m,
                                             int mc) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  s->mr[wv][2 * lane] = wa.best_len >= 3 ? mq_key(wa.best_len, 0) : 0u;
  s->mr[wv][2 * lane + 1] = wb.best_len >= 3 ? mq_key(wb.best_len, 0) : 0u;
  m.head = m.tail = 0;
  m.ready = false;
  for (int step = 0; step < mc && __ballot(wa.active || wb.active) != 0; ++step) {
    walk_pair_hop_mq(wa, wb, s, P, step, m);
    // (every MQ_FLUSH + 1 steps the queue is measured even when short: long
    // chains would otherwise walk on with an old filter)
    if ((step & MQ_FLUSH) == MQ_FLUSH && m.tail != m.head) mq_process(s, P, m);
    if (m.ready) {
      mq_poll(wa, s, P, 2 * lane);
      mq_poll(wb, s, P, 2 * lane + 1);
      m.ready = false;
    }
  }
  // (fewer than 64 are left: one pass; bounded all the same)
  for (int k = 0; k < 2 && m.tail != m.head; ++k) mq_process(s, P, m);
  mq_poll(wa, s, P, 2 * lane);
  mq_poll(wb, s, P, 2 * lane + 1);
}


// finish position pb + K when the chain found nothing of the key's length:
// the near probes, then the newest earlier position with the same 4 bytes
// (the 4-byte-key table; the chains' 8-byte keys miss the 4..7-byte matches
// that make up much of source text)
template <int K, bool DICT>
__device__ __forceinline__ uint32_t walk_finish(const Walk &w, const MatchShared *s, const DeflateParams &P,
                                                const uint32_t (&win)[9], uint32_t near, uint32_t lim4, uint32_t d4,
                                                uint32_t floor, uint32_t &carry_len, uint32_t &carry_dist) {
  uint32_t best_len = w.best_len < w.cl ? w.cl : w.best_len, best_dist = w.best_dist;
  // a far 3-byte match (carried from the previous position) is dropped in
  // the end: it must not hide a near one
  if (best_len == 3 && best_dist > (uint32_t)P.too_far) best_len = 0;
  const bool short_ = best_len < (uint32_t)P.klen;
  if (near == 0 && w.max_len >= 3 && short_)
    near_probe<K, 1>(win, w.cur, w.cur2, DICT ? w.p - floor : w.p, w.max_len, P.probe, best_len, best_dist);
  // (positions from lim4 on have no 4-byte link: their keys would need bytes
  // past the segment's end)
  if (w.max_len >= 4 && short_ && w.p < lim4) {
    uint32_t qw[2];
    ld_run<2>(s, w.p - d4, qw);
    const uint32_t x0 = qw[0] ^ w.cur, x1 = qw[1] ^ w.cur2;
    uint32_t len = x0 ? 0u : 4 + min((uint32_t)(__ffs(x1) - 1) >> 3, 4u);
    len = len < w.max_len ? len : w.max_len;
    // a far match must be longer by two bytes than a near one to replace it
    // (its distance code costs more than the byte it gains)
    const uint32_t need = best_len + (best_len >= 3 && d4 > (uint32_t)P.too_far ? 2u : 1u);
    if (d4 != 0 && len >= 4 && len >= need && (len > 4 || d4 <= (uint32_t)ZT_DF_P4FAR)) {
      best_len = len;
      best_dist = d4;
    }
  }
  carry_len = best_len;
  carry_dist = best_dist;
  if (best_len == 3 && best_dist > (uint32_t)P.too_far) best_len = 0;
  return best_len >= 3 ? res_pack(0, best_len, best_dist) : 0u;
}

// longest match for positions [pb, pb + 4) of the sub-chunk [p0, p1) -> res_out[p - p0];
// matches end at pml (>= p1); floor: the first rel position that holds data
// (0, or a preset dictionary's first byte: near probes stop there, the chains
// and the 4-byte table never held a position below it).  DICT = false: the
// floor is 0 at compile time
// R = ROLE_PROBE adds the walks' counts to late and nmeas.  R = ROLE_QUEUED:
// every lane of the wave stays (the queue's passes need the whole wave);
// lanes past the sub-chunk walk nothing and store nothing.
template <bool DICT, Role R>
__device__ void search_quad(MatchShared *s, const DeflateParams &P, uint32_t pb, uint32_t p0, uint32_t p1,
                            uint32_t pml, uint32_t lim4, uint32_t floor, Key key, uint32_t *res_out, int mc,
                            [[maybe_unused]] uint32_t &late, [[maybe_unused]] uint32_t &nmeas) {
  [[maybe_unused]] MqState m;
  if constexpr (R == ROLE_QUEUED) {
    m.pml = pml;
    if (pb >= p1) pml = 0;  // (no walk of this lane starts: max_len 0)
  } else {
    if (pb >= p1) return;
  }
  // the pair loop of positions pb + k0 and pb + k0 + 2
  auto pair_loop = [&](Walk &wa, Walk &wb, uint32_t k0) {
    if constexpr (R == ROLE_QUEUED) {
      m.pbase = pb - 4 * (threadIdx.x & 63) + k0;
      mq_pair_loop(wa, wb, s, P, m, mc);
    } else {
      for (int step = 0; wa.active || wb.active; ++step) walk_pair_step<R>(wa, wb, s, P, step);
    }
  };
  // bytes [pb - 16, pb + 20) (pb is a multiple of 4; before rel 0 the words
  // are never used: near distances stay <= p)
  uint32_t w[9];
  ring_dwords<8>(s, ridx(pb - 16) >> 2, w);
  // the four positions' 4-byte-table links (final: the super-step waited for
  // them), read with the window so that walk_finish's lookups start from
  // the candidate's bytes -- one LDS round trip each instead of two
  const uint2 l4 = *reinterpret_cast<const uint2 *>(&s->link4[pb & (DF_SUB - 1)]);
  // (and the four chain links the walks start from: positions 1 and 3 begin
  // after 0 and 2 finish, their first link already in registers)
  const uint2 l8 = *reinterpret_cast<const uint2 *>(&s->prev[ridx(pb)]);
  // positions 0 and 2 walk together, then 1 and 3 with the carry of 0 and 2
  uint32_t out[4];
  uint32_t c0l, c0d, c2l, c2d, cl, cd;
  const uint32_t nr0 = near_any<0, 1>(w, win32<16>(w), ~0u), nr1 = near_any<1, 1>(w, win32<17>(w), ~0u);
  const uint32_t nr2 = near_any<2, 1>(w, win32<18>(w), ~0u), nr3 = near_any<3, 1>(w, win32<19>(w), ~0u);
  Walk wa, wb;
  wa.late = wb.late = 0;
  wa.nmeas = wb.nmeas = 0;
  walk_init(wa, s, P, pb, pml, win32<16>(w), win32<20>(w), win32<24>(w), win32<28>(w), 0, 0, l8.x & 0xFFFFu, mc);
  walk_init(wb, s, P, pb + 2, pml, win32<18>(w), win32<22>(w), win32<26>(w), win32<30>(w), 0, 0, l8.y & 0xFFFFu, mc);
  pair_loop(wa, wb, 0);
  out[0] = walk_finish<0, DICT>(wa, s, P, w, nr0, lim4, l4.x & 0xFFFFu, floor, c0l, c0d);
  out[2] = walk_finish<2, DICT>(wb, s, P, w, nr2, lim4, l4.y & 0xFFFFu, floor, c2l, c2d);
  walk_init(wa, s, P, pb + 1, pml, win32<17>(w), win32<21>(w), win32<25>(w), win32<29>(w), c0l, c0d, l8.x >> 16, mc);
  walk_init(wb, s, P, pb + 3, pml, win32<19>(w), win32<23>(w), win32<27>(w), win32<31>(w), c2l, c2d, l8.y >> 16, mc);
  pair_loop(wa, wb, 1);
  if constexpr (R == ROLE_PROBE) {
    late += wa.late + wb.late;
    nmeas += wa.nmeas + wb.nmeas;
  }
  out[1] = walk_finish<1, DICT>(wa, s, P, w, nr1, lim4, l4.x >> 16, floor, cl, cd);
  out[3] = walk_finish<3, DICT>(wb, s, P, w, nr3, lim4, l4.y >> 16, floor, cl, cd);
  // the positions' own bytes (res_pack)
  out[0] |= win32<16>(w) << 24;
  out[1] |= win32<17>(w) << 24;
  out[2] |= win32<18>(w) << 24;
  out[3] |= win32<19>(w) << 24;
  if constexpr (R == ROLE_QUEUED) {
    if (pb >= p1) return;
  }
  if (pb + 4 <= p1) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    u32x4 v = {out[0], out[1], out[2], out[3]};
    *reinterpret_cast<u32x4 *>(res_out + (pb - p0)) = v;
  } else {
    for (uint32_t k = 0; k < 4 && pb + k < p1; ++k) res_out[pb - p0 + k] = out[k];
  }
}

// DICT: a batch whose streams have a preset dictionary (D); false: the code
// of every launch without one, with no trace of the dictionary path
template <bool DICT>
__device__ __forceinline__ void match_body(const DeflateParams P, const DictView D, MatchShared &s) {
  const uint32_t t = threadIdx.x;
  // workgroups go to the 8 XCDs round robin, and every 8th super-chunk starts
  // a segment (no history: 18 % fewer positions): rotate each group of 8 so
  // that every XCD gets its share of those
  uint32_t wg = blockIdx.x;
  if ((wg | 7u) < gridDim.x) wg = (wg & ~7u) | ((wg + (wg >> 3)) & 7u);
  const bool big = wg < P.big_wgs;
  const uint32_t b0 = big ? wg * P.blocks_per_wg : P.big_wgs * P.blocks_per_wg + (wg - P.big_wgs) * P.tail_k;
  const uint32_t kb = big ? P.blocks_per_wg : P.tail_k;
  const uint32_t b1 = (b0 + kb) < P.nblocks ? (b0 + kb) : P.nblocks;
  if (P.store) {  // every block of the super-chunk goes stored: nothing to search
    bool all = true;
    for (uint32_t b = b0; b < b1; ++b) all = all && P.store[b];
    if (all) return;
  }
  // (batch: a workgroup's blocks belong to one stream, which starts at f_lo)
  const uint64_t f_lo = P.span ? P.halo + P.span[2 * (uint64_t)b0] : 0;
  const uint64_t f_end = P.span ? P.halo + P.span[2 * (uint64_t)b0 + 1] : P.end;
  const uint64_t s_lo = P.halo + (uint64_t)b0 * DF_BLOCK;
  const uint64_t s_hi = (P.halo + (uint64_t)b1 * DF_BLOCK) < f_end ? (P.halo + (uint64_t)b1 * DF_BLOCK) : f_end;
  // a segment start (restart point) sees no history: its matches stay inside
  // the segment, so inflate can decode segments independently
  const bool restart = P.span ? (((s_lo - f_lo) / DF_BLOCK) % P.restart) == 0
                              : (b0 % P.restart) == 0 && (b0 > 0 || P.halo == 0);
  // history: whole sub-chunks, so that the searched range starts on a sub-chunk
  const uint64_t hmax = P.hist_max;
  // a stream with a preset dictionary: its first workgroup's history is the
  // dictionary (D.dict: rel [0, hist), data from rel `floor` on), the stream
  // follows at rel hist; h_lo may then lie before the buffer (modular
  // arithmetic, no byte below rel hist is read through g)
  const bool dfirst = DICT && s_lo == f_lo;
  const uint64_t hist = dfirst    ? (uint64_t)D.hist
                        : restart ? 0
                                  : ((s_lo - f_lo) < hmax ? ((s_lo - f_lo) & ~uint64_t(DF_SUB - 1)) : hmax);
  const uint32_t floor = dfirst ? D.floor : 0u;
  const uint64_t h_lo = s_lo - hist;
  const uint8_t *g = DICT ? reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(P.base) + h_lo)
                          : P.base + h_lo;  // rel 0
  // rel r's bytes: the dictionary below dsplit (a multiple of DF_SUB: no
  // sub-chunk or head straddles it), else the stream
  const uint32_t dsplit = dfirst ? D.hist : 0u;
  const uint8_t *gd = dfirst ? D.dict : g;
  // (DICT = false keeps the expressions g + r of the plain kernel as they were)
  auto src = [&](uint32_t r) -> const uint8_t * { return (r < dsplit ? gd : g) + r; };
  const uint32_t rs = (uint32_t)(s_lo - h_lo), re = (uint32_t)(s_hi - h_lo);
  // bytes available for hashing: the stream's, but not past the end of the
  // super-chunk's segment (a restart point): positions near a segment end
  // are never linked, so a segment is searched alike whether the stream goes
  // on or ends there (a shard, a pipeline piece, zt_shard.py)
  const bool seg_end = s_hi == f_end || (P.span ? ((s_hi - f_lo) / DF_BLOCK) % P.restart == 0
                                                 : ((s_hi - P.halo) / DF_BLOCK) % P.restart == 0);
  const uint32_t rend = seg_end ? (uint32_t)(s_hi - h_lo) : (uint32_t)(f_end - h_lo);
  Key key;
  key.kmask = P.klen >= 4 ? 0xFFFFFFFFu : 0xFFFFFFu;
  key.kmask2 = P.klen >= 8 ? 0xFFFFFFFFu : P.klen == 6 ? 0xFFFFu : P.klen == 5 ? 0xFFu : 0u;
  const uint32_t kext = (uint32_t)P.klen - 1;  // a key at p needs bytes up to p + kext

  // the chain heads' format (workgroup-uniform): u32 until a block queues
  bool fmt16 = P.heads == 16;
  if (fmt16) {
    for (uint32_t i = t; i < DF_HSIZE / 2; i += DF_THREADS) s.head[i] = 0x80008000u;  // (rel 0 - 32768: out of reach)
  } else {
    for (uint32_t i = t; i < DF_HSIZE; i += DF_THREADS) s.head32[i] = kNoHead;
  }
  for (uint32_t i = t; i < DF_H4SIZE; i += DF_THREADS) s.head4[i] = kNoHead;
  // the last kext positions of the first sub-chunk read link4 before any
  // link reached their slots: no candidate (not the LDS left by an earlier
  // workgroup, which made the output depend on the run)
  for (uint32_t i = t; i < DF_SUB; i += DF_THREADS) s.link4[i] = 0;
  __syncthreads();
  uint32_t inserted = floor;  // positions [floor, inserted) are in the chains
  if (re > 0) load_sub(&s, DICT ? src(0) : g, 0, re < DF_SUB ? re : DF_SUB);
  // (the second sub-chunk's head: bytes [DF_SUB, DF_SUB + DF_HEAD); heads
  // run on past the super-chunk into the stream, so that a position at a
  // block end is linked and searched alike whatever the super-chunk size)
  if (DF_HEAD && t < (uint32_t)DF_HEAD && DF_SUB + t < rend) {
    ring_put8(&s, ridx(DF_SUB + t), DICT ? src(DF_SUB)[t] : g[DF_SUB + t]);
  }
  const bool g_aligned =
      ((reinterpret_cast<uintptr_t>(g) | (DICT ? reinterpret_cast<uintptr_t>(gd) : uintptr_t(0))) & 3) == 0;
  for (uint32_t p0 = 0; p0 < re; p0 += DF_SUB) {
    const uint32_t p1 = (p0 + DF_SUB) < re ? (p0 + DF_SUB) : re;
    lds_barrier();
    [[maybe_unused]] uint64_t t0, t1, t2, t3;
    DF_T(t0);
    // bytes in the ring: the sub-chunk and the next one's head
    const uint32_t dend = DF_HEAD ? (p1 + DF_HEAD < rend ? p1 + DF_HEAD : rend) : p1;
    uint32_t ih = dend >= kext ? dend - kext : 0;
    if (ih > p1) ih = p1;
    if (rend >= kext && ih > rend - kext) ih = rend - kext;
    const bool link = ih > inserted;
    // per-block depth: the block's first sub-chunk (the probe) walks max_chain
    // hops and counts late improvements; its verdict holds for the rest of
    // the block (a function of the block's own positions: streams do not
    // depend on how blocks are grouped into workgroups)
    const bool probe_sub = p0 >= rs && ((p0 - rs) % DF_BLOCK) == 0;
    if (t == 0) {
      s.linked = link ? inserted : ih;
      s.linked4 = link ? inserted : ih;
      s.work = 0;
      if (p0 > rs && ((p0 - rs) % DF_BLOCK) == DF_SUB) {  // (the probe's counts are complete: a barrier since)
        s.depth = P.adapt_depth && s.late * 4096u <= (uint32_t)P.adapt_thr * DF_SUB     ? P.adapt_depth
                  : P.adapt_depth2 && s.late2 * 4096u <= (uint32_t)P.adapt_thr2 * DF_SUB ? P.adapt_depth2
                                                                                          : P.max_chain;
        // (both ways of measuring give the same matches: the choice is one of time only)
        s.queued = P.mq_thr && (uint64_t)s.nmeas * 4096u >= (uint64_t)P.mq_thr * DF_SUB;
        atomicAdd(&g_match_modes[s.queued ? 0 : 1], 1ull);
      }
      if (probe_sub) s.late = s.late2 = s.nmeas = 0;
    }
    // the heads follow the block's way of measuring (the queues lie in the
    // u32 heads' upper half): every thread derives the verdict thread 0
    // stores in s.queued from the same count (complete since the barrier
    // that closed the probe sub-chunk; no one writes it before the next
    // probe), so the branch and its barrier are taken by all or by none
    bool converted = false;
    if (P.heads == 0 && P.mq_thr && p0 > rs && ((p0 - rs) % DF_BLOCK) == DF_SUB) {
      const uint32_t nm = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.nmeas);
      const bool want16 = (uint64_t)nm * 4096u >= (uint64_t)P.mq_thr * DF_SUB;
      if (want16 != fmt16) {
        if (want16)
          head_convert<true>(&s, p0);
        else
          head_convert<false>(&s, p0);
        if (t == 0) atomicAdd(&g_head_formats[want16 ? 0 : 1], 1ull);
        fmt16 = want16;
        converted = true;
      }
    }
    // the next sub-chunk is fetched while this one is searched
    const uint32_t n0 = p0 + DF_SUB;
    const bool fast = g_aligned && n0 + DF_SUB <= re;
    uint32_t nv = 0;
    if (fast) nv = reinterpret_cast<const uint32_t *>(DICT ? src(n0) : g + n0)[t];
    // and the head of the one after it (written with nv, after the search)
    const uint32_t hd0 = n0 + DF_SUB;
    const bool hload = DF_HEAD && t < (uint32_t)DF_HEAD && hd0 + t < rend;
    uint8_t hb = 0;
    if (hload) hb = DICT ? src(hd0)[t] : g[hd0 + t];
    // matches end at the block's end (or the data's)
    uint32_t pml = p1;
    if (DF_HEAD && p0 >= rs) {
      const uint32_t bend = rs + ((p0 - rs) / DF_BLOCK + 1) * DF_BLOCK;
      pml = bend < dend ? bend : dend;
    }
    if (link) hash_keys(&s, inserted, ih, key);
    // (a change to u16 at p0 left the heads as a sweep at p0 does)
    if (fmt16 && !converted && (p0 / DF_SUB) % HEAD_SWEEP == 0 && link) head_sweep(&s, p0);
    lds_barrier();
    DF_T(t1);
    // wave 0 links the 8-byte-key chains and wave 1 the 4-byte-key table,
    // step by step; every wave (waves 0 and 1 once done) takes super-steps of
    // 256 positions in order and searches them as soon as their links are
    // final (positions only read links of older ones)
    if (t < 64 && link) {
      if (fmt16)
        link_range<0, true>(&s, inserted, ih, key, P.link != 0);
      else
        link_range<0, false>(&s, inserted, ih, key, P.link != 0);
    }
    if (t >= 64 && t < 128 && link) link_range<1>(&s, inserted, ih, key, P.link != 0);
#ifdef ZT_DF_TIME
    uint64_t tl;
    DF_T(tl);
    if ((t & 63) == 0 && t < 128 && link) atomicAdd(&g_df_time[4], (unsigned long long)(tl - t1));
    uint64_t t_wait = 0, t_srch = 0, n_ss = 0;
#endif
    inserted = link ? ih : inserted;
    if (p0 >= rs) {
      const uint32_t nss = (p1 - p0 + 255) / 256;
      const int mc = probe_sub || !P.adapt_depth ? P.max_chain : s.depth;
      uint32_t late = 0, nmeas = 0;
      // (workgroup-uniform, fixed for the sub-chunk)
      const bool counting = P.adapt_depth || P.mq_thr;
      const Role role = probe_sub ? (counting ? ROLE_PROBE : ROLE_PLAIN) : counting && s.queued ? ROLE_QUEUED : ROLE_PLAIN;
      uint32_t *res_out = P.res + (h_lo + p0 - P.halo);  // res[input pos]: rel r <-> input h_lo + r - halo
      for (;;) {
        uint32_t ss = 0;
        if ((t & 63) == 0) ss = atomicAdd(&s.work, 1u);
        ss = (uint32_t)__shfl((int)ss, 0, 64);
        if (ss >= nss) break;
        const uint32_t need = (p0 + 256 * (ss + 1)) < ih ? (p0 + 256 * (ss + 1)) : ih;
#ifdef ZT_DF_TIME
        uint64_t w0, w1, w2;
        DF_T(w0);
#endif
        while (min(__hip_atomic_load(&s.linked, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP),
                   __hip_atomic_load(&s.linked4, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) < need)
          __builtin_amdgcn_s_sleep(1);
#ifdef ZT_DF_TIME
        DF_T(w1);
#endif
        const uint32_t pb = p0 + 256 * ss + 4 * (t & 63);
        if (role == ROLE_PROBE)
          search_quad<DICT, ROLE_PROBE>(&s, P, pb, p0, p1, pml, ih, DICT ? floor : 0u, key, res_out, mc, late, nmeas);
        else if (role == ROLE_QUEUED)
          search_quad<DICT, ROLE_QUEUED>(&s, P, pb, p0, p1, pml, ih, DICT ? floor : 0u, key, res_out, mc, late, nmeas);
        else
          search_quad<DICT, ROLE_PLAIN>(&s, P, pb, p0, p1, pml, ih, DICT ? floor : 0u, key, res_out, mc, late, nmeas);
#ifdef ZT_DF_TIME
        DF_T(w2);
        t_wait += w1 - w0;
        t_srch += w2 - w1;
        n_ss += 1;
#endif
      }
      if (probe_sub && P.adapt_depth) {
        // (per wave each half stays below 2^16: 256 positions x < 20 hops)
        for (int o = 32; o; o >>= 1) late += (uint32_t)__shfl_xor((int)late, o, 64);
        if ((t & 63) == 0 && (late & 0xFFFFu)) atomicAdd(&s.late, late & 0xFFFFu);
        if ((t & 63) == 0 && (late >> 16)) atomicAdd(&s.late2, late >> 16);
      }
      if (probe_sub && P.mq_thr) {
        for (int o = 32; o; o >>= 1) nmeas += (uint32_t)__shfl_xor((int)nmeas, o, 64);
        if ((t & 63) == 0 && nmeas) atomicAdd(&s.nmeas, nmeas);
      }
    }
    DF_T(t2);
    lds_barrier();
    DF_T(t3);
#ifdef ZT_DF_TIME
    // per wave (lane 0): hash phase, searching, barrier wait, (wave, sub-chunk)
    // pairs, link waits, super-steps, link + search loop
    if ((t & 63) == 0) {
      atomicAdd(&g_df_time[0], (unsigned long long)(t1 - t0));
      atomicAdd(&g_df_time[1], (unsigned long long)t_srch);
      atomicAdd(&g_df_time[2], (unsigned long long)(t3 - t2));
      atomicAdd(&g_df_time[3], 1ull);
      atomicAdd(&g_df_time[5], (unsigned long long)t_wait);
      atomicAdd(&g_df_time[6], (unsigned long long)n_ss);
      atomicAdd(&g_df_time[7], (unsigned long long)(t2 - t1));
    }
#endif
    if (fast) {
      ring_put32(&s, (ridx(n0) >> 2) + t, nv);
    } else if (n0 < re) {
      load_sub(&s, DICT ? src(n0) : g + n0, n0, (re - n0) < DF_SUB ? (re - n0) : DF_SUB);
    }
    if (hload) {
      ring_put8(&s, ridx(hd0 + t), hb);
    }
  }
}

__global__ __launch_bounds__(DF_THREADS) void match_kernel(DeflateParams P) {
  __shared__ MatchShared s;
  match_body<false>(P, DictView{}, s);
}
// batches with a preset dictionary
__global__ __launch_bounds__(DF_THREADS) void match_dict_kernel(DeflateParams P, DictView D) {
  __shared__ MatchShared s;
  match_body<true>(P, D, s);
}

__global__ void write_bytes(uint8_t *dst, uint64_t v, uint32_t n) {
  if (threadIdx.x < n) dst[threadIdx.x] = (uint8_t)(v >> (8 * threadIdx.x));
}

// reference-style stored blocks (compressionType NONE, src/RawDeflate.ts:93-100,122-153)
__global__ __launch_bounds__(256) void stored_blocks(const uint8_t *__restrict__ in, uint64_t n,
                                                     uint8_t *__restrict__ out, int final_) {
  const uint64_t b = blockIdx.x;
  const uint64_t lo = b * 65535, hi = (lo + 65535) < n ? lo + 65535 : n;
  const uint32_t len = (uint32_t)(hi - lo);
  uint8_t *o = out + b * (65535 + 5);
  if (threadIdx.x == 0) {
    o[0] = (final_ && hi == n) ? 1 : 0;
    o[1] = len & 0xFF;
    o[2] = len >> 8;
    o[3] = (~len) & 0xFF;
    o[4] = ((~len) >> 8) & 0xFF;
  }
  for (uint32_t i = threadIdx.x; i < len; i += 256) o[5 + i] = in[lo + i];
}

}  // namespace

// ---- host driver -----------------------------------------------------------------------------
struct DeflateLevel {
  int max_chain, nice, lazy, too_far, skip, klen, probe, good, opt;
  int adapt_depth = 0, adapt_thr = 0, adapt_depth2 = 0, adapt_thr2 = 0;  // per-block depth (DeflateParams)
  int mq_thr = 0;  // per-block queued measurement (DeflateParams; 0: never)
  int heads = 0;   // chain-head format (DeflateParams; 0: per block)
  int parse_serial = 0;  // the serial window walk in parse / price (DeflateParams)
  int link = 1;    // the link waves' lean groups and undrained progress (DeflateParams; 0: the former link)
};

// the level table: a function of the level alone (level_params applies the
// environment hooks)
static DeflateLevel level_table(int level) {
  switch (level) {
    // {max_chain, nice, lazy, too_far, skip, klen, probe, good}: chains on
    // 8-byte keys find the long matches (a 3-byte key chain of the same depth
    // sees mostly candidates that cannot win); near probes (registers) find
    // the short ones; a carried match of `good` bytes cuts the chain to 1/4
    case 1: return {4, 16, 0, 4096, 16, 8, 8, 4, 0};
    case 2: return {8, 32, 0, 4096, 32, 8, 8, 4, 0};
    case 3: return {16, 64, 0, 4096, 64, 8, 16, 4, 0};
    case 4: return {16, 128, 1, 4096, 128, 8, 16, 8, 1};
    case 5: return {24, 128, 1, 4096, 128, 8, 16, 16, 1};
    case 7: return {64, 258, 1, 4096, 258, 8, 16, 16, 1};
    case 8: return {128, 258, 1, 4096, 258, 8, 16, 32, 1};
    case 9: return {512, 258, 1, 4096, 258, 8, 16, 258, 1};
    default: break;
  }
  // 6: chain 28 since matches run past 4 KiB sub-chunk ends (DF_HEAD): the
  // 16-window gate's wordsalad worst 1.0179 (chain 32 without heads:
  // 1.0171), 5 % less chain walking (profiles/r04j_gate.log); 20 since the
  // DP tries cut lengths up to 24 (OP_SHORT): worst window 1.0190, match
  // 24.9 -> 22.4 ms per GiB (chain 18: 1.0225; profiles/r04os_sweep.txt)
  DeflateLevel L{20, 128, 1, 4096, 128, 8, 16, 16, 1};
  // per-block depth 6 when at most 40 of the probe's 4096 positions
  // improved at hop 6 or later, else 10 when at most 320 improved at hop 10
  // or later (the 16-window gate: worst window 1.0190 -> 1.0193, source 0.9875
  // -> 0.9904; match per GiB: source text 54.2 -> 44.2 ms, structured 16.6 ->
  // 15.1, the bench corpus 21.0 -> 20.5, wordsalad unchanged;
  // profiles/r06h_adapt_sweep.log, tools/adapt_sweep.py)
  L.adapt_depth = 6;
  L.adapt_thr = 40;
  L.adapt_depth2 = 10;
  L.adapt_thr2 = 320;
  // queued measurement where the probe measured a candidate at every
  // second position or more: wordsalad's blocks (97 %) and part of
  // source text's, none of structured data's (0.002 per position).  Match ms
  // per GiB with the threshold 0 / 256 / 1024 / 2048 / 3072: wordsalad 45.3
  // / 40.0 / 39.9 / 40.0 / 39.9, source text 44.4 / 43.7 / 43.4 / 43.1 /
  // 44.4, structured 16.3-16.4 throughout; 1 (every block that measured
  // anything) costs structured 11 %.  Off at the other levels: level 9's
  // long walks lose 40 % with it, level 1's 20 % (tools/experiments/README.md)
  L.mq_thr = 2048;
  return L;
}

// the level's parameters after the environment hooks (read per call: tests
// set them between calls)
static DeflateLevel level_params(int level) {
  DeflateLevel L = level_table(level);
  // tuning hook: ZT_DF_PARAMS="max_chain,nice,lazy,skip,klen,probe[,good[,opt]]"
  // overrides the level; set (even unparsable), level 6 loses its per-block
  // depth and queue defaults
  if (const char *e = getenv("ZT_DF_PARAMS")) {
    DeflateLevel O{64, 128, 1, 4096, 128, 8, 16, 8, 0};
    if (sscanf(e, "%d,%d,%d,%d,%d,%d,%d,%d", &O.max_chain, &O.nice, &O.lazy, &O.skip, &O.klen, &O.probe, &O.good,
               &O.opt) < 6)
      O = DeflateLevel{L.max_chain, L.nice, L.lazy, L.too_far, L.skip, L.klen, L.probe, L.good, L.opt};
    L = O;
  }
  // tuning hook: ZT_DF_ADAPT="depth,thr[,depth2,thr2]" (per-block depth; depth 0: off)
  if (const char *e = getenv("ZT_DF_ADAPT")) {
    int d = 0, t = 0, d2 = 0, t2 = 0;
    if (sscanf(e, "%d,%d,%d,%d", &d, &t, &d2, &t2) >= 2) {
      L.adapt_depth = d > 0 && d < L.max_chain ? d : 0;
      L.adapt_thr = t;
      L.adapt_depth2 = L.adapt_depth && d2 > d && d2 < L.max_chain ? d2 : 0;
      L.adapt_thr2 = t2;
    }
  }
  // tuning hook: ZT_DF_MQ=<n>: blocks whose probe measured at least n
  // candidates per 4096 positions measure through the queues (0: none, 1:
  // every block whose probe measured anything); the streams do not depend on it
  if (const char *e = getenv("ZT_DF_MQ")) L.mq_thr = atoi(e) > 0 ? atoi(e) : 0;
  // A/B and test hook: ZT_DF_HEADS=16: u16 chain heads throughout (the only
  // format before the per-block choice); 32: u32 throughout, which leaves no
  // room for the queues: no block queues; the streams do not depend on it
  if (const char *e = getenv("ZT_DF_HEADS")) {
    L.heads = atoi(e) == 16 ? 16 : atoi(e) == 32 ? 32 : 0;
    if (L.heads == 32) L.mq_thr = 0;
  }
  // A/B and test hook: ZT_PARSE_SERIAL=1: the serial window walk in
  // parse_kernel and price_kernel (the reference the lane-parallel walk is
  // tested against); the streams do not depend on it
  if (const char *e = getenv("ZT_PARSE_SERIAL")) L.parse_serial = atoi(e) != 0;
  // A/B and test hook: ZT_DF_LINK=0: the match kernel's former serial link
  // (bounds selects in every group, a drained release store per group); the
  // streams do not depend on it
  if (const char *e = getenv("ZT_DF_LINK")) L.link = atoi(e) != 0;
  return L;
}

static uint32_t deflate_nblocks(size_t n) {
  const uint32_t nb = (uint32_t)((n + DF_BLOCK - 1) / DF_BLOCK);
  return nb ? nb : 1;
}

// Work split: enough workgroups to cover every CU twice, at most 4 blocks
// (128 KiB) per workgroup (small super-chunks balance uneven data across
// CUs; each loads 28 KiB of history; 1 GiB mixed corpus, match kernel:
// 8 / 4 / 2 blocks 31.8 / 30.7 / 31.4 ms in round 2; round 4: 26.65 / 25.44 /
// 25.75 ms, 16 blocks 29.6; tools/experiments/README.md), a power of two so
// segments (32 blocks) align.
struct DeflateGeom {
  uint32_t k, nwg, big_wgs, tail_k;
};

static DeflateGeom deflate_geometry(const DeviceCtx *c, uint32_t nblocks) {
  DeflateGeom g;
  uint32_t kk = (nblocks + 2 * c->num_cu - 1) / (2 * c->num_cu);
  const uint32_t cap = (uint32_t)((128u << 10) / DF_BLOCK);
  // test hook: ZT_DF_SUPER_MIN = blocks per workgroup at least (within the
  // cap): a small input in multi-block workgroups, as large inputs run (read
  // per call; the streams do not depend on it)
  const char *min_env = getenv("ZT_DF_SUPER_MIN");
  if (min_env && atoi(min_env) > (int)kk) kk = (uint32_t)atoi(min_env);
  uint32_t k2 = 1;
  while (k2 < kk && k2 < cap) k2 <<= 1;
  g.k = k2;
  g.nwg = (nblocks + k2 - 1) / k2;
  // the last round of num_cu workgroups is the tail where CUs run dry: its
  // blocks go to one-block workgroups (streams identical; 1 GiB bench, match
  // kernel 25.47 -> 24.85 ms; 2-block tail 25.03, two tail rounds 24.92,
  // 8-block workgroups + tail 25.5: profiles/r04tail_sweep.txt).  Test hook:
  // ZT_DF_TAILK = blocks per tail workgroup (0 = none)
  static const int tk_env = getenv("ZT_DF_TAILK") ? atoi(getenv("ZT_DF_TAILK")) : -1;
  const uint32_t tk = tk_env >= 0 ? (uint32_t)tk_env : 1u;
  g.big_wgs = g.nwg;
  g.tail_k = k2;
  const uint64_t tail = (uint64_t)c->num_cu * k2;
  if (tk > 0 && tk < k2 && (k2 % tk) == 0 && (uint64_t)nblocks > tail) {
    g.big_wgs = (uint32_t)((nblocks - tail) / k2);
    g.tail_k = tk;
    g.nwg = g.big_wgs + (nblocks - g.big_wgs * k2 + tk - 1) / tk;
  }
  return g;
}

// The pipeline's scratch, carved in one place: the pointers and the size
// they need cannot drift apart.  Every piece starts 256-byte aligned.
struct DeflateScratch {
  uint32_t *res;       // nblocks x DF_BLOCK words
  uint8_t *slots;      // nblocks x DF_SLOT
  uint32_t *slot_len;  // nblocks
  uint64_t *off;       // nblocks + 1: scan_sizes
  BlockPlan *plans;    // nblocks
  uint8_t *store;      // nblocks flags (classify_kernel)
  uint32_t *nstore;    // the flagged-blocks counter, then the encode fault word
  uint64_t *span;      // batch: nblocks x [start, end)
  size_t bytes;        // all of it
};

// base null: the size alone
static DeflateScratch deflate_scratch(void *base, uint32_t nblocks, bool batch) {
  uint8_t *sb = static_cast<uint8_t *>(base);
  size_t at = 0;
  auto take = [&](size_t bytes) {
    void *p = sb ? sb + at : nullptr;
    at += (bytes + 255) & ~size_t(255);
    return p;
  };
  const size_t nb = nblocks;
  DeflateScratch S;
  S.res = static_cast<uint32_t *>(take(nb * DF_BLOCK * 4));
  S.slots = static_cast<uint8_t *>(take(nb * DF_SLOT));
  S.slot_len = static_cast<uint32_t *>(take(nb * 4));
  S.off = static_cast<uint64_t *>(take((nb + 1) * 8));
  S.plans = static_cast<BlockPlan *>(take(nb * sizeof(BlockPlan)));
  S.store = static_cast<uint8_t *>(take(nb));
  S.nstore = static_cast<uint32_t *>(take(8));
  take(256);  // (unused)
  S.span = batch ? static_cast<uint64_t *>(take(nb * 16)) : nullptr;
  S.bytes = at;
  return S;
}

size_t deflate_scratch_bytes(const DeviceCtx *, size_t n) {
  return deflate_scratch(nullptr, deflate_nblocks(n), false).bytes;
}
size_t deflate_batch_scratch_bytes(const DeviceCtx *, size_t padded) {
  return deflate_scratch(nullptr, deflate_nblocks(padded), true).bytes;
}

static_assert(kDictMaxTail == DF_MAXDIST && kDictSub == DF_SUB, "dict_host.h states the match kernel's geometry");

// bytes per independent segment: a deflate call on a slice that starts at a
// multiple of it (halo 0) writes that slice's part of the whole-buffer stream
size_t deflate_segment_bytes() { return (size_t)kRestartBlocks * DF_BLOCK; }

size_t deflate_bound_bytes(size_t n) {
  size_t nb = (n + DF_BLOCK - 1) / DF_BLOCK;
  return n + nb * 16 + (nb / 4 + 1) * kRestartMarkerLen + 64;
}

// What every call's DeflateParams has in common: the level after the hooks,
// the block count and the scratch.  The callers add their stream(s): base,
// halo, end, final_, the work split (blocks_per_wg, big_wgs, tail_k),
// restart and span.
// (level: resolve_opts', the strategy above the level's bits)
static DeflateParams deflate_params(int level, int ctype, uint32_t nblocks, const DeflateScratch &S, uint8_t *d_out) {
  const DeflateLevel L = level_params(level_plain(level));
  DeflateParams P{};
  P.strategy = level_strategy(level);
  P.nblocks = nblocks;
  P.hist_max = DF_HIST;
  P.max_chain = L.max_chain;
  P.nice_len = L.nice;
  P.lazy = L.lazy;
  P.too_far = L.too_far;
  P.skip_len = L.skip;
  P.klen = L.klen;
  P.probe = L.probe;
  P.good = L.good;
  P.adapt_depth = L.adapt_depth;
  P.adapt_thr = L.adapt_thr;
  P.adapt_depth2 = L.adapt_depth2;
  P.adapt_thr2 = L.adapt_thr2;
  P.mq_thr = L.mq_thr;
  P.heads = L.heads;
  P.parse_serial = L.parse_serial;
  P.link = L.link;
  P.ctype = ctype;
  P.opt = L.opt && ctype == 2;
  // classify_kernel runs for the best-of-three block choice (compressionType
  // DYNAMIC) with one parse block per DEFLATE block
  P.store = ctype == 2 && DF_GROUP == 1 ? S.store : nullptr;
  P.nstore = S.nstore;
  P.fault = S.nstore + 1;
  P.res = S.res;
  P.slots = S.slots;
  P.slot_len = S.slot_len;
  P.plans = S.plans;
  P.out = d_out;
  P.boff = S.off;
  return P;
}

// The pipeline's first part on s: classify -> match (nwg workgroups; D: the
// _dict kernels).  res holds every searched position's match word afterwards
// (zt_debug_match stops here).
static int deflate_match_launch(DeviceCtx *c, const DeflateParams &P, uint32_t nwg, const DictView *D, hipStream_t s) {
  if (P.strategy && D) return set_error(ZT_E_INTERNAL, "deflate: a strategy with a dictionary");
  ZT_HIP(hipMemsetAsync(P.nstore, 0, 8, s));
  if (P.store) {
    if (D)
      classify_dict_kernel<<<P.nblocks, 256, 0, s>>>(P, *D);
    else
      classify_kernel<<<P.nblocks, 256, 0, s>>>(P);
    ZT_HIP(hipGetLastError());
  }
  ZT_TRY(timing_begin(c, s, 0));
  if (P.strategy) {
    ZT_TRY(deflate_strategy_launch(P, s));
  } else {
    if (D)
      match_dict_kernel<<<nwg, DF_THREADS, 0, s>>>(P, *D);
    else
      match_kernel<<<nwg, DF_THREADS, 0, s>>>(P);
    ZT_HIP(hipGetLastError());
  }
  ZT_TRY(timing_end(c, s, 0));
  return ZT_OK;
}

// The pipeline on s: deflate_match_launch -> deflate_post_run (->
// deflate_index_kernel when the call asks for its index entries), then
// off[first .. nblocks] read back into h_off and the fault check.
static int deflate_pipeline(DeviceCtx *c, const DeflateParams &P, uint64_t *off, uint32_t nwg, const DictView *D,
                            uint32_t first, uint64_t *h_off, hipStream_t s, const DeflateIndexReq *ix = nullptr) {
  ZT_TRY(timing_begin(c, s, 1));
  ZT_TRY(deflate_match_launch(c, P, nwg, D, s));
  ZT_TRY(deflate_post_run(P, off, s));
  ZT_TRY(timing_end(c, s, 1));
  if (ix) ZT_TRY(deflate_index_launch(P, *ix, s));
  uint32_t nst[2] = {0, 0};  // blocks stored unsearched, fault bits
  {
    void *mb;
    const size_t bb = (size_t)(P.nblocks + 1 - first) * 8;
    ZT_TRY(mailbox(c, bb + 8, &mb));
    ZT_TRY(x_copy(mb, off + first, bb, s));
    ZT_TRY(x_copy((uint8_t *)mb + bb, P.nstore, 8, s));
    ZT_HIP(hipStreamSynchronize(s));
    memcpy(h_off, mb, bb);
    memcpy(nst, (uint8_t *)mb + bb, 8);
  }
  if (nst[1] & kFaultEncode) return set_error(ZT_E_INTERNAL, "deflate: a block's encoded size differs from its plan");
  if (nst[1]) return set_error(ZT_E_INTERNAL, "deflate: the index entries do not follow the restart markers");
  c->times.blocks_unsearched += nst[0];
  ZT_TRY(timing_collect(c, &c->times.deflate_ms, &c->times.deflate_launches, 0));
  ZT_TRY(timing_collect(c, &c->times.deflate_pipeline_ms, &c->times.deflate_pipelines, 1));
  return ZT_OK;
}

// One stream of n > 0 bytes at d_in (halo bytes of history in front of it) in
// one pipeline: its scratch, its parameters and its work split (deflate_dev_run
// and zt_debug_match)
struct DeflateCall {
  DeflateScratch S;
  DeflateParams P;
  uint32_t nwg;
};

static int deflate_stream_call(const DeviceCtx *c, const uint8_t *d_in, size_t n, size_t halo, int final_, int ctype,
                               int level, uint8_t *d_out, void *scratch_base, size_t scratch_size, DeflateCall *k) {
  const uint32_t nblocks = deflate_nblocks(n);
  const DeflateGeom G = deflate_geometry(c, nblocks);
  k->S = deflate_scratch(scratch_base, nblocks, false);
  if (k->S.bytes > scratch_size) return set_error(ZT_E_NOMEM, "deflate scratch too small");
  DeflateParams &P = k->P;
  P = deflate_params(level, ctype, nblocks, k->S, d_out);
  P.base = d_in - halo;
  P.halo = halo;
  P.end = halo + n;
  P.final_ = final_;
  P.blocks_per_wg = G.k;
  P.big_wgs = G.big_wgs;
  P.tail_k = G.tail_k;
  P.restart = (kRestartBlocks + G.k - 1) / G.k * G.k;
  k->nwg = G.nwg;
  return ZT_OK;
}

int deflate_dev_run(DeviceCtx *c, const uint8_t *d_in, size_t n, size_t halo, int final_, int ctype, int level,
                    uint8_t *d_out, size_t *out_len, void *scratch_base, size_t scratch_size, hipStream_t s,
                    const DeflateIndexReq *ix) {
  if (ix && (n == 0 || ctype == 0)) return set_error(ZT_E_INTERNAL, "deflate: no index entries for this call");
  if (n == 0) {  // one empty stored block
    write_bytes<<<1, 64, 0, s>>>(d_out, final_ ? 0xFFFF000001ull : 0xFFFF000000ull, 5);
    ZT_HIP(hipGetLastError());
    *out_len = 5;
    return ZT_OK;
  }
  if (ctype == 0) {
    // stored blocks of <= 65535 bytes (final one flagged)
    size_t nb = (n + 65534) / 65535;
    stored_blocks<<<(unsigned)nb, 256, 0, s>>>(d_in, n, d_out, final_);
    ZT_HIP(hipGetLastError());
    *out_len = n + 5 * nb;
    return ZT_OK;
  }
  DeflateCall k;
  ZT_TRY(deflate_stream_call(c, d_in, n, halo, final_, ctype, level, d_out, scratch_base, scratch_size, &k));
  uint64_t total = 0;
  ZT_TRY(deflate_pipeline(c, k.P, k.S.off, k.nwg, nullptr, k.P.nblocks, &total, s, ix));
  *out_len = total;
  return ZT_OK;
}

// Batch of independent streams in one pipeline (configs C4 / C2's producer):
// stream f's bytes are at d_in + off[f] (off 32 KiB aligned, increasing, each
// stream's blocks directly after the previous stream's), len[f] > 0.  Every
// workgroup of the match kernel takes one block, so a stream's history never
// reaches into another; each stream's last block carries BFINAL and restart
// markers stay inside streams.  Stream f's bytes land at d_out +
// out_off[f] .. out_off[f + 1] (host array of count + 1).
int deflate_batch_dev_run(DeviceCtx *c, const uint8_t *d_in, size_t count, const uint64_t *off, const uint64_t *len,
                          int ctype, int level, uint8_t *d_out, uint64_t *out_off, void *scratch_base,
                          size_t scratch_size, hipStream_t s, const DictHist *dict) {
  if (count == 0) return ZT_OK;
  if (dict && dict->d_hist &&
      (dict->hist == 0 || dict->hist % DF_SUB || dict->hist > (uint32_t)DF_HIST || dict->floor >= (uint32_t)DF_SUB ||
       dict->hist - dict->floor > (uint32_t)DF_MAXDIST || (reinterpret_cast<uintptr_t>(dict->d_hist) & 3)))
    return set_error(ZT_E_ARG, "invalid dictionary history");
  const uint64_t padded = off[count - 1] + ((len[count - 1] + DF_BLOCK - 1) / DF_BLOCK) * DF_BLOCK;
  const uint32_t nblocks = deflate_nblocks(padded);
  const DeflateScratch S = deflate_scratch(scratch_base, nblocks, true);
  if (S.bytes > scratch_size) return set_error(ZT_E_NOMEM, "deflate scratch too small");
  std::vector<uint64_t> span((size_t)nblocks * 2, 0);
  std::vector<uint32_t> first(count);
  for (size_t f = 0; f < count; ++f) {
    const uint64_t b0 = off[f] / DF_BLOCK, nb = (len[f] + DF_BLOCK - 1) / DF_BLOCK;
    if (off[f] % DF_BLOCK || len[f] == 0 || (f && b0 * DF_BLOCK != off[f - 1] + ((len[f - 1] + DF_BLOCK - 1) / DF_BLOCK) * DF_BLOCK))
      return set_error(ZT_E_ARG, "batch streams must be non-empty and packed at 32 KiB boundaries");
    first[f] = (uint32_t)b0;
    for (uint64_t b = b0; b < b0 + nb; ++b) {
      span[2 * b] = off[f];
      span[2 * b + 1] = off[f] + len[f];
    }
  }
  ZT_HIP(hipMemcpyAsync(S.span, span.data(), span.size() * 8, hipMemcpyHostToDevice, s));
  DeflateParams P = deflate_params(level, ctype, nblocks, S, d_out);
  P.base = d_in;
  P.halo = 0;
  P.end = padded;
  P.final_ = 1;
  P.blocks_per_wg = 1;
  P.big_wgs = nblocks;
  P.tail_k = 1;
  P.restart = kRestartBlocks;
  P.span = S.span;
  const bool has_dict = dict && dict->d_hist;
  const DictView DV{has_dict ? dict->d_hist : nullptr, has_dict ? dict->hist : 0u, has_dict ? dict->floor : 0u};
  std::vector<uint64_t> boff((size_t)nblocks + 1);
  ZT_TRY(deflate_pipeline(c, P, S.off, nblocks, has_dict ? &DV : nullptr, 0, boff.data(), s));
  for (size_t f = 0; f < count; ++f) out_off[f] = boff[first[f]];
  out_off[count] = boff[nblocks];
  return ZT_OK;
}

// (zt_internal.h: the member writers' compute step)
int deflate_members_dev(DeviceCtx *c, const uint8_t *d_in, size_t count, const uint64_t *off, const uint64_t *len,
                        int ctype, int level, uint8_t *d_body, uint64_t *out_off, void *scratch_base,
                        size_t scratch_size, const DictHist *dict, uint32_t *d_sums, hipEvent_t landed) {
  if (d_sums) {  // on the second stream, over the same device bytes
    if (!landed) {
      ZT_HIP(hipEventRecord(c->aux_ev, c->stream));
      landed = c->aux_ev;
    }
    ZT_HIP(hipStreamWaitEvent(c->aux, landed, 0));
    ZT_TRY(checksums_batch_dev(c, d_in, count, off, len, d_sums, c->aux));
    ZT_HIP(hipEventRecord(c->aux_ev, c->aux));
  }
  if (ctype == 0) return ZT_OK;  // (stored blocks are the caller's framing)
  return deflate_batch_dev_run(c, d_in, count, off, len, ctype, level, d_body, out_off, scratch_base, scratch_size,
                               c->stream, dict);
}

// blocks that measured through the queues, blocks that measured at once,
// since the last call (of the current device)
extern "C" int zt_debug_head_formats(uint64_t out[2]) {
  unsigned long long v[2] = {}, z[2] = {};
  ZT_HIP(hipDeviceSynchronize());
  ZT_HIP(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_head_formats), sizeof v));
  ZT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_head_formats), z, sizeof z));
  out[0] = v[0];
  out[1] = v[1];
  return ZT_OK;
}
extern "C" int zt_debug_match_modes(uint64_t out[2]) {
  unsigned long long v[2] = {}, z[2] = {};
  ZT_HIP(hipDeviceSynchronize());
  ZT_HIP(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_match_modes), sizeof v));
  ZT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_match_modes), z, sizeof z));
  out[0] = v[0];
  out[1] = v[1];
  return ZT_OK;
}

// the match stage's result for one stream (zt_internal.h)
extern "C" int zt_debug_match(const uint8_t *in, size_t n, size_t halo, int level, uint32_t *res, uint8_t *store,
                              uint32_t *info) {
  return zt_debug_match_strategy(in, n, halo, level, 0, res, store, info);
}

extern "C" int zt_debug_match_strategy(const uint8_t *in, size_t n, size_t halo, int level, int strategy,
                                       uint32_t *res, uint8_t *store, uint32_t *info) {
  if (!in || !res || !store || !info || n == 0 || halo > 32768)
    return set_error(ZT_E_ARG, "zt_debug_match: bad argument");
  ZT_TRY(strategy_check(strategy));
  const StrategyScope scope(strategy);
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  const zt_deflate_opts opts{2, 0, level};  // DYNAMIC: the blocks are classified
  int ct, lv;
  ZT_TRY(resolve_opts(&opts, &ct, &lv));
  hipStream_t s = c->stream;
  void *d_in, *d_scr;
  ZT_TRY(scratch(c, kIn, halo + n + 64, &d_in));
  const size_t ss = deflate_scratch_bytes(c, n);
  ZT_TRY(scratch(c, kDeflateOrDesc, ss, &d_scr));
  ZT_TRY(upload(c, d_in, in, halo + n, s));
  DeflateCall k;
  ZT_TRY(deflate_stream_call(c, (const uint8_t *)d_in + halo, n, halo, 1, ct, lv, nullptr, d_scr, ss, &k));
  const DeflateParams &P = k.P;
  // (length 511: a position the kernel never wrote stays visible)
  ZT_HIP(hipMemsetAsync(P.res, 0xFF, (size_t)P.nblocks * DF_BLOCK * 4, s));
  ZT_TRY(deflate_match_launch(c, P, k.nwg, nullptr, s));
  ZT_TRY(download(c, res, P.res, n * 4, s));
  ZT_TRY(download(c, store, k.S.store, P.nblocks, s));
  const uint32_t rec[kDebugMatchInfo] = {
      (uint32_t)DF_BLOCK,      (uint32_t)DF_SUB,       (uint32_t)DF_MAXDIST,    P.restart * (uint32_t)DF_BLOCK,
      P.blocks_per_wg,         (uint32_t)P.max_chain,  (uint32_t)P.nice_len,    (uint32_t)P.skip_len,
      (uint32_t)P.good,        (uint32_t)P.klen,       (uint32_t)P.probe,       (uint32_t)P.too_far,
      (uint32_t)ZT_DF_P4FAR,   (uint32_t)P.adapt_depth, (uint32_t)P.adapt_thr,  (uint32_t)P.adapt_depth2,
      (uint32_t)P.adapt_thr2,  (uint32_t)P.mq_thr,     P.nblocks,               k.nwg};
  memcpy(info, rec, sizeof rec);
  return ZT_OK;
}

#ifdef ZT_DF_TIME
extern "C" int zt_debug_df_time(unsigned long long *out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_df_time), sizeof(unsigned long long) * 8);
  unsigned long long z[8] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_df_time), z, sizeof z);
  return 0;
}
#endif

#ifdef ZT_DF_COUNT
extern "C" int zt_debug_df_count(unsigned long long *out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_df_count), sizeof(unsigned long long) * 8);
  unsigned long long z[8] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_df_count), z, sizeof z);
  return 0;
}
#endif

}  // namespace zt
