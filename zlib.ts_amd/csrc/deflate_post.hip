// deflate_post.hip -- the post-match stages of the raw DEFLATE encoder: from
// the match kernel's per-position words in res (deflate.hip) to the stream.
// Replaces src/RawDeflate.ts, src/Heap.ts and src/Bitstream.ts.
//
// Kernels over device memory, launched by deflate_post_run (the file's one
// exported function; the host driver in deflate.hip calls it after
// match_kernel):
//
//   1. price_kernel + optparse_kernel -- one wave per 32 KiB block: bit
//      prices from the greedy parse of the block's first quarter, then a
//      backward shortest-path DP over every position (cut lengths 3..16 and
//      the full match), choices written over res.
//   2. parse_kernel -- one wave per block: parse of the DP's choices
//      (lane-parallel: 64 lanes x 32 positions per step, the lanes' entries
//      settled by pointer jumping), tokens over res, histograms (a small
//      LDS footprint: many waves per CU).
//      block_kernel -- one wave per block: length-limited Huffman lengths by
//      wave-parallel package-merge, canonical codes, the RLE'd code-length
//      header, and the smallest of stored / fixed / dynamic.
//   3. encode_kernel -- 512 threads per block: prefix sum of per-thread bit
//      counts, word-parallel packing; every block ends byte-aligned with an
//      empty stored block (00 00 FF FF) so blocks concatenate bytewise.
//   4. scan_sizes (before encode_kernel: block_kernel plans every block's
//      exact size) places each block, encode_kernel writes it there; 1 MiB
//      segment boundaries get a restart marker (two empty stored blocks) for
//      segment-parallel inflate (inflate_seg.hip).
//
// Shared with deflate.hip through zt_internal.h ("deflate device pipeline"):
// DeflateParams, BlockPlan, the res word format and the block geometry.
#include "deflate_index_host.h"
#include "zt_internal.h"

namespace zt {

#ifdef ZT_DF_TIME
__device__ unsigned long long g_bk_time[8];  // debug: block_kernel phase cycles (lane 0), [6] = blocks
#endif

#ifndef ZT_ENC_THREADS
#define ZT_ENC_THREADS 512  // 128 / 256 / 512 / 1024: 1.70 / 1.42 / 1.38 / 1.75 ms per GiB (profiles/r02q_encode_variants.txt)
#endif
constexpr int ENC_THREADS = ZT_ENC_THREADS;

namespace {

__constant__ uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ uint32_t dist_sym(uint32_t d, uint32_t &ebits, uint32_t &evalue) {
  if (d <= 4) {
    ebits = 0;
    evalue = 0;
    return d - 1;
  }
  uint32_t x = d - 1;
  uint32_t k = 31 - __clz(x);
  ebits = k - 1;
  evalue = x & ((1u << (k - 1)) - 1);
  return 2 * k + ((x >> (k - 1)) & 1);
}

__device__ __forceinline__ uint32_t len_sym(uint32_t L) {  // 0..28 (symbol - 257)
  if (L == 258) return 28;
  if (L <= 10) return L - 3;
  uint32_t x = L - 3;
  uint32_t k = 31 - __clz(x);  // >= 3
  return 4 * (k - 1) + ((x >> (k - 2)) & 3);
}

// ================================ 2. block_kernel ================================
constexpr int PM_MAX = 2 * 286;  // package-merge list length bound (2m - 2)
// words of a level's package bitmap: a bit for every list entry.  (PM_MAX / 32
// = 17 words stopped at entry 543: from 274 used symbols on, the entries past
// it set bits in the next level's row, and the codes came out incomplete)
constexpr int PM_WORDS = (PM_MAX + 31) / 32;
static_assert(PM_WORDS * 32 >= PM_MAX, "a package bit for every list entry");
struct HufScratch {
  uint32_t key[320];              // (freq << 9) | symbol, sorted ascending (the first m are used)
  uint32_t lst[2][PM_MAX];        // package-merge lists (weights), ping-pong
  uint32_t pkg[14][PM_WORDS];     // per level: which list entries are packages
  uint32_t items[16];             // selected items per level
  uint32_t bl_count[16];
};

// lane-parallel parse (parse_block_lanes): a step is 64 lanes x PL_LANE
// positions, each lane's res words staged in an LDS row of its own
constexpr int PL_LANE = 32;            // positions per lane: one 128-byte line of res
constexpr int PL_STEP = 64 * PL_LANE;  // positions per step
// dwords per row, odd: word j of the 64 rows falls in 32 distinct banks per half-wave
constexpr int PL_ROW = PL_LANE + 1;
struct LaneStage {
  uint32_t row[64][PL_ROW];  // res words of the step, the length after the lazy rule
  uint8_t ent[64];           // entry offset handed to a lane by the on-path lane that jumps into it
};

struct BlockShared {
  uint32_t lit_hist[288];
  uint32_t dist_hist[32];
  uint32_t n_cl_syms, hlit, hdist, hclen;
  union {
    struct {
      uint32_t lit_code[288];
      uint32_t dist_code[32];
      uint32_t cl_code[19];
      uint8_t lit_len[288];
      uint8_t dist_len[32];
      uint8_t cl_len[20];
      uint16_t cl_syms[320];  // sym | extra_value << 5
      HufScratch huf;
    };
  };
};

// One wave per workgroup: LDS operations of a wave complete in order, so a
// hand-off between lanes only needs the compiler not to reorder.
__device__ __forceinline__ void wsync() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// freq[0..n) -> len[0..n), limited to `limit` bits.  Always produces a complete
// code with >= 2 symbols (zlib's rule), forcing symbols 0/1 in when needed.
// ascending bitonic sort of 64 * R keys held R per lane (key index lane * R + r):
// partners inside a lane are register swaps, others one cross-lane shuffle
template <int R>
__device__ __forceinline__ void reg_bitonic(uint32_t (&key)[R], int lane) {
  constexpr int N = 64 * R;
#pragma unroll
  for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j < R) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if ((r & j) == 0) {
            const uint32_t i = (uint32_t)lane * R + r;
            const bool up = (i & k) == 0;
            const uint32_t a = key[r], b = key[r | j];
            const bool sw = (a > b) == up;
            key[r] = sw ? b : a;
            key[r | j] = sw ? a : b;
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const uint32_t other = (uint32_t)__shfl_xor((int)key[r], j / R, 64);
          const uint32_t i = (uint32_t)lane * R + r;
          const bool up = (i & k) == 0;
          const bool lower = (i & j) == 0;
          const uint32_t mn = key[r] < other ? key[r] : other, mx = key[r] < other ? other : key[r];
          key[r] = (lower == up) ? mn : mx;
        }
      }
    }
  }
}

// keys (freq << 9 | symbol, or ~0 for unused) sorted ascending into h.key[0..)
template <int R>
__device__ __forceinline__ void sort_keys(HufScratch &h, const uint32_t *freq_in, int n, int lane) {
  uint32_t key[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = lane * R + r;
    const uint32_t f = i < n ? freq_in[i] : 0u;
    key[r] = (i < n && f) ? ((f << 9) | (uint32_t)i) : 0xFFFFFFFFu;
  }
  reg_bitonic<R>(key, lane);
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (lane * R + r < 320) h.key[lane * R + r] = key[r];
}

// (always inlined: left to the inliner, block_kernel's three calls came out
// differently once debug_huffman_kernel called it too -- block_kernel 0.598 ->
// 0.653 ms per GiB; inlined everywhere 0.579, profiles/huffman_audit.txt)
__device__ __forceinline__ void huff_lengths(BlockShared *s, const uint32_t *freq_in, int n, int limit,
                                             uint8_t *len_out) {
  const int lane = threadIdx.x & 63;
  HufScratch &h = s->huf;
  for (int i = lane; i < n; i += 64) len_out[i] = 0;
  wsync();
  uint32_t m = 0;
  for (int i = lane; i < n; i += 64) m += (freq_in[i] != 0);
  for (int off = 32; off; off >>= 1) m += __shfl_xor(m, off, 64);
  if (m < 2) {
    // a complete code needs two symbols (zlib rejects a lone one-bit code)
    if (lane == 0) {
      int a = -1;
      for (int i = 0; i < n; ++i)
        if (freq_in[i]) a = i;
      int b0 = (a == 0) ? 1 : 0;
      if (a < 0) {
        len_out[0] = 1;
        len_out[1] = 1;
      } else {
        len_out[a] = 1;
        len_out[b0] = 1;
      }
    }
    wsync();
    return;
  }
  // sort by (frequency, symbol) in registers
  if (n <= 64)
    sort_keys<1>(h, freq_in, n, lane);
  else
    sort_keys<8>(h, freq_in, n, lane);
  wsync();
  // Length-limited optimal code lengths by package-merge, wave-parallel: the
  // level-j list is the items merged with the packages (pairs) of the level
  // j-1 list, kept to its first 2m - 2 entries; each merge by merge-path
  // (every lane a contiguous run of outputs after a binary search).  The
  // selection is then a prefix of every level: c_L = 2m - 2 entries at the
  // top, c_{j-1} = 2 x (packages among the first c_j), and item k's code
  // length is the number of levels whose selected prefix holds it.
  const uint32_t mm = m, cap = 2 * mm - 2;
  for (uint32_t i = lane; i < mm; i += 64) h.lst[0][i] = h.key[i] >> 9;
  for (int j = 0; j < limit - 1; ++j)
    for (uint32_t w = lane; w < PM_WORDS; w += 64) h.pkg[j][w] = 0;
  wsync();
  uint32_t lp = mm;  // length of the previous level's list
  for (int j = 1; j < limit; ++j) {
    const uint32_t *P = h.lst[(j - 1) & 1];
    uint32_t *Q = h.lst[j & 1];
    const uint32_t np = lp / 2;
    const uint32_t lq = mm + np < cap ? mm + np : cap;
    auto A = [&](uint32_t i) -> uint32_t { return h.key[i] >> 9; };
    auto B = [&](uint32_t i) -> uint32_t { return P[2 * i] + P[2 * i + 1]; };
    const uint32_t per = (lq + 63) / 64;
    const uint32_t d = (uint32_t)lane * per;
    if (d < lq) {
      // merge path: a = items among the first d outputs (items first on ties)
      uint32_t lo = d > np ? d - np : 0, hi = d < mm ? d : mm;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A(mid) <= B(d - mid - 1)) lo = mid + 1;
        else hi = mid;
      }
      uint32_t ia = lo, ib = d - lo;
      const uint32_t e = d + per < lq ? d + per : lq;
      for (uint32_t o = d; o < e; ++o) {
        const bool take_a = ib >= np || (ia < mm && A(ia) <= B(ib));
        Q[o] = take_a ? A(ia) : B(ib);
        if (!take_a) atomicOr(&h.pkg[j - 1][o >> 5], 1u << (o & 31));
        ia += take_a ? 1 : 0;
        ib += take_a ? 0 : 1;
      }
    }
    wsync();
    lp = lq;
  }
  // selection, top level down (lane 0; 15 steps of a popcount)
  if (lane == 0) {
    uint32_t c = cap;
    for (int j = limit - 1; j >= 1; --j) {
      uint32_t pk = 0;
      for (uint32_t w = 0; w < (c >> 5); ++w) pk += __popc(h.pkg[j - 1][w]);
      if (c & 31) pk += __popc(h.pkg[j - 1][c >> 5] & ((1u << (c & 31)) - 1));
      h.items[j] = c - pk;
      c = 2 * pk;
    }
    h.items[0] = c;
  }
  wsync();
  for (uint32_t k = lane; k < mm; k += 64) {
    uint32_t l = 0;
    for (int j = 0; j < limit; ++j) l += k < h.items[j] ? 1u : 0u;
    len_out[h.key[k] & 511] = (uint8_t)l;
  }
  wsync();
}

// canonical codes (bit-reversed for LSB-first emission), wave-parallel: the
// rank of a symbol among equal lengths by ballots per 64-symbol chunk
__device__ void huff_codes(const uint8_t *len, int n, uint32_t *code) {
  const int lane = threadIdx.x & 63;
  uint32_t cnt = 0;  // lane l < 16: symbols of length l
  for (int b0 = 0; b0 < n; b0 += 64) {
    const int i = b0 + lane;
    const uint32_t l = i < n ? len[i] : 0u;
#pragma unroll
    for (int L = 1; L < 16; ++L) {
      const uint32_t c = (uint32_t)__popcll(__ballot(l == (uint32_t)L));
      if (lane == L) cnt += c;
    }
  }
  // first code of each length: next[l] = (next[l-1] + cnt[l-1]) << 1
  uint32_t next = 0, run = 0;
  for (int L = 1; L < 16; ++L) {
    const uint32_t prev_cnt = L > 1 ? (uint32_t)__builtin_amdgcn_readlane((int)cnt, L - 1) : 0u;
    run = (run + prev_cnt) << 1;
    if (lane == L) next = run;
  }
  for (int b0 = 0; b0 < n; b0 += 64) {
    const int i = b0 + lane;
    const uint32_t l = i < n ? len[i] : 0u;
    uint32_t v = 0;
#pragma unroll
    for (int L = 1; L < 16; ++L) {
      const uint64_t peers = __ballot(l == (uint32_t)L);
      const uint32_t base = (uint32_t)__builtin_amdgcn_readlane((int)next, L);
      if (l == (uint32_t)L) v = base + (uint32_t)__popcll(peers & lanemask_lt(lane));
      if (lane == L) next += (uint32_t)__popcll(peers);
    }
    if (i < n) code[i] = l ? ((l << 16) | (__brev(v) >> (32 - l))) : 0u;
  }
  wsync();
}

__device__ __forceinline__ uint32_t fixed_lit(uint32_t sym) {
  uint32_t l, c;
  if (sym <= 143) {
    l = 8;
    c = 0x30 + sym;
  } else if (sym <= 255) {
    l = 9;
    c = 0x190 + sym - 144;
  } else if (sym <= 279) {
    l = 7;
    c = sym - 256;
  } else {
    l = 8;
    c = 0xC0 + sym - 280;
  }
  return (l << 16) | (__brev(c) >> (32 - l));
}


// LDS histogram increment as inline asm: one ds_add_u32 without a returned
// value.  (LDS operations complete in order, so the compiler's own lgkmcnt
// waits stay sufficient.)
__device__ __forceinline__ void lds_inc(uint32_t *p) {
  const uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)p;
  __asm__ volatile("ds_add_u32 %0, %1" ::"v"(a), "v"(1u) : "memory");
}

#ifndef ZT_PW_SCALAR
#define ZT_PW_SCALAR 3  // match lanes up to which a window's path is walked by scalar jumps
#endif
// parse -> tokens over res, histograms.  One 64-position window per step:
// the path through it from `entry` (a scalar walk over the match lanes, or
// pointer doubling when they are many), its tokens written in order.
// (WRITE = false: histograms of the greedy parse only, res untouched)
template <bool WRITE, class S>
__device__ __forceinline__ void parse_window(S *s, const DeflateParams &P, uint32_t *r_blk, uint32_t len, uint32_t w0,
                                             uint32_t r, uint32_t r_next, uint32_t &entry, uint32_t &ntok) {
  const int lane = threadIdx.x & 63;
    const uint32_t i = w0 + lane;
    uint32_t L = res_len(r);
    if (P.lazy && !P.opt) {
      // one-step lazy: a longer match at i + 1 defers this one
      uint32_t nb = res_len((uint32_t)__shfl_down((int)r, 1, 64));
      const uint32_t first_next = res_len((uint32_t)__shfl((int)r_next, 0, 64));
      if (lane == 63) nb = first_next;
      if (L >= 3 && i + 1 < len && nb > L) L = 0;
    }
    // the path through the window.  Few match lanes past the entry: a scalar
    // walk (literal runs up to the next match lane, then a jump past it);
    // many: pointer doubling (6 rounds of lane shuffles)
    const uint64_t valid = __ballot(i < len);
    const uint64_t mm = __ballot(i < len && L >= 3);
    uint64_t path = 0;
    uint32_t exit;
    if (__popcll(mm & (~0ull << entry)) <= ZT_PW_SCALAR) {
      uint32_t cur = entry;
      while (cur < 64) {
        const uint64_t rest = mm & (~0ull << cur);
        const uint32_t m = rest ? (uint32_t)__builtin_ctzll(rest) : 64u;
        path |= (m >= 64 ? ~0ull : ((1ull << m) - 1)) & (~0ull << cur);
        if (m >= 64) {
          cur = 64;
          break;
        }
        path |= 1ull << m;
        cur = m + (uint32_t)__builtin_amdgcn_readlane((int)L, (int)m);
      }
      path &= valid;
      exit = cur;
    } else {
      const uint32_t step = L >= 3 ? L : 1;
      uint32_t ptr = i < len ? lane + step : 64u;
      uint64_t mask = i < len ? 1ull << lane : 0ull;
      // rounds until every lane's chain has left the window (at most 6)
      for (int rnd = 0; rnd < 6 && __ballot(ptr < 64); ++rnd) {
        const bool in = ptr < 64;
        const int src = in ? (int)ptr : lane;
        uint32_t mlo = __shfl((uint32_t)mask, src, 64);
        uint32_t mhi = __shfl((uint32_t)(mask >> 32), src, 64);
        uint32_t nptr = __shfl(ptr, src, 64);
        if (in) {
          mask |= ((uint64_t)mhi << 32) | mlo;
          ptr = nptr;
        }
      }
      // (readlane returns int: go through uint32_t so the low half is not sign-extended)
      const uint32_t path_hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mask >> 32), (int)entry);
      const uint32_t path_lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mask, (int)entry);
      path = ((uint64_t)path_hi << 32) | path_lo;
      exit = (uint32_t)__builtin_amdgcn_readlane((int)ptr, (int)entry);
    }
    const bool on = (path >> lane) & 1;
    // one literal / length increment for every path lane, then the distances
    // (the two branches issued one LDS atomic instruction each: parse 2.35 ->
    // 2.29 ms, price 0.565 -> 0.554 per GiB, streams identical; variant abH
    // of the round 6 post-match micro-variants, tools/experiments/README.md)
    if (on) {
      const bool mt = L >= 3;
      const uint32_t token = mt ? (L << 16) | res_dist(r) : res_byte(r);
      lds_inc(&s->lit_hist[mt ? 257 + len_sym(L) : token]);
      if (mt) {
        uint32_t eb, ev;
        lds_inc(&s->dist_hist[dist_sym(res_dist(r), eb, ev)]);
      }
      if (WRITE) r_blk[ntok + __popcll(path & lanemask_lt(lane))] = token;
    }
    ntok += __popcll(path);
    entry = exit - 64;
}

// register-prefetch driver (any alignment / length)
constexpr int PB_PF = 6;  // parse windows prefetched
template <bool WRITE, class S>
__device__ uint32_t parse_block_regs(S *s, const DeflateParams &P, uint32_t *r_blk, uint32_t len) {
  const int lane = threadIdx.x & 63;
  uint32_t entry = 0;  // first path position relative to the current window
  uint32_t ntok = 0;
  // software pipeline: PB_PF windows' loads are in flight while one is parsed
  // (rq[j] holds window w0 + 64 j; rq[j + 1] is the lazy look-ahead)
  uint32_t rq[PB_PF];
#pragma unroll
  for (int j = 0; j < PB_PF; ++j) {
    const uint32_t p = 64u * j + lane;
    rq[j] = p < len ? r_blk[p] : 0u;
  }
  for (uint32_t wb = 0; wb < len; wb += 64 * PB_PF) {
#pragma unroll
    for (int j = 0; j < PB_PF; ++j) {
      const uint32_t w0 = wb + 64u * j;
      if (w0 >= len) break;
      const uint32_t r = rq[j];
      {
        const uint32_t p = w0 + 64u * PB_PF + lane;
        rq[j] = p < len ? r_blk[p] : 0u;
      }
      const uint32_t r_next = rq[(j + 1) % PB_PF];
      if (entry >= 64) {
        entry -= 64;
        continue;
      }
      parse_window<WRITE>(s, P, r_blk, len, w0, r, r_next, entry, ntok);
    }
  }
  return ntok;
}

// ---- lane-parallel driver -------------------------------------------------
// The choice at every position is fixed before the parse (the match, the lazy
// rule or the DP's length), so the walk only finds which positions lie on the
// path from the start: list ranking.  A step covers PL_STEP positions, lane k
// the PL_LANE positions from 32 k on, held as one row of LDS words.
//
// The path through one lane's positions from offset e: literal runs by mask
// arithmetic on the match mask mm, one length lookup per match on the path.
// `old` is the path of an earlier walk of the lane (0: none): once the walk
// reaches one of its positions, the rest of the path and the exit ex (>=
// PL_LANE, relative to the lane) are that walk's.
__device__ __forceinline__ void lane_walk(const uint32_t *row, uint32_t mm, uint32_t e, uint32_t old, uint32_t &path,
                                          uint32_t &ex) {
  uint32_t p = 0, cur = e;
  bool merged = false;
  while (cur < (uint32_t)PL_LANE) {
    const uint32_t from = ~0u << cur;
    const uint32_t rest = mm & from;
    const uint32_t m = rest ? (uint32_t)__builtin_ctz(rest) : 32u;  // next match, or the end
    const uint32_t below = m >= 32 ? ~0u : (1u << m) - 1;
    const uint32_t upto = m >= 31 ? ~0u : (2u << m) - 1;
    if (old & from & upto) {
      p |= (below | old) & from;
      merged = true;
      break;
    }
    p |= below & from;
    cur = m;
    if (m < 32) {
      p |= 1u << m;
      cur = m + res_len(row[m]);
    }
  }
  path = p;
  if (!merged) ex = cur;
}

typedef unsigned int pl_u32x4 __attribute__((ext_vector_type(4)));

// The lane's words w (sequence positions pos0 ..) into its row, branch-free
// and statically unrolled; returns the mask of match positions.  LZ: the
// one-step lazy rule as in parse_window (a longer match at i + 1 < slen defers
// the one at i: its length field is cleared); nbw is the word after the
// lane's last.
template <bool LZ>
__device__ __forceinline__ uint32_t lane_facts(uint32_t *row, const pl_u32x4 (&w)[PL_LANE / 4], uint32_t nbw,
                                               uint32_t pos0, uint32_t slen) {
  uint32_t mm = 0;
#pragma unroll
  for (int j = 0; j < PL_LANE; ++j) {
    uint32_t r = w[j >> 2][j & 3];
    uint32_t L = res_len(r);
    if (LZ) {
      const uint32_t nb = res_len(j + 1 < PL_LANE ? w[((j + 1) & 31) >> 2][(j + 1) & 3] : nbw);
      const bool defer = (L >= 3) & (nb > L) & (pos0 + (uint32_t)j + 1 < slen);
      r = defer ? r & ~(511u << 15) : r;
      L = defer ? 0u : L;
    }
    mm |= (L >= 3 ? 1u : 0u) << j;
    row[j] = r;
  }
  return mm;
}

// One sequence of len positions at r_blk (PIECE = 0), or npieces sequences of
// PIECE positions each, `stride` words apart, every one walked from its own
// start with nothing carried between them (PIECE / PL_LANE lanes per piece,
// as many pieces per step as fill the wave).  Per step:
//  1. every lane loads its line of res (the next step's is prefetched), applies
//     the lazy rule, builds its match mask and stages the words in its row;
//  2. every lane walks its positions from offset 0 (the sequence's first lane
//     from the carried entry): a speculative path and exit;
//  3. the exits link the lanes into lists; pointer jumping finds the lanes on
//     the list from the sequence's entry lane, each on-path lane hands its
//     successor the offset it enters at, and a lane whose walk assumed another
//     offset walks again (lane_walk joins its earlier path where they meet).
//     Repeated until no on-path lane changed: every round settles at least the
//     leftmost unsettled on-path lane, so at most 64 rounds for any data;
//  4. on-path lanes emit their tokens in position order (a wave prefix sum of
//     the per-lane counts places them) and count the histograms.
// In place: after step t, ntok <= PL_STEP (t + 1), so a step's stores end at or
// before the end of its own positions; its words are in LDS by then (the
// stores depend on them), the prefetched next step lies wholly beyond, and
// later steps are loaded only after these stores.
// (WRITE = false: histograms only, res untouched)
template <bool WRITE, int PIECE, class S>
__device__ uint32_t parse_block_lanes(S *s, const DeflateParams &P, uint32_t *r_blk, uint32_t len, uint32_t npieces,
                                      uint32_t stride) {
  static_assert(PIECE % PL_LANE == 0 && (PIECE == 0 || PL_STEP % PIECE == 0), "pieces are whole lanes, steps whole pieces");
  constexpr uint32_t LP = PIECE ? PIECE / PL_LANE : 64;  // lanes per sequence in a step
  constexpr uint32_t PS = 64 / LP;                       // sequences per step
  const uint32_t lane = threadIdx.x & 63;
  LaneStage *st = &s->stage;
  uint32_t *row = st->row[lane];
  const bool lz = P.lazy && !P.opt;
  const uint32_t nsteps = PIECE ? (npieces + PS - 1) / PS : (len + PL_STEP - 1) / PL_STEP;
  const uint32_t sl = lane & (LP - 1);  // lane within its sequence's lanes
  // the lane's line in step t: position within its sequence, that sequence's
  // length (0: none) and the words
  auto seq_pos = [&](uint32_t t) -> uint32_t { return PIECE ? sl * PL_LANE : t * PL_STEP + lane * PL_LANE; };
  auto seq_len = [&](uint32_t t) -> uint32_t {
    if (!PIECE) return t < nsteps ? len : 0u;
    return t * PS + lane / LP < npieces ? (uint32_t)PIECE : 0u;
  };
  auto load = [&](uint32_t t, pl_u32x4 *w) {
    const uint32_t *src = PIECE ? r_blk + (size_t)(t * PS + lane / LP) * stride + sl * PL_LANE
                                : r_blk + t * PL_STEP + lane * PL_LANE;
    const bool in = seq_pos(t) < seq_len(t);
#pragma unroll
    for (int q = 0; q < PL_LANE / 4; ++q)
      w[q] = in ? reinterpret_cast<const pl_u32x4 *>(src)[q] : pl_u32x4{0u, 0u, 0u, 0u};
  };
  uint32_t entry = 0;  // first path position of the sequence not yet walked (PIECE = 0)
  uint32_t ntok = 0;
  pl_u32x4 nw[PL_LANE / 4];
  load(0, nw);
  for (uint32_t t = 0; t < nsteps; ++t) {
    pl_u32x4 cw[PL_LANE / 4];
#pragma unroll
    for (int q = 0; q < PL_LANE / 4; ++q) cw[q] = nw[q];
    load(t + 1, nw);
    const uint32_t pos0 = seq_pos(t), slen = seq_len(t);
    const uint32_t nvalid = pos0 < slen ? (slen - pos0 < (uint32_t)PL_LANE ? slen - pos0 : (uint32_t)PL_LANE) : 0u;
    const uint32_t vm = nvalid >= 32 ? ~0u : (1u << nvalid) - 1;
    // 1. lazy rule, match mask, rows.  The neighbour of the lane's last
    // position is the next lane's first word, lane 63's the next step's
    uint32_t nbw = 0;
    if (lz) {
      nbw = (uint32_t)__shfl_down((int)cw[0][0], 1, 64);
      const uint32_t first_next = (uint32_t)__shfl((int)nw[0][0], 0, 64);
      if (lane == 63) nbw = first_next;
    }
    // (one wave-uniform branch on the lazy rule around the 32 unrolled
    // positions: tested per position it cost an exec-mask branch each, 700
    // instructions per step for this part)
    const uint32_t mm = (lz ? lane_facts<true>(row, cw, nbw, pos0, slen) : lane_facts<false>(row, cw, nbw, pos0, slen)) & vm;
    // 2. speculative walk
    uint32_t src, soff, send;  // the sequence's entry lane and offset; the end of its lanes in this step
    if (PIECE) {
      src = lane & ~(LP - 1);
      soff = 0;
      send = (uint32_t)PIECE;
    } else {
      const uint32_t rel = entry - t * PL_STEP;  // < PL_STEP: a match is at most 258 long
      src = rel / PL_LANE;
      soff = rel % PL_LANE;
      send = (t + 1) * PL_STEP;
    }
    uint32_t a = lane == src ? soff : 0u;  // the offset the lane's walk assumed
    uint32_t path = 0, ex = PL_LANE;
    lane_walk(row, mm, a, 0u, path, ex);
    path &= vm;
    // 3. entries across lanes
    bool on = false;
    uint32_t nxt = 64;
    for (int round = 0; round <= 64; ++round) {  // (settled after at most 64; the bound is never the exit)
      nxt = pos0 + ex < send ? lane + ex / PL_LANE : 64u;  // the lane the exit lies in
      if (__ballot(nxt != lane + 1 && sl != LP - 1) == 0) {
        // every exit lies in the next lane (a sequence's last lane has none):
        // the lists are the sequences' lanes from their entry lane on
        on = lane >= src;
      } else {
        uint32_t ptr = nxt;
        uint64_t reach = 1ull << lane;
        for (int rnd = 0; rnd < 6 && __ballot(ptr < 64); ++rnd) {
          const bool in = ptr < 64;
          const int from = in ? (int)ptr : (int)lane;
          const uint32_t rlo = (uint32_t)__shfl((int)(uint32_t)reach, from, 64);
          const uint32_t rhi = (uint32_t)__shfl((int)(uint32_t)(reach >> 32), from, 64);
          const uint32_t nptr = (uint32_t)__shfl((int)ptr, from, 64);
          if (in) {
            reach |= ((uint64_t)rhi << 32) | rlo;
            ptr = nptr;
          }
        }
        const uint32_t slo = (uint32_t)__shfl((int)(uint32_t)reach, (int)src, 64);
        const uint32_t shi = (uint32_t)__shfl((int)(uint32_t)(reach >> 32), (int)src, 64);
        on = (((((uint64_t)shi << 32) | slo) >> lane) & 1) != 0;
      }
      if (on && nxt < 64) st->ent[nxt] = (uint8_t)(ex % PL_LANE);
      wsync();
      const uint32_t te = lane == src ? soff : (uint32_t)st->ent[lane];
      const bool changed = on && te != a;
      wsync();
      if (!__ballot(changed)) break;
      bool moved = false;  // the walk left the lane elsewhere than before
      if (changed) {
        const uint32_t ex0 = ex;
        lane_walk(row, mm, te, path, path, ex);
        path &= vm;
        a = te;
        moved = ex != ex0;
      }
      // no exit moved: the lists, and so every entry, stay as they are
      if (!__ballot(moved)) break;
    }
    if (!on) path = 0;
    if (!PIECE) {
      // the one on-path lane whose exit leaves the step carries the entry on
      const uint64_t last = __ballot(on && nxt >= 64);
      const int ll = last ? __builtin_ctzll(last) : 0;
      entry = (uint32_t)__builtin_amdgcn_readlane((int)(pos0 + ex), ll);
    }
    // 4. tokens and histograms
    const uint32_t cnt = (uint32_t)__popc(path);
    uint32_t incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t v = (uint32_t)__shfl_up((int)incl, off, 64);
      if (lane >= (uint32_t)off) incl += v;
    }
    // (each lane stores its own tokens at its running offset; compacted in the
    // rows and copied out 64 in a row instead: parse 1.211 -> 1.189 ms, not
    // kept, tools/experiments/parse_lanes_staged_stores.patch)
    uint32_t idx = ntok + incl - cnt;
    for (uint32_t q = path; q; q &= q - 1) {
      const uint32_t r = row[__builtin_ctz(q)];
      const uint32_t L = res_len(r);
      const bool mt = L >= 3;
      const uint32_t token = mt ? (L << 16) | res_dist(r) : res_byte(r);
      lds_inc(&s->lit_hist[mt ? 257 + len_sym(L) : token]);
      if (mt) {
        uint32_t eb, ev;
        lds_inc(&s->dist_hist[dist_sym(res_dist(r), eb, ev)]);
      }
      if (WRITE) r_blk[idx++] = token;
    }
    ntok += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  }
  return ntok;
}

// ================================ 1b. optparse_kernel ================================
// Cost-based parse of one 32 KiB block per wavefront (levels with opt = 1).
// price_kernel: the greedy parse of the block gives symbol statistics; their
// entropy gives a price per literal, length and distance symbol (1/8 bit
// units, <= 15 bits per symbol).  optparse_kernel: each lane runs a backward
// shortest-path DP over its own 512-position segment (plus OP_OV = 64
// positions of the next segment, where paths have converged): C[i] =
// min(lit(i) + C[i+1], min_l len(l) + dist(D_i) + C[i+l]) over l in
// 3..min(L_i, OP_SHORT) and l = L_i, for the longest match
// (L_i, D_i) the match kernel found at i.  The chosen length is written over
// res[i] (0 = literal), so the block kernel's parse follows the DP's path.
// Every value left in res is a valid (shorter or equal) match, so the stream
// stays correct whatever the cost model says.
// C is kept modulo 2^16 in an OP_RING-row LDS ring per lane (row = step mod OP_RING,
// all lanes on the same row at the same step, so reads of one length l hit
// distinct banks): differences over <= 258 positions stay below 2^15.
typedef unsigned int op_u32x4 __attribute__((ext_vector_type(4)));
constexpr int OP_SEG = DF_BLOCK / 64;  // one segment per lane
#ifndef ZT_OP_OV
#define ZT_OP_OV 64  // 128 / 96 / 64 / 32: post-match 7.64 / 7.50 / 7.42 / 7.28 ms per GiB, worst ratio window 1.0179 / 1.0180 / 1.0182 / 1.0195 (tools/gpu_r04ov.sh)
#endif
constexpr int OP_OV = ZT_OP_OV;  // positions of the next segment each lane's DP runs over (paths converge)
// C ring rows: C[i + l] for l <= OP_RING.  A longer match reads C[i + OP_RING]
// instead of C[i + L] (an estimate of its continuation: the parse stays
// valid, only the DP's cost model is approximate there); 64 rows keep the
// LDS at 8.5 KiB (round 2, 16-position groups: 80 rows / 4 groups, 3 waves
// per SIMD, 2.83 ms against 2.73 at 64 / 3 and 4 waves,
// profiles/r02q_optparse_variants.txt; bench ratio unchanged to 5 digits;
// 260 rows: 1 wave per SIMD)
#ifndef ZT_OP_RING
#define ZT_OP_RING 64
#endif
constexpr int OP_RING = ZT_OP_RING;
#ifndef ZT_OP_SHORT
#define ZT_OP_SHORT 24  // 8..14 / 16 / 18 / 20: worst ratio window 1.042..1.026 / 1.0182 / 1.0153 / 1.0144 at chain 28; at chain 20: 20 / 24 / 28 1.0207 / 1.0190 / 1.0188 -- the headroom spent on level 6's chain 28 -> 20 (profiles/r04os_sweep.txt)
#endif
constexpr int OP_SHORT = ZT_OP_SHORT;  // every cut length 3..OP_SHORT is tried (even), longer ones only at L
static_assert(OP_SHORT % 2 == 0 && OP_SHORT >= 4, "cut lengths go in pairs");
#ifndef ZT_OP_PF
#define ZT_OP_PF 1
#endif
constexpr int OP_PF = ZT_OP_PF;
constexpr int OP_G = 32;  // positions per group (one 128-byte line of res)

// prices of one block, in 1/8 bits (price_kernel -> optparse_kernel), kept at
// the start of the block's slot until block_kernel writes its header there
struct BlockPrices {
  uint8_t litc[256];
  uint8_t lenc[260];  // by match length (3..258), extra bits included
  uint8_t distc[32];  // by distance symbol, extra bits included
  uint32_t any_match;
};

struct PriceShared {
  uint32_t lit_hist[288];
  uint32_t dist_hist[32];
  LaneStage stage;
};

__device__ __forceinline__ uint32_t op_price(uint32_t f, float inv_total) {
  // -log2((f + 0.5) / total) in 1/8 bits, clamped to [1, 15] bits
  float b = -__log2f(((float)f + 0.5f) * inv_total) * 8.0f;
  int c = (int)(b + 0.5f);
  return (uint32_t)(c < 8 ? 8 : c > 120 ? 120 : c);
}

// price sample: 1/ZT_PRICE_SAMPLE of each block in ZT_PRICE_PIECES pieces
// spread over it.  The block's first 1/4 (sample 4, one piece) -> 1/8 in eight
// 512-position pieces: price 0.55 -> 0.30 ms per GiB, streams smaller at
// levels 6 and 9 (bench corpus at 128 MiB 0.53382 -> 0.53379), gate worst
// 1.0193 -> 1.0191.  1/4 in 4 pieces: price unchanged, gate 1.0193; 1/8 in 4:
// 0.29 ms, 1.0192; 1/16 in 4: 0.16 ms, 1.0197 (variants abS4, abS8, abC,
// abS16, abS8p8 of the round 6 post-match micro-variants,
// tools/experiments/README.md)
#ifndef ZT_PRICE_SAMPLE
#define ZT_PRICE_SAMPLE 8
#endif
#ifndef ZT_PRICE_PIECES
#define ZT_PRICE_PIECES 8
#endif
// greedy parse statistics -> prices (one wave per block, small LDS: many waves per CU)
__global__ __launch_bounds__(64) void price_kernel(DeflateParams P) {
  __shared__ PriceShared sh;
  PriceShared *s = &sh;
  const int lane = threadIdx.x;
  const uint32_t blk = blockIdx.x;
  if (P.store && P.store[blk]) return;  // stored block (classify_kernel)
  const uint64_t lo = (uint64_t)blk * DF_BLOCK;
  const uint64_t n = stream_end(P, blk);
  const uint32_t blen = (uint32_t)((n - lo) < DF_BLOCK ? (n - lo) : DF_BLOCK);
  for (int i = lane; i < 288; i += 64) s->lit_hist[i] = 0;
  if (lane < 32) s->dist_hist[lane] = 0;
  wsync();
  // the prices only need symbol statistics: a greedy parse of 1/ZT_PRICE_SAMPLE
  // of the block estimates them (a short block: its start, or all of it)
  const uint32_t plen = blen < (uint32_t)(DF_BLOCK / ZT_PRICE_SAMPLE) ? blen : (uint32_t)(DF_BLOCK / ZT_PRICE_SAMPLE);
  if (ZT_PRICE_PIECES > 1 && blen == DF_BLOCK) {
    // the sample in ZT_PRICE_PIECES pieces spread over the block, each parsed
    // greedily from its own start
    constexpr uint32_t pl = DF_BLOCK / ZT_PRICE_SAMPLE / ZT_PRICE_PIECES;
    if (P.parse_serial) {
      for (int j = 0; j < ZT_PRICE_PIECES; ++j)
        parse_block_regs<false>(s, P, P.res + lo + (uint64_t)j * (DF_BLOCK / ZT_PRICE_PIECES), pl);
    } else {
      // PL_STEP / pl pieces per step, pl / PL_LANE lanes each
      parse_block_lanes<false, (int)pl>(s, P, P.res + lo, 0u, ZT_PRICE_PIECES, DF_BLOCK / ZT_PRICE_PIECES);
    }
  } else if (P.parse_serial) {
    parse_block_regs<false>(s, P, P.res + lo, plen);
  } else {
    parse_block_lanes<false, 0>(s, P, P.res + lo, plen, 0u, 0u);
  }
  wsync();
  BlockPrices *bp = reinterpret_cast<BlockPrices *>(P.slots + (size_t)blk * DF_SLOT);
  float tl = 0.f, td = 0.f;
  for (int i = lane; i < 286; i += 64) tl += (float)s->lit_hist[i] + 0.5f;
  uint32_t dsum = lane < 30 ? s->dist_hist[lane] : 0u;
  if (lane < 30) td = (float)dsum + 0.5f;
  for (int off = 32; off; off >>= 1) {
    tl += __shfl_xor(tl, off, 64);
    td += __shfl_xor(td, off, 64);
    dsum += __shfl_xor(dsum, off, 64);
  }
  const float il = 1.0f / tl, id = 1.0f / td;
  for (int i = lane; i < 256; i += 64) bp->litc[i] = (uint8_t)op_price(s->lit_hist[i], il);
  if (lane < 32) bp->distc[lane] = lane < 30 ? (uint8_t)(op_price(s->dist_hist[lane], id) + 8 * dist_extra(lane)) : 255;
  for (int l = lane; l < 260; l += 64) {
    uint8_t v = 255;
    if (l >= 3 && l <= 258) {
      const uint32_t ls = len_sym(l);
      v = (uint8_t)(op_price(s->lit_hist[257 + ls], il) + 8 * len_extra(ls));
    }
    bp->lenc[l] = v;
  }
  if (lane == 0) bp->any_match = dsum;
}

struct OptShared {
  BlockPrices pr;
  uint16_t ring[OP_RING][64];
};

__device__ __forceinline__ uint32_t op_min3(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

#ifndef ZT_OP_MINW
#define ZT_OP_MINW 3  // waves per SIMD the register budget must allow (168 VGPRs: cut lengths to 24 take 138; at 4 waves, 128 VGPRs, 20 and more spill: optparse +0.1 ms)
#endif
__global__ __launch_bounds__(64, ZT_OP_MINW) void optparse_kernel(DeflateParams P) {
  __shared__ OptShared sh;
  OptShared *s = &sh;
  const int lane = threadIdx.x;
  const uint32_t blk = blockIdx.x;
  if (P.store && P.store[blk]) return;  // stored block (classify_kernel)
  const uint64_t lo = (uint64_t)blk * DF_BLOCK;
  const uint64_t n = stream_end(P, blk);
  const uint32_t blen = (uint32_t)((n - lo) < DF_BLOCK ? (n - lo) : DF_BLOCK);
  uint32_t *r_blk = P.res + lo;
  const BlockPrices *bp = reinterpret_cast<const BlockPrices *>(P.slots + (size_t)blk * DF_SLOT);
  if (bp->any_match == 0) return;  // no match anywhere: the greedy parse is all literals already
  {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(bp);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&s->pr);
    for (int i = lane; i < (int)(sizeof(BlockPrices) / 4); i += 64) dst[i] = src[i];
    uint32_t *rw = reinterpret_cast<uint32_t *>(&s->ring[0][0]);
    for (int i = lane; i < OP_RING * 32; i += 64) rw[i] = 0;
  }
  wsync();
  uint32_t lk[OP_SHORT + 1];  // price << 9 | l of the cut lengths (wave-uniform, SGPRs)
#pragma unroll
  for (int l = 3; l <= OP_SHORT; ++l)
    lk[l] = (uint32_t)__builtin_amdgcn_readfirstlane((int)(((uint32_t)s->pr.lenc[l] << 9) | (uint32_t)l));
  // backward DP, one segment per lane
  const uint32_t s0 = (uint32_t)lane * OP_SEG;
  if (s0 < blen) {
    const uint32_t seg_end = s0 + OP_SEG < blen ? s0 + OP_SEG : blen;
    const uint32_t e = seg_end + OP_OV < blen ? seg_end + OP_OV : blen;
    uint32_t C1 = 0;   // C[i + 1]
    uint32_t row = 0;  // step mod OP_RING
    uint32_t cr9[OP_SHORT + 1];  // cr9[l] = C[i + l] << 9 (0 past the segment's end)
#pragma unroll
    for (int l = 0; l <= OP_SHORT; ++l) cr9[l] = 0;
    const uint32_t g_last = (e - 1) & ~uint32_t(OP_G - 1);
    const uint32_t ngroups = (g_last - s0) / OP_G + 1;
    // a group is OP_G = 32 positions: one whole 128-byte line of res per
    // lane (the literal's byte rides in res), so the 64 lanes' scattered
    // reads each use the full line they fetch (16-position groups read half
    // lines + 16 data bytes: 13.4 GB of reads per GiB, profiles/r04pmc_*)
    auto load_g = [&](uint32_t g, op_u32x4 *r4) {
      const op_u32x4 *src = reinterpret_cast<const op_u32x4 *>(r_blk + g);
#pragma unroll
      for (int q = 0; q < OP_G / 4; ++q) r4[q] = src[q];
    };
    // OP_PF groups in flight per lane: HBM latency is hidden by depth
    op_u32x4 rq[OP_PF][OP_G / 4];
#pragma unroll
    for (int j = 0; j < OP_PF; ++j)
      if ((uint32_t)j < ngroups) load_g(g_last - (uint32_t)OP_G * (uint32_t)j, rq[j]);
    uint32_t gi = 0;  // groups done
    while (gi < ngroups) {
#pragma unroll
      for (int j = 0; j < OP_PF; ++j) {
        if (gi < ngroups) {
          const uint32_t g = g_last - (uint32_t)OP_G * gi;
          op_u32x4 rv[OP_G / 4];
#pragma unroll
          for (int q = 0; q < OP_G / 4; ++q) rv[q] = rq[j][q];
          if (gi + OP_PF < ngroups) load_g(g - (uint32_t)OP_G * OP_PF, rq[j]);
#pragma unroll
          for (int k = OP_G - 1; k >= 0; --k) {
            // positions >= e (the tail of the block's last group) are steps
            // with price 0 and no match: C stays 0 there, as past the end
            const uint32_t i = g + (uint32_t)k;
            const bool live = i < e;
            {
              const uint32_t r = rv[k >> 2][k & 3];
              const uint32_t L = live ? res_len(r) : 0u, D = res_dist(r);
              // C[i+1 .. i+OP_SHORT] live in registers (cr[1..]); only the
              // full-length candidate reads the LDS ring.  Candidates are
              // compared as keys (price relative to C[i+1], biased) << 9 | l.
              uint32_t eb, ev;
              const uint32_t Dc = D ? D : 1u;
              const int dc = (int)s->pr.distc[dist_sym(Dc, eb, ev)];
              const uint32_t Lc = L < 3 ? 3u : L;
              const uint32_t Lr = Lc < (uint32_t)OP_RING ? Lc : (uint32_t)OP_RING;
              const uint32_t rr = row >= Lr ? row - Lr : row + OP_RING - Lr;
              const int c_far = (int)(int16_t)(uint16_t)(s->ring[rr][lane] - (uint16_t)C1) + (int)s->pr.lenc[Lc];
              const int lit = live ? (int)s->pr.litc[res_byte(r)] : 0;
              uint32_t key = (uint32_t)(lit + 0x8000) << 9;
              // key of length l: (price + C[i+l] - C[i+1] + bias) << 9 | l,
              // one add3 of pre-shifted terms (exact modulo 2^32: the
              // unshifted value is below 2^23)
              const uint32_t base9 = (uint32_t)(dc + 0x8000 - (int)C1) << 9;
              // a pair of cut lengths enters when both are valid (one compare
              // and one select per pair: optparse 2.63 -> 2.41 ms per GiB with
              // two selects under one compare, r05au); the odd length L
              // itself, whose pair does not, is the full-length candidate
              // below, taken for every match (the same key: C[i + L] from the
              // ring)
#pragma unroll
              for (uint32_t l = 3; l < OP_SHORT; l += 2) {
                const uint32_t ka = base9 + cr9[l] + lk[l], kb = base9 + cr9[l + 1] + lk[l + 1];
                const uint32_t m = op_min3(key, ka, kb);
                key = l + 1 <= L ? m : key;
              }
              {
                const uint32_t kl = ((uint32_t)(dc + 0x8000 + c_far) << 9) | (Lc & 511);
                key = (L >= 3 && kl < key) ? kl : key;
              }
              const uint32_t choice = key & 511;
              const int best = (int)(key >> 9) - 0x8000;
              C1 += (uint32_t)best;
              s->ring[row][lane] = (uint16_t)C1;
              row = row + 1 == OP_RING ? 0 : row + 1;
#pragma unroll
              for (int l = OP_SHORT; l > 1; --l) cr9[l] = cr9[l - 1];
              cr9[1] = C1 << 9;
              rv[k >> 2][k & 3] = (r & 0xFF000000u) | (choice << 15) | D;
            }
          }
          // the group's choices in whole-line stores (positions >= seg_end
          // belong to the next lane; a group straddles seg_end only at the
          // block's end, where the positions past blen are never read)
          if (g < seg_end) {
            op_u32x4 *dst = reinterpret_cast<op_u32x4 *>(r_blk + g);
#pragma unroll
            for (int q = 0; q < OP_G / 4; ++q) dst[q] = rv[q];
          }
          ++gi;
        }
      }
    }
  }
}

// parse of one block per wave (the DP's path, or the greedy / lazy parse):
// tokens written over res, literal / length and distance histograms and the
// token count handed to block_kernel through the start of the block's slot
// (its prices are consumed by then; block_kernel writes the header there only
// after reading them).  A kernel of its own so that its LDS (histograms + the
// lane rows, 9.6 KiB) keeps 16 waves per CU, instead of block_kernel's 15
// (its Huffman scratch, 10.3 KiB).  P.parse_serial (ZT_PARSE_SERIAL=1) takes
// the serial window walk instead: the same tokens and histograms.
__global__ __launch_bounds__(64) void parse_kernel(DeflateParams P) {
  __shared__ PriceShared sh;
  PriceShared *s = &sh;
  const int lane = threadIdx.x;
  const uint32_t blk = blockIdx.x;
  if (P.store && P.store[blk]) return;  // stored block (classify_kernel)
  const uint64_t lo = (uint64_t)blk * DF_BLOCK;
  const uint64_t n = stream_end(P, blk);
  const uint32_t blen = (uint32_t)((n - lo) < DF_BLOCK ? (n - lo) : DF_BLOCK);
  for (int i = lane; i < 288; i += 64) s->lit_hist[i] = 0;
  if (lane < 32) s->dist_hist[lane] = 0;
  wsync();
  const uint32_t ntok = P.parse_serial ? parse_block_regs<true>(s, P, P.res + lo, blen)
                                       : parse_block_lanes<true, 0>(s, P, P.res + lo, blen, 0u, 0u);
  wsync();
  uint32_t *hs = reinterpret_cast<uint32_t *>(P.slots + (size_t)blk * DF_SLOT);
  for (int i = lane; i < 288; i += 64) hs[i] = s->lit_hist[i];
  if (lane < 32) hs[288 + lane] = s->dist_hist[lane];
  if (lane == 0) hs[320] = ntok;
}

// one wave per DEFLATE block: launched per parse block, the group's leader
// works, the others return
__global__ __launch_bounds__(64) void block_kernel(DeflateParams P) {
  __shared__ BlockShared sh;
  BlockShared *s = &sh;
  const int lane = threadIdx.x;
  const uint32_t blk = blockIdx.x;
  if (!group_leader(P, blk)) return;
  const uint32_t nsub = group_size(P, blk);
  const uint64_t lo = (uint64_t)blk * DF_BLOCK;
  const uint64_t n = stream_end(P, blk);
  const uint64_t gspan = (uint64_t)nsub * DF_BLOCK;
  const uint32_t blen = (uint32_t)((n - lo) < gspan ? (n - lo) : gspan);
  BlockPlan *plan = P.plans + blk;
  const bool last = P.span ? lo + gspan >= n : P.final_ && (blk + nsub == P.nblocks);
  if (P.store && P.store[blk]) {  // classify_kernel: bytes that cannot beat a stored block
    if (lane == 0) P.slot_len[blk] = blen + 5 * ((blen + 65534) / 65535) + 5;
    if (lane > 0 && (uint32_t)lane < nsub) P.slot_len[blk + lane] = 0;
    if (lane == 0) {
      plan->ntok = 0;
      plan->btype = 0;
      plan->hdr_bits = 0;
      plan->hdr_tail = 0;
      plan->blen = blen;
      plan->last = last ? 1 : 0;
      plan->nsub = nsub;
    }
    return;
  }
  // the parse's histograms and token counts (parse_kernel, in each parse
  // block's slot), summed over the group
  uint32_t ntok = 0;
  for (uint32_t k = 0; k < nsub; ++k) {
    const uint32_t *hs = reinterpret_cast<const uint32_t *>(P.slots + (size_t)(blk + k) * DF_SLOT);
    for (int i = lane; i < 288; i += 64) s->lit_hist[i] = (k ? s->lit_hist[i] : 0u) + hs[i];
    if (lane < 32) s->dist_hist[lane] = (k ? s->dist_hist[lane] : 0u) + hs[288 + lane];
    const uint32_t nt = hs[320];
    if (lane == 0) plan->ntok_sub[k] = nt;
    ntok += nt;
  }
  wsync();
#ifdef ZT_DF_TIME
  uint64_t bt0 = __builtin_readcyclecounter(), btk;
#define BK_T(k)                                                                          \
  btk = __builtin_readcyclecounter();                                                    \
  if (lane == 0) atomicAdd(&g_bk_time[k], (unsigned long long)(btk - bt0));              \
  bt0 = btk;
#else
#define BK_T(k) (void)0
#endif
  BK_T(0);
  wsync();
  if (lane == 0) s->lit_hist[256] += 1;  // end of block
  wsync();
  huff_lengths(s, s->lit_hist, 286, 15, s->lit_len);
  huff_lengths(s, s->dist_hist, 30, 15, s->dist_len);
  BK_T(1);
  {
    // trailing zero lengths trimmed (RFC 1951 3.2.7: HLIT >= 257, HDIST >= 1)
    uint32_t hi_lit = 0;
    for (int c = 0; c < 5; ++c) {
      const int i = c * 64 + lane;
      const uint64_t nz = __ballot(i < 286 && s->lit_len[i] != 0);
      if (nz) hi_lit = (uint32_t)(c * 64 + 64 - __clzll(nz));
    }
    const uint64_t dnz = __ballot(lane < 30 && s->dist_len[lane] != 0);
    const uint32_t hlit = hi_lit > 257 ? hi_lit : 257;
    const uint32_t hdist = dnz ? (uint32_t)(64 - __clzll(dnz)) : 1u;
    const uint32_t total = hlit + hdist;
    if (lane < 19) s->cl_code[lane] = 0;  // CL symbol frequencies until the codes are built
    if (lane == 0) {
      s->hlit = hlit;
      s->hdist = hdist;
    }
    wsync();
    // RLE of the concatenated lengths, one lane per run: runs start where the
    // value changes; each run's symbols are counted, placed by a scan, then
    // written by its lane
    auto val = [&](uint32_t i) -> uint32_t { return i < hlit ? s->lit_len[i] : s->dist_len[i - hlit]; };
    uint64_t starts[5];
    for (int c = 0; c < 5; ++c) {
      const uint32_t i = (uint32_t)(c * 64 + lane);
      starts[c] = __ballot(i < total && (i == 0 || val(i) != val(i - 1)));
    }
    uint32_t base = 0;
    for (int c = 0; c < 5; ++c) {
      const uint32_t i = (uint32_t)(c * 64 + lane);
      const bool st = (starts[c] >> lane) & 1;
      uint32_t v = 0, r = 0, cnt = 0;
      if (st) {
        // the run's end: the next start (or the end of the lengths)
        uint32_t e = total;
        const uint64_t rest = lane < 63 ? starts[c] & (~0ull << (lane + 1)) : 0ull;
        if (rest) {
          e = (uint32_t)(c * 64) + (uint32_t)__builtin_ctzll(rest);
        } else {
          for (int cc = c + 1; cc < 5; ++cc)
            if (starts[cc]) {
              e = (uint32_t)(cc * 64) + (uint32_t)__builtin_ctzll(starts[cc]);
              break;
            }
        }
        v = val(i);
        r = e - i;
        // symbol count of the run (the writer below, counting only)
        uint32_t q = r;
        if (v == 0) {
          while (q >= 11) {
            q -= q < 138 ? q : 138;
            ++cnt;
          }
          cnt += q >= 3 ? 1 : q;
        } else {
          cnt = 1;
          --q;
          while (q >= 3) {
            q -= q < 6 ? q : 6;
            ++cnt;
          }
          cnt += q;
        }
      }
      // exclusive scan of the counts
      uint32_t incl = cnt;
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, off, 64);
        if (lane >= off) incl += y;
      }
      uint32_t o = base + incl - cnt;
      base += (uint32_t)__shfl((int)incl, 63, 64);
      if (st) {
        uint32_t q = r;
        if (v == 0) {
          while (q >= 11) {
            const uint32_t x = q < 138 ? q : 138;
            s->cl_syms[o++] = (uint16_t)(18 | ((x - 11) << 5));
            atomicAdd(&s->cl_code[18], 1u);
            q -= x;
          }
          if (q >= 3) {
            s->cl_syms[o++] = (uint16_t)(17 | ((q - 3) << 5));
            atomicAdd(&s->cl_code[17], 1u);
          } else if (q) {
            atomicAdd(&s->cl_code[0], q);
            for (; q; --q) s->cl_syms[o++] = 0;
          }
        } else {
          s->cl_syms[o++] = (uint16_t)v;
          uint32_t nv = 1;
          --q;
          while (q >= 3) {
            const uint32_t x = q < 6 ? q : 6;
            s->cl_syms[o++] = (uint16_t)(16 | ((x - 3) << 5));
            atomicAdd(&s->cl_code[16], 1u);
            q -= x;
          }
          for (; q; --q, ++nv) s->cl_syms[o++] = (uint16_t)v;
          atomicAdd(&s->cl_code[v], nv);
        }
      }
    }
    if (lane == 0) s->n_cl_syms = base;
  }
  wsync();
  BK_T(2);
  huff_lengths(s, s->cl_code, 19, 7, s->cl_len);
  huff_codes(s->lit_len, 286, s->lit_code);
  huff_codes(s->dist_len, 30, s->dist_code);
  huff_codes(s->cl_len, 19, s->cl_code);
  BK_T(3);
  // sizes of the three choices (bits, without the sync marker)
  uint64_t dyn = 0, fix = 0;
  for (int i = lane; i < 286; i += 64) {
    uint32_t f = s->lit_hist[i];
    uint32_t extra = i >= 257 ? len_extra(i - 257) : 0;
    dyn += (uint64_t)f * (s->lit_len[i] + extra);
    fix += (uint64_t)f * ((fixed_lit(i) >> 16) + extra);
  }
  if (lane < 30) {
    uint32_t f = s->dist_hist[lane];
    uint32_t extra = dist_extra(lane);
    dyn += (uint64_t)f * (s->dist_len[lane] + extra);
    fix += (uint64_t)f * (5 + extra);
  }
  uint32_t hclen = 19;
  while (hclen > 4 && s->cl_len[kClOrder[hclen - 1]] == 0) --hclen;
  uint32_t hdr = 0;
  for (uint32_t k = lane; k < s->n_cl_syms; k += 64) {
    uint32_t c = s->cl_syms[k] & 31;
    hdr += s->cl_len[c] + (c == 16 ? 2 : c == 17 ? 3 : c == 18 ? 7 : 0);
  }
  for (int off = 32; off; off >>= 1) {
    dyn += __shfl_xor(dyn, off, 64);
    fix += __shfl_xor(fix, off, 64);
    hdr += __shfl_xor(hdr, off, 64);
  }
  hdr += 3 + 5 + 5 + 4 + 3 * hclen;
  dyn += hdr;
  fix += 3;
  // stored: the block's bytes + 5 header bytes; Huffman forms add the
  // 3-bit marker header, padding and the 4 sync bytes
  const uint64_t stored_bits = 8ull * (blen + 5 * ((blen + 65534) / 65535) + 5);  // + its sync point
  const uint64_t dyn_bits = ((dyn + 3 + 7) & ~7ull) + 32;
  const uint64_t fix_bits = ((fix + 3 + 7) & ~7ull) + 32;
  BK_T(4);
  uint32_t bt;
  if (P.ctype == 1) bt = 1;
  else if (stored_bits <= dyn_bits && stored_bits <= fix_bits) bt = 0;
  else bt = dyn_bits <= fix_bits ? 2 : 1;
  // the block's exact size: scan_sizes places it before it is encoded
  if (lane == 0) P.slot_len[blk] = (uint32_t)((bt == 0 ? stored_bits : bt == 1 ? fix_bits : dyn_bits) >> 3);
  if (lane > 0 && (uint32_t)lane < nsub) P.slot_len[blk + lane] = 0;
  // codes for the encoder
  for (int i = lane; i < 288; i += 64) plan->lit_code[i] = bt == 2 ? (i < 286 ? s->lit_code[i] : 0u) : fixed_lit(i);
  if (lane < 32) plan->dist_code[lane] = bt == 2 ? (lane < 30 ? s->dist_code[lane] : 0u)
                                                 : ((5u << 16) | (__brev((uint32_t)lane) >> 27));
  // the dynamic header, wave-parallel: every field an item (value, bits),
  // bit offsets by a scan, OR-ed into an LDS word buffer (the package-merge
  // list space, free now), complete words copied to the slot
  uint32_t hbits = 0, htail = 0;
  if (bt == 1) {
    hbits = 3;
    htail = 2;  // BFINAL=0, BTYPE=01
  } else if (bt == 2) {
    uint32_t *hw = s->huf.lst[0];
    for (int k = lane; k < 160; k += 64) hw[k] = 0;
    wsync();
    const uint32_t nsym = s->n_cl_syms, nitems = 1 + hclen + nsym;
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < nitems; c0 += 64) {
      const uint32_t it = c0 + (uint32_t)lane;
      uint32_t v = 0, nb = 0;
      if (it == 0) {
        v = 4u | ((s->hlit - 257) << 3) | ((s->hdist - 1) << 8) | ((hclen - 4) << 13);  // BTYPE=10, HLIT, HDIST, HCLEN
        nb = 17;
      } else if (it <= hclen) {
        v = s->cl_len[kClOrder[it - 1]];
        nb = 3;
      } else if (it < nitems) {
        const uint32_t cs = s->cl_syms[it - 1 - hclen], c = cs & 31;
        const uint32_t cc = s->cl_code[c], cl = cc >> 16;
        const uint32_t xb = c == 16 ? 2u : c == 17 ? 3u : c == 18 ? 7u : 0u;
        v = (cc & 0xFFFF) | ((cs >> 5) << cl);
        nb = cl + xb;
      }
      uint32_t incl = nb;
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, off, 64);
        if (lane >= off) incl += y;
      }
      const uint32_t o = base + incl - nb;
      base += (uint32_t)__shfl((int)incl, 63, 64);
      if (nb) {
        const uint32_t sh = o & 31;
        atomicOr(&hw[o >> 5], v << sh);
        if (sh + nb > 32) atomicOr(&hw[(o >> 5) + 1], v >> (32 - sh));
      }
    }
    wsync();
    hbits = base;
    uint32_t *slot = reinterpret_cast<uint32_t *>(P.slots + (size_t)blk * DF_SLOT);
    for (uint32_t k = lane; k < (hbits >> 5); k += 64) slot[k] = hw[k];
    htail = hw[hbits >> 5] & ((hbits & 31) ? ((1u << (hbits & 31)) - 1) : 0u);
  }
  if (lane == 0) {
    plan->ntok = ntok;
    plan->btype = bt;
    plan->hdr_bits = hbits;
    plan->hdr_tail = htail;
    plan->blen = blen;
    plan->last = last ? 1 : 0;
    plan->nsub = nsub;
  }
  BK_T(5);
#ifdef ZT_DF_TIME
  if (lane == 0) atomicAdd(&g_bk_time[6], 1ull);
#endif
#undef BK_T
}

// ================================ 3. encode_kernel ================================
#ifndef ZT_ENC_LDS
#define ZT_ENC_LDS 1  // block words staged in LDS, then written out coalesced
#endif
#ifndef ZT_ENC_CACHE
#define ZT_ENC_CACHE (ZT_DF_GROUP == 1)  // a thread's first tokens kept in registers between the two passes
#endif
#ifndef ZT_ENC_NCACHE
#define ZT_ENC_NCACHE 32  // 16 / 32 / 48 / 64: encode 1.19 / 1.10 / 1.16 / 1.55 ms per GiB; L2 read requests 1.96 -> 1.16 GB (the second pass's re-reads missed L2; tools/gpu_r04ec*.sh)
#endif
constexpr int ENC_CACHE = ZT_ENC_NCACHE;  // tokens per thread kept (a multiple of 4)
// a dynamic block is never planned larger than its stored form
// (block_kernel); a fixed-code block (compressionType FIXED) may take 9 bits
// per byte: 36 KiB + header and marker
constexpr uint32_t ENC_OBUF_WORDS = (ZT_ENC_LDS ? (DF_GROUP * DF_BLOCK / 8 * 9 + 64) / 4 + 64 : 1);
struct EncShared {
  uint32_t lit_code[288];
  uint32_t dist_code[32];
  uint32_t start[ENC_THREADS + 1];  // exclusive prefix of per-thread bit counts
  uint32_t first_val[ENC_THREADS];  // contribution to the (partial) first word
  uint32_t wsum[ENC_THREADS / 64];
  uint32_t obuf[ENC_OBUF_WORDS];    // the block's words (ZT_ENC_LDS)
};

// a block's words in the stream: dst = the aligned word holding its first
// byte; words 0 and `wlast` are shared with the neighbouring blocks (or the
// restart marker), so only the block's own bytes [lo, hi) of them are stored.
// ZT_ENC_LDS: every word goes to the LDS buffer first -- each thread packs its
// own few words, so direct stores left most lines of the stream partially
// written per instruction (encode_kernel wrote 1.47 GB per GiB for 0.57 GB of
// stream, profiles/r04k_pmc_traffic.txt) -- and flush() writes them out
// coalesced.
struct BlockWords {
  uint8_t *dst;
  uint32_t wlast, lo, hi;
  uint32_t *obuf;
  __device__ __forceinline__ void store_global(uint32_t w, uint32_t v) const {
    if (w != 0 && w != wlast) {
      reinterpret_cast<uint32_t *>(dst)[w] = v;
      return;
    }
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) {
      const uint32_t x = 4 * w + b;
      if (x >= lo && x < hi) dst[x] = (uint8_t)(v >> (8 * b));
    }
  }
  __device__ __forceinline__ void store(uint32_t w, uint32_t v) const {
    if (ZT_ENC_LDS)
      obuf[w] = v;
    else
      store_global(w, v);
  }
  // after a workgroup barrier: words [0, wlast] from the LDS buffer
  __device__ __forceinline__ void flush(uint32_t t) const {
    if (!ZT_ENC_LDS) return;
    for (uint32_t w = t; w <= wlast; w += ENC_THREADS) store_global(w, obuf[w]);
  }
};

// bit accumulator writing aligned 32-bit words of one block
struct BitOut {
  uint64_t acc;
  uint32_t nacc;      // valid bits in acc (acc bit 0 = bit `word * 32` of the block's words)
  uint32_t word;      // index of the word acc starts at
  uint32_t first;     // first word index of this thread's range
  BlockWords slot;
  uint32_t first_val;
  bool first_partial;
  bool wrote_first;

  __device__ void init(uint32_t start_bit, const BlockWords &sl) {
    slot = sl;
    word = start_bit >> 5;
    first = word;
    nacc = start_bit & 31;
    acc = 0;
    first_partial = nacc != 0;
    wrote_first = false;
    first_val = 0;
  }
  __device__ __forceinline__ void put(uint32_t v, uint32_t n) {
    acc |= (uint64_t)v << nacc;
    nacc += n;
    if (nacc >= 32) {
      uint32_t w = (uint32_t)acc;
      if (word == first && first_partial) {
        first_val = w;
        wrote_first = true;
      } else {
        slot.store(word, w);
      }
      ++word;
      acc >>= 32;
      nacc -= 32;
    }
  }
};

__device__ __forceinline__ uint32_t token_bits(const EncShared *s, uint32_t tk) {
  if (tk < 256) return s->lit_code[tk] >> 16;
  const uint32_t L = tk >> 16, D = tk & 0xFFFF;
  const uint32_t ls = len_sym(L);
  uint32_t eb, ev;
  const uint32_t ds = dist_sym(D, eb, ev);
  return (s->lit_code[257 + ls] >> 16) + len_extra(ls) + (s->dist_code[ds] >> 16) + eb;
}

__device__ __forceinline__ void put_token(BitOut &bo, const EncShared *s, uint32_t tk) {
  if (tk < 256) {
    const uint32_t c = s->lit_code[tk];
    bo.put(c & 0xFFFF, c >> 16);
    return;
  }
  const uint32_t L = tk >> 16, D = tk & 0xFFFF;
  const uint32_t ls = len_sym(L);
  const uint32_t c = s->lit_code[257 + ls];
  bo.put(c & 0xFFFF, c >> 16);
  const uint32_t lx = len_extra(ls);
  if (lx) bo.put(L - len_base(ls), lx);
  uint32_t eb, ev;
  const uint32_t ds = dist_sym(D, eb, ev);
  const uint32_t dc = s->dist_code[ds];
  bo.put(dc & 0xFFFF, dc >> 16);
  if (eb) bo.put(ev, eb);
}

// f(token) for tokens [a, b) of this thread, read 64 bytes at a time (four
// 16-byte loads issued together): a thread's range is contiguous, so the
// lanes of a wave touch 64 different lines per load and one 4-byte load per
// token would fetch every line many times over
template <typename F>
__device__ __forceinline__ void for_tokens(const uint32_t *tok, uint32_t a, uint32_t b, F &&f) {
  typedef unsigned int u32x4t __attribute__((ext_vector_type(4)));
  uint32_t i = a;
  for (; i < b && (i & 3); ++i) f(tok[i]);
  for (; i + 16 <= b; i += 16) {
    const u32x4t *v = reinterpret_cast<const u32x4t *>(tok + i);
    const u32x4t x0 = v[0], x1 = v[1], x2 = v[2], x3 = v[3];
    f(x0.x); f(x0.y); f(x0.z); f(x0.w);
    f(x1.x); f(x1.y); f(x1.z); f(x1.w);
    f(x2.x); f(x2.y); f(x2.z); f(x2.w);
    f(x3.x); f(x3.y); f(x3.z); f(x3.w);
  }
  for (; i + 4 <= b; i += 4) {
    const u32x4t x = *reinterpret_cast<const u32x4t *>(tok + i);
    f(x.x); f(x.y); f(x.z); f(x.w);
  }
  for (; i < b; ++i) f(tok[i]);
}

// f(token) for tokens [a, b) of the group's concatenated token lists
template <typename F>
__device__ __forceinline__ void for_group_tokens(const DeflateParams &P, const BlockPlan *plan, uint32_t blk,
                                                 uint32_t a, uint32_t b, F &&f) {
  uint32_t off = 0;
  for (uint32_t k = 0; k < plan->nsub && off < b; ++k) {
    const uint32_t nk = plan->ntok_sub[k];
    const uint32_t lo = a > off ? a - off : 0u, hi = b - off < nk ? b - off : nk;
    if (lo < hi) for_tokens(P.res + (uint64_t)(blk + k) * DF_BLOCK, lo, hi, f);
    off += nk;
  }
}

// bytes [src, src + n) to [dst, dst + n) by the workgroup: dst-aligned words,
// each from two aligned source words (src may be unaligned)
__device__ __forceinline__ void enc_copy(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t t) {
  const uint32_t h0 = (4u - (uint32_t)((uintptr_t)dst & 3)) & 3, h = h0 < n ? h0 : n;
  if (t < h) dst[t] = src[t];
  const uint32_t n4 = (n - h) / 4;
  const uint8_t *s8 = src + h;
  uint32_t *d4 = reinterpret_cast<uint32_t *>(dst + h);
  const uint32_t sh = (uint32_t)((uintptr_t)s8 & 3);
  const uint32_t *s4 = reinterpret_cast<const uint32_t *>(s8 - sh);
  const uint32_t nsrc = (sh + 4 * n4 + 3) / 4;  // source words holding bytes of the copy
  for (uint32_t w = t; w < n4; w += ENC_THREADS) {
    const uint32_t lo = s4[w], hi = sh && w + 1 < nsrc ? s4[w + 1] : 0u;
    d4[w] = sh ? __builtin_amdgcn_alignbyte(hi, lo, sh) : lo;
  }
  for (uint32_t i = h + 4 * n4 + t; i < n; i += ENC_THREADS) dst[i] = src[i];
}

// one workgroup per DEFLATE block (launched per parse block; followers
// return): the block goes straight to its place in the stream, out +
// boff[blk] (its size was planned exactly by block_kernel and placed by
// scan_sizes), followed by the restart marker where a segment ends
__global__ __launch_bounds__(ENC_THREADS) void encode_kernel(DeflateParams P) {
  __shared__ EncShared sh;
  EncShared *s = &sh;
  const uint32_t t = threadIdx.x;
  const uint32_t blk = blockIdx.x;
  if (!group_leader(P, blk)) return;
  const BlockPlan *plan = P.plans + blk;
  const uint32_t bt = plan->btype, blen = plan->blen;
  const bool last = plan->last != 0;
  const uint8_t *slot_bytes = P.slots + (size_t)blk * DF_SLOT;
  uint8_t *dst = P.out + P.boff[blk];
  const uint32_t plan_bytes = P.slot_len[blk];
  if (t < kRestartMarkerLen && restart_after(blk + plan->nsub - 1, P.nblocks, P.restart, P.final_, P.span))
    dst[plan_bytes + t] = (t % 5) < 3 ? 0 : 0xFF;  // 00 00 00 FF FF x 2
  if (bt == 0) {
    // stored block: header byte, LEN, NLEN, data
    const uint8_t *raw = P.base + P.halo + (uint64_t)blk * DF_BLOCK;
    // followed, like every block, by an empty stored block (the sync point
    // inflate splits on), which carries BFINAL on the stream's last block
    // (pieces of at most 65535 bytes: a stored block's LEN is 16 bits)
    const uint32_t nparts = blen ? (blen + 65534) / 65535 : 1;
    if (t < nparts) {
      const uint32_t plen = blen - t * 65535 < 65535 ? blen - t * 65535 : 65535;
      uint8_t *h = dst + (size_t)t * (65535 + 5);
      h[0] = 0;
      h[1] = plen & 0xFF;
      h[2] = plen >> 8;
      h[3] = (~plen) & 0xFF;
      h[4] = ((~plen) >> 8) & 0xFF;
    }
    if (t == 0) {
      uint8_t *e = dst + 5 * nparts + blen;
      e[0] = last ? 1 : 0;
      e[1] = 0;
      e[2] = 0;
      e[3] = 0xFF;
      e[4] = 0xFF;
      if (blen + 5 * nparts + 5 != plan_bytes) atomicOr(P.fault, 1u);
    }
    for (uint32_t k = 0; k < nparts; ++k) {
      const uint32_t plen = blen - k * 65535 < 65535 ? blen - k * 65535 : 65535;
      enc_copy(dst + (size_t)k * (65535 + 5) + 5, raw + (size_t)k * 65535, plen, t);
    }
    return;
  }
  for (uint32_t i = t; i < 288; i += ENC_THREADS) s->lit_code[i] = plan->lit_code[i];
  if (t < 32) s->dist_code[t] = plan->dist_code[t];
  __syncthreads();
  const uint32_t ntok = plan->ntok;
  const uint32_t hdr_bits = plan->hdr_bits;
  const uint32_t a = (uint32_t)(((uint64_t)ntok * t) / ENC_THREADS);
  const uint32_t b = (uint32_t)(((uint64_t)ntok * (t + 1)) / ENC_THREADS);
  uint32_t bits = 0;
  const uint32_t *tok = P.res + (uint64_t)blk * DF_BLOCK;  // (DF_GROUP 1: the block's own tokens)
#if ZT_ENC_CACHE
  // the thread's first ENC_CACHE tokens stay in registers for the packing
  // pass (5 aligned 16-byte loads, then a shift by a % 4): only the rest is
  // read twice
  typedef unsigned int u32x4e __attribute__((ext_vector_type(4)));
  const uint32_t nc = b - a < (uint32_t)ENC_CACHE ? b - a : (uint32_t)ENC_CACHE;
  uint32_t cache[ENC_CACHE];
  {
    uint32_t raw[ENC_CACHE + 4];
    const u32x4e *v = reinterpret_cast<const u32x4e *>(tok + (a & ~3u));
#pragma unroll
    for (int q = 0; q < ENC_CACHE / 4 + 1; ++q) {
      const u32x4e x = (4 * q < (int)((a & 3) + nc)) ? v[q] : u32x4e{0, 0, 0, 0};
      raw[4 * q] = x.x;
      raw[4 * q + 1] = x.y;
      raw[4 * q + 2] = x.z;
      raw[4 * q + 3] = x.w;
    }
    const uint32_t sh = a & 3;
#pragma unroll
    for (int j = 0; j < ENC_CACHE; ++j)
      cache[j] = sh == 0 ? raw[j] : sh == 1 ? raw[j + 1] : sh == 2 ? raw[j + 2] : raw[j + 3];
  }
#pragma unroll
  for (int j = 0; j < ENC_CACHE; ++j)
    if ((uint32_t)j < nc) bits += token_bits(s, cache[j]);
  for_tokens(tok, a + nc, b, [&](uint32_t tk) { bits += token_bits(s, tk); });
#else
  if constexpr (DF_GROUP == 1)
    for_tokens(tok, a, b, [&](uint32_t tk) { bits += token_bits(s, tk); });
  else
    for_group_tokens(P, plan, blk, a, b, [&](uint32_t tk) { bits += token_bits(s, tk); });
#endif
  if (t == 0) bits += hdr_bits;
  const uint32_t eob = s->lit_code[256] >> 16;
  if (t == ENC_THREADS - 1) bits += eob;  // marker bits appended after the scan
  {
    const int lane = t & 63, wave = t >> 6;
    uint32_t x = bits;
    for (int off = 1; off < 64; off <<= 1) {
      uint32_t y = __shfl_up(x, off, 64);
      if (lane >= off) x += y;
    }
    if (lane == 63) s->wsum[wave] = x;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wave; ++w) before += s->wsum[w];
    const uint32_t incl = x + before;
    s->start[t] = incl - bits;
    if (t == ENC_THREADS - 1) s->start[ENC_THREADS] = incl;
  }
  __syncthreads();
  // bit positions from here on count from the aligned word holding the
  // block's first byte: B0 bits of it belong to the previous block
  const uint32_t B0 = 8u * (uint32_t)((uintptr_t)dst & 3);
  const uint32_t total_end = s->start[ENC_THREADS];
  // marker: 3-bit stored header (BFINAL on the stream's last block), pad, 00 00 FF FF
  const uint32_t after = total_end + 3;
  const uint32_t padded = (after + 7) & ~7u;
  const uint32_t block_end = padded + 32;
  if (t == 0 && (block_end >> 3) != plan_bytes) atomicOr(P.fault, 1u);
  BlockWords bw;
  bw.dst = dst - (B0 >> 3);
  bw.lo = B0 >> 3;
  bw.hi = (B0 + block_end) >> 3;
  bw.wlast = (B0 + block_end - 1) >> 5;
  bw.obuf = s->obuf;
  if (ZT_ENC_LDS && bw.wlast >= ENC_OBUF_WORDS) {  // (cannot happen: see ENC_OBUF_WORDS)
    if (t == 0) atomicOr(P.fault, 1u);
    return;
  }
  BitOut bo;
  // thread 0 starts at the header: its complete words come from the slot
  // (block_kernel), then its partial last word
  bo.init(B0 + (t == 0 ? 0u : s->start[t]), bw);
  if (t == 0) {
    bo.first_partial = false;  // word 0's other bytes are the previous block's: stored masked (BlockWords)
    const uint32_t *hw = reinterpret_cast<const uint32_t *>(slot_bytes);
    for (uint32_t k = 0; k < (hdr_bits >> 5); ++k) bo.put(hw[k], 32);
    if (hdr_bits & 31) bo.put(plan->hdr_tail, hdr_bits & 31);
  }
#if ZT_ENC_CACHE
#pragma unroll
  for (int j = 0; j < ENC_CACHE; ++j)
    if ((uint32_t)j < nc) put_token(bo, s, cache[j]);
  for_tokens(tok, a + nc, b, [&](uint32_t tk) { put_token(bo, s, tk); });
#else
  if constexpr (DF_GROUP == 1)
    for_tokens(tok, a, b, [&](uint32_t tk) { put_token(bo, s, tk); });
  else
    for_group_tokens(P, plan, blk, a, b, [&](uint32_t tk) { put_token(bo, s, tk); });
#endif
  if (t == ENC_THREADS - 1) {
    const uint32_t c = s->lit_code[256];
    bo.put(c & 0xFFFF, c >> 16);
    bo.put(last ? 1 : 0, 3);
    bo.put(0, padded - after);
    bo.put(0xFFFF0000u, 32);
  }
  // share the partial first word; the first thread touching a word writes it
  s->first_val[t] = bo.first_partial ? (bo.wrote_first ? bo.first_val : (uint32_t)bo.acc) : 0;
  __syncthreads();
  const bool have_tail = bo.nacc > 0 && !(bo.word == bo.first && bo.first_partial);
  if (have_tail) {
    // this thread started at or before the tail word's first bit: it owns it
    const uint32_t w = bo.word;
    uint32_t v = (uint32_t)bo.acc;
    for (uint32_t u = t + 1; u < ENC_THREADS; ++u) {
      const uint32_t us = B0 + s->start[u], ue = B0 + ((u == ENC_THREADS - 1) ? block_end : s->start[u + 1]);
      if (ue == us) continue;
      if ((us >> 5) != w) break;
      v |= s->first_val[u];
      if (ue >= (w + 1) * 32) break;
    }
    bw.store(w, v);
  }
  if (ZT_ENC_LDS) {
    __syncthreads();
    bw.flush(t);
  }
}

// ================================ 4. stitching ================================
// A restart point (segment boundary) is announced by two empty stored blocks
// after the preceding block (which always ends byte-aligned):
//   00 00 00 FF FF 00 00 00 FF FF
// An ordinary block boundary carries at most one, so the 10-byte pattern at a
// stored-block end marks a segment that inflate may decode on its own.
// (a non-final call -- a shard -- also ends with the marker: the next shard
// is independent when deflated with halo 0, see zt_shard.py).  The rule is
// restart_after (deflate_index_host.h: the deflate-time index shares it).

__global__ __launch_bounds__(1024) void scan_sizes(const uint32_t *__restrict__ len, uint32_t n,
                                                   uint64_t *__restrict__ off, uint64_t base, uint32_t restart,
                                                   int final_, const uint64_t *__restrict__ span) {
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (n + 1023) / 1024;
  const uint32_t a = t * per, b = (a + per) < n ? (a + per) : n;
  uint64_t sum = 0;
  for (uint32_t i = a; i < b; ++i) sum += len[i] + (restart_after(i, n, restart, final_, span) ? kRestartMarkerLen : 0);
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    uint64_t v = (int)t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint64_t run = base + part[t] - sum;
  for (uint32_t i = a; i < b; ++i) {
    off[i] = run;
    run += len[i] + (restart_after(i, n, restart, final_, span) ? kRestartMarkerLen : 0);
  }
  if (t == 1023) off[n] = base + part[1023];
}

// block_kernel's two Huffman device functions on histograms handed in
// (zt_debug_huffman): one wave per histogram, staged in LDS as block_kernel's
// own are
__global__ __launch_bounds__(64) void debug_huffman_kernel(const uint32_t *__restrict__ freq, uint32_t n,
                                                           uint32_t limit, uint8_t *__restrict__ lens,
                                                           uint32_t *__restrict__ codes) {
  __shared__ BlockShared sh;
  BlockShared *s = &sh;
  const uint32_t lane = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * n;
  for (uint32_t i = lane; i < 288; i += 64) s->lit_hist[i] = i < n ? freq[base + i] : 0u;
  wsync();
  huff_lengths(s, s->lit_hist, (int)n, (int)limit, s->lit_len);
  huff_codes(s->lit_len, (int)n, s->lit_code);
  for (uint32_t i = lane; i < n; i += 64) {
    lens[base + i] = s->lit_len[i];
    codes[base + i] = s->lit_code[i];
  }
}

}  // namespace

// huff_lengths + huff_codes on host histograms (zt_internal.h)
extern "C" int zt_debug_huffman(const uint32_t *freqs, uint32_t count, uint32_t n, uint32_t limit, uint8_t *lens,
                                uint32_t *codes) {
  if (!freqs || !lens || !codes || count == 0 || count > (1u << 20) || n < 2 || n > 286 ||
      (limit != 7 && limit != 15) || n > (1u << limit))
    return set_error(ZT_E_ARG, "zt_debug_huffman: bad argument");
  // the sort key is freq << 9 | symbol in 32 bits, and the package weights
  // (below 15 times a histogram's sum) are 32-bit sums
  for (uint32_t h = 0; h < count; ++h) {
    uint64_t sum = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t f = freqs[(size_t)h * n + i];
      if (f >= (1u << 23)) return set_error(ZT_E_ARG, "zt_debug_huffman: frequency of 2^23 or more");
      sum += f;
    }
    if (sum >= (1u << 27)) return set_error(ZT_E_ARG, "zt_debug_huffman: histogram sum of 2^27 or more");
  }
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  hipStream_t s = c->stream;
  const size_t total = (size_t)count * n;
  uint32_t *d_freq = nullptr, *d_codes = nullptr;
  uint8_t *d_lens = nullptr;
  ZT_TRY(scratch_carved(c, kDeflateOrDesc, [&](void *base) {
    Carve cv(base);
    d_freq = cv.take<uint32_t>(total);
    d_codes = cv.take<uint32_t>(total);
    d_lens = cv.take<uint8_t>(total);
    return cv.bytes();
  }));
  ZT_HIP(hipMemcpyAsync(d_freq, freqs, total * 4, hipMemcpyHostToDevice, s));
  debug_huffman_kernel<<<count, 64, 0, s>>>(d_freq, n, limit, d_lens, d_codes);
  ZT_HIP(hipGetLastError());
  ZT_HIP(hipMemcpyAsync(lens, d_lens, total, hipMemcpyDeviceToHost, s));
  ZT_HIP(hipMemcpyAsync(codes, d_codes, total * 4, hipMemcpyDeviceToHost, s));
  ZT_HIP(hipStreamSynchronize(s));
  return ZT_OK;
}

int deflate_post_run(const DeflateParams &P, uint64_t *boff, hipStream_t s) {
  if (P.opt) {
    price_kernel<<<P.nblocks, 64, 0, s>>>(P);
    ZT_HIP(hipGetLastError());
    optparse_kernel<<<P.nblocks, 64, 0, s>>>(P);
    ZT_HIP(hipGetLastError());
  }
  parse_kernel<<<P.nblocks, 64, 0, s>>>(P);
  ZT_HIP(hipGetLastError());
  block_kernel<<<P.nblocks, 64, 0, s>>>(P);
  ZT_HIP(hipGetLastError());
  scan_sizes<<<1, 1024, 0, s>>>(P.slot_len, P.nblocks, boff, 0, P.restart, P.final_, P.span);
  ZT_HIP(hipGetLastError());
  encode_kernel<<<P.nblocks, ENC_THREADS, 0, s>>>(P);
  ZT_HIP(hipGetLastError());
  return ZT_OK;
}

#ifdef ZT_DF_TIME
extern "C" int zt_debug_bk_time(unsigned long long *out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bk_time), sizeof(unsigned long long) * 8);
  unsigned long long z[8] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_bk_time), z, sizeof z);
  return 0;
}
#endif

}  // namespace zt
