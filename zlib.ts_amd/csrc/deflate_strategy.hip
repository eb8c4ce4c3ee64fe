// deflate_strategy.hip -- the strategies' producer of res (include/zt_strategy.h):
// what deflate_match_launch (deflate.hip) runs in place of match_kernel for
// ZT_STRATEGY_RLE and ZT_STRATEGY_HUFFMAN_ONLY.  A streaming kernel: it reads
// every input byte once and writes one res word (res_pack) per position, 5
// bytes moved per input byte; the post-match stages (deflate_post.hip) read
// res as they read match_kernel's.
//
// Huffman-only: res[i] = res_pack(byte[i], 0, 0).
//
// RLE (the definition: include/zt_strategy.h; tests/strategy_ref.py restates
// it): res[i] = res_pack(byte[i], L(i), L(i) ? 1 : 0), where a run reaches
// back no further than lo(i) -- the stream's first byte, the halo's first
// byte for the first segment of a single stream with a halo, the start of
// i's segment from the second segment on -- and forward no further than 258
// bytes, i's block and the stream.  Every position holds exactly that word,
// inside a longer run too: nothing is carried from one position to the next.
//
// One workgroup per 32 KiB block, whatever the match kernel's work split: a
// run is cut at the block's end (cap), so no look-ahead leaves the block, and
// the only byte read outside it is the one in front of its first position.
//   1. every thread loads 8 chunks of 16 bytes (16-byte loads, all issued
//      before the first use) and puts them into the block's LDS image;
//   2. (RLE) per chunk 16 *break* bits, one per position: byte[x] != byte[x - 1],
//      or no byte in front of x that x may reference.  Bits from the stream's
//      end on are set, and so are the words behind the block's: run_end(x) is
//      then the next set bit after x, and the block and stream bounds of
//      cap(x) need no code of their own.  A run spans at most 258 bytes, so the
//      search reads at most 12 words of the 4 KiB bit image; no scan over the
//      block, nothing between workgroups, no atomics;
//   3. every thread takes 4 consecutive positions per step -- a dword of the
//      image, a 64-bit window of the break bits -- and stores their 4 words
//      with one 16-byte store: a wave writes 1 KiB of res contiguously.
// LDS: 32 KiB image + 4.1 KiB break bits = 4 workgroups (16 waves) per CU with
// 128 KiB of loads in flight.  The image's ds_write_b128 (lane k at 16 k) and
// ds_read_b32 (lane k at 4 k) are conflict-free; the break bits' reads of one
// step touch 8 consecutive words per wave, mostly broadcast.
// (profiles/strategy_resource_usage.txt: registers and LDS as compiled.)
#include "../../include/zt_strategy.h"
#include "zt_internal.h"

namespace zt {

namespace {

constexpr uint32_t ST_THREADS = 256;
constexpr uint32_t ST_CHUNKS = DF_BLOCK / 16;             // 16-byte chunks of a block
constexpr uint32_t ST_PER_THREAD = ST_CHUNKS / ST_THREADS;  // chunks a thread loads
constexpr uint32_t ST_STEP = ST_THREADS * 4;              // positions per step of the store loop
constexpr uint32_t ST_BRK_WORDS = DF_BLOCK / 32;
// words of set bits behind the block's: a 64-bit window from the last quad
// reads 2 of them, the search for a break up to 262 positions on 10 more
constexpr uint32_t ST_BRK_PAD = 12;
constexpr uint32_t ST_MAX_LEN = 258;
static_assert(DF_BLOCK % (16 * ST_THREADS) == 0 && DF_BLOCK % ST_STEP == 0, "whole rounds of chunks and quads");
static_assert((ST_MAX_LEN + 4 + 31) / 32 + 2 <= ST_BRK_PAD, "the break search stays inside the padding");

struct StrategyShared {
  uint4 image[ST_CHUNKS];                     // the block's bytes (zero from the stream's end on)
  uint32_t brk[ST_BRK_WORDS + ST_BRK_PAD];    // RLE: bit x: position x cannot continue a run
};

// `valid` (0..16) bytes at p as a chunk, the rest zero: the ragged end of a
// stream (nothing behind the stream is read) and inputs that are not 16-byte
// aligned (a halo of odd length in front of a caller's buffer)
__device__ __forceinline__ uint4 load_bytes(const uint8_t *p, uint32_t valid) {
  uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k)
    if (k < valid) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// break bits of one chunk: bit k = byte k differs from the byte in front of it
// (prev: the byte in front of the chunk, or 0x100: none that may be referenced)
__device__ __forceinline__ uint32_t chunk_breaks(const uint4 v, uint32_t prev) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = prev > 0xFFu ? 1u : 0u;
  uint32_t pb = prev & 0xFFu;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t d = w[j] ^ ((w[j] << 8) | pb);  // every byte against the one in front of it
    m |= ((d & 0xFFu) ? 1u : 0u) << (4 * j);
    m |= ((d & 0xFF00u) ? 2u : 0u) << (4 * j);
    m |= ((d & 0xFF0000u) ? 4u : 0u) << (4 * j);
    m |= ((d & 0xFF000000u) ? 8u : 0u) << (4 * j);
    pb = w[j] >> 24;
  }
  return m;
}

template <bool RLE>
__global__ __launch_bounds__(ST_THREADS) void strategy_kernel(DeflateParams P) {
  __shared__ StrategyShared sh;
  const uint32_t t = threadIdx.x;
  const uint32_t blk = blockIdx.x;
  const uint64_t lo = (uint64_t)blk * DF_BLOCK;  // the block's first position (batch: in the packed buffer)
  const uint64_t n = stream_end(P, blk);
  const uint32_t blen = (uint32_t)((n - lo) < DF_BLOCK ? (n - lo) : DF_BLOCK);
  const uint8_t *g = P.base + P.halo + lo;  // the block's first byte
  const bool aligned = (reinterpret_cast<uintptr_t>(g) & 15) == 0;

  // 1. the block into registers, then into the image
  uint4 v[ST_PER_THREAD];
  if (aligned && blen == DF_BLOCK) {  // a whole block: no branch between the loads, all in flight at once
#pragma unroll
    for (uint32_t k = 0; k < ST_PER_THREAD; ++k)
      v[k] = *reinterpret_cast<const uint4 *>(g + (k * ST_THREADS + t) * 16);
  } else {  // a stream's last block, or an unaligned input: chunk by chunk
#pragma unroll
    for (uint32_t k = 0; k < ST_PER_THREAD; ++k) {
      const uint32_t x = (k * ST_THREADS + t) * 16;
      if (aligned && x + 16 <= blen)
        v[k] = *reinterpret_cast<const uint4 *>(g + x);
      else
        v[k] = load_bytes(g + x, x < blen ? (blen - x < 16 ? blen - x : 16u) : 0u);
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < ST_PER_THREAD; ++k) sh.image[k * ST_THREADS + t] = v[k];

  if (RLE) {
    __syncthreads();
    // 2. break bits.  The byte in front of a chunk is the image's, in front
    // of the block it is the input's -- unless the block starts a segment
    // (restart point) or its stream: then position 0 may reference nothing,
    // except the halo in front of a single stream's first block
    const uint64_t first = P.span ? P.span[2 * (uint64_t)blk] / DF_BLOCK : 0;
    const bool seg_start = ((blk - first) % P.restart) == 0;
    const bool front = !seg_start || (!P.span && blk == 0 && P.halo > 0);
    const uint8_t *img = reinterpret_cast<const uint8_t *>(sh.image);
    typedef uint16_t __attribute__((may_alias)) brk_half;  // (the words are read whole in step 3)
    brk_half *brk16 = reinterpret_cast<brk_half *>(sh.brk);
#pragma unroll
    for (uint32_t k = 0; k < ST_PER_THREAD; ++k) {
      const uint32_t c = k * ST_THREADS + t, x = c * 16;
      uint32_t m = 0xFFFFu;
      if (x < blen) {
        const uint32_t prev = x ? img[x - 1] : front ? g[-1] : 0x100u;
        m = chunk_breaks(v[k], prev);
        if (blen - x < 16) m |= 0xFFFFu << (blen - x);  // from the stream's end on
      }
      brk16[c] = (uint16_t)m;
    }
    if (t < ST_BRK_PAD) sh.brk[ST_BRK_WORDS + t] = 0xFFFFFFFFu;
  }
  __syncthreads();

  // 3. four positions per thread and step
  const uint32_t *img32 = reinterpret_cast<const uint32_t *>(sh.image);
  uint32_t *res = P.res + lo;
#pragma unroll 4
  for (uint32_t x = t * 4; x < blen; x += ST_STEP) {
    const uint32_t w = img32[x >> 2];
    uint32_t len[4] = {0, 0, 0, 0};
    if (RLE) {
      // W: the break bits of positions x .. x + 63
      const uint32_t bi = x >> 5, sft = x & 31;
      const uint64_t w01 = (uint64_t)sh.brk[bi] | ((uint64_t)sh.brk[bi + 1] << 32);
      const uint32_t w2 = sh.brk[bi + 2];
      const uint64_t W = sft ? (w01 >> sft) | ((uint64_t)w2 << (64 - sft)) : w01;
      if ((W & 15u) != 15u) {  // a position of the quad continues a run
        // the first break at or behind x + 64, as a distance from x; 262 or
        // more is as good as any (the longest run wanted ends at x + 3 + 258)
        uint32_t far = ST_MAX_LEN + 4;
        if ((W >> 4) == 0) {
          const uint32_t part = sft ? (w2 >> sft) : 0u;  // bits x + 64 .. of word bi + 2
          if (part) {
            far = 64 + (uint32_t)__builtin_ctz(part);
          } else {
            for (uint32_t wi = bi + (sft ? 3 : 2); wi * 32 < x + ST_MAX_LEN + 4; ++wi) {
              const uint32_t b = sh.brk[wi];
              if (b) {
                far = wi * 32 + (uint32_t)__builtin_ctz(b) - x;
                break;
              }
            }
          }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
          if ((W >> k) & 1) continue;
          const uint64_t rest = W >> (k + 1);  // breaks behind x + k
          const uint32_t next = rest ? k + 1 + (uint32_t)__builtin_ctzll(rest) : far;
          const uint32_t run = next - k;       // run_end - position, cut at the block's and the stream's end
          const uint32_t l = run < ST_MAX_LEN ? run : ST_MAX_LEN;
          len[k] = l >= 3 ? l : 0;
        }
      }
    }
    uint4 o;
    o.x = res_pack(w & 0xFFu, len[0], len[0] ? 1u : 0u);
    o.y = res_pack((w >> 8) & 0xFFu, len[1], len[1] ? 1u : 0u);
    o.z = res_pack((w >> 16) & 0xFFu, len[2], len[2] ? 1u : 0u);
    o.w = res_pack(w >> 24, len[3], len[3] ? 1u : 0u);
    // (the words behind a ragged end are literals of zero bytes, inside res: nobody reads them)
    *reinterpret_cast<uint4 *>(res + x) = o;
  }
}

}  // namespace

int deflate_strategy_launch(const DeflateParams &P, hipStream_t s) {
  if (P.strategy == ZT_STRATEGY_RLE)
    strategy_kernel<true><<<P.nblocks, ST_THREADS, 0, s>>>(P);
  else if (P.strategy == ZT_STRATEGY_HUFFMAN_ONLY)
    strategy_kernel<false><<<P.nblocks, ST_THREADS, 0, s>>>(P);
  else
    return set_error(ZT_E_INTERNAL, "deflate: unknown strategy");
  ZT_HIP(hipGetLastError());
  return ZT_OK;
}

}  // namespace zt
