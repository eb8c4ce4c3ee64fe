// zipcrypto.hip -- ZipCrypto on the device (src/ZipCrypto.ts; zipcrypto.h).
//
// Per plaintext byte p the cipher does
//   ks   = (((key2 & 0xFFFF) | 2) * (((key2 & 0xFFFF) | 2) ^ 1) >> 8) & 0xFF   (before the update)
//   key0 = crc_step(key0, p)
//   key1 = (key1 + (key0 & 0xFF)) * 134775813 + 1
//   key2 = crc_step(key2, key1 >> 24)
// and writes p ^ ks.
//
// ENCRYPT knows the plaintext, so all three registers are prefix scans.  A
// stream is cut into tiles of kTile bytes (one workgroup), a tile into chunks
// of kChunk bytes (one lane):
//   key0 at a chunk start = A^pos(K0) ^ S, S the from-zero CRC register of the
//     pos bytes before it and A^pos the advance over pos zero bytes -- a
//     multiplication by x^(8 pos) mod P, a constant for the fixed distances
//     kChunk * 2^k, kChunk * lane and kTile * 2^k;
//   key1: each byte applies x -> M x + (b M + 1), b = key0 & 0xFF after the
//     update; affine maps compose as (a2 a1, a2 c1 + c2) mod 2^32;
//   key2: a CRC scan again, over the bytes key1 >> 24.
// Four walks of the data (pass A: from-zero CRC; B: true key0, key1's maps;
// C: true key0 / key1, key2's from-zero CRC; D: the cipher) and between them
// three carry kernels, one wave per stream, that turn the tiles' aggregates
// into the registers at every tile start.  Nothing waits in-launch for another
// workgroup: every hand-over is a kernel boundary.
//
// DECRYPT is serial per stream (each plaintext byte feeds the key that
// decrypts the next): one lane per stream, 16-byte loads and stores.
//
// CRC step: a 256-entry table in LDS (ZT_ZC_TABLE=1, the default) or the
// table-free register step of checksum.hip (ZT_ZC_TABLE=0); the measured
// rates of both are in profiles/zipcrypto_time.json.
#include <cstdlib>

#include "zipcrypto.h"
#include "zt_internal.h"

namespace zt {
namespace zc {
namespace {

// ---- constants: x^(8 n) mod P, reflected (x^k is bit 31 - k) --------------------
constexpr uint32_t c_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if ((a >> (31 - i)) & 1) p ^= b;
    b = (b & 1) ? (b >> 1) ^ ZT_CRC_POLY : b >> 1;
  }
  return p;
}
constexpr uint32_t c_xpow8(uint64_t nbytes) {  // x^(8 nbytes)
  uint32_t r = 1u << 31, base = 1u << 23;     // x^0, x^8
  while (nbytes) {
    if (nbytes & 1) r = c_mul(r, base);
    base = c_mul(base, base);
    nbytes >>= 1;
  }
  return r;
}
struct LaneTab {
  uint32_t v[kLanes];
};
constexpr LaneTab make_lane_tab() {
  LaneTab t{};
  t.v[0] = 1u << 31;
  const uint32_t xc = c_xpow8(kChunk);
  for (uint32_t l = 1; l < kLanes; ++l) t.v[l] = c_mul(t.v[l - 1], xc);
  return t;
}
struct StepTab {
  uint32_t chunk[8];  // x^(8 kChunk 2^k)
  uint32_t tile[6];   // x^(8 kTile 2^k)
};
constexpr StepTab make_step_tab() {
  StepTab t{};
  for (int k = 0; k < 8; ++k) t.chunk[k] = c_xpow8((uint64_t)kChunk << k);
  for (int k = 0; k < 6; ++k) t.tile[k] = c_xpow8((uint64_t)kTile << k);
  return t;
}
__constant__ LaneTab kLaneTab = make_lane_tab();  // x^(8 kChunk lane)
constexpr StepTab kStep = make_step_tab();
static_assert(kLanes == 256 && kTile <= (16u << 10), "tile geometry");

// a * b mod P, branch-free
__device__ __forceinline__ uint32_t zc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    p ^= b & (0u - ((a >> (31 - i)) & 1u));
    b = (b >> 1) ^ (ZT_CRC_POLY & (0u - (b & 1u)));
  }
  return p;
}

__device__ __forceinline__ uint32_t crc_reg_byte(uint32_t c, uint32_t b) {
  c ^= b;
#pragma unroll
  for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (ZT_CRC_POLY & (0u - (c & 1u)));
  return c;
}
template <bool TAB>
__device__ __forceinline__ uint32_t crc_step(const uint32_t *tab, uint32_t c, uint32_t b) {
  if (TAB) return tab[(c ^ b) & 0xFF] ^ (c >> 8);
  return crc_reg_byte(c, b & 0xFF);
}
template <int THREADS>
__device__ __forceinline__ void fill_table(uint32_t *tab) {
  for (uint32_t i = threadIdx.x; i < 256; i += THREADS) tab[i] = crc_reg_byte(0, i);
  __syncthreads();
}

// f(byte) -> byte over the first len bytes of a 16-byte aligned chunk; STORE:
// the results go to dst (whole 16-byte pieces: bytes past len keep their value)
template <bool STORE, class F>
__device__ __forceinline__ void walk(const uint4 *src, uint4 *dst, uint32_t len, F &&f) {
#pragma unroll 1
  for (uint32_t w = 0; w * 16 < len; ++w) {
    const uint4 v = src[w];
    uint32_t x[4] = {v.x, v.y, v.z, v.w};
    const uint32_t nb = len - w * 16;
    if (nb >= 16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t y = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) y |= (f((x[j] >> (8 * b)) & 0xFF) & 0xFF) << (8 * b);
        x[j] = y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if ((uint32_t)(j * 4 + b) < nb) {
            const uint32_t o = f((x[j] >> (8 * b)) & 0xFF) & 0xFF;
            x[j] = (x[j] & ~(0xFFu << (8 * b))) | (o << (8 * b));
          }
      }
    }
    if (STORE) dst[w] = make_uint4(x[0], x[1], x[2], x[3]);
  }
}

__device__ __forceinline__ uint32_t chunk_len(uint32_t tile_len, uint32_t lane) {
  const uint32_t off = lane * kChunk;
  return off < tile_len ? min(kChunk, tile_len - off) : 0u;
}

// inclusive scan of from-zero CRC registers over the tile's lanes (every chunk
// before a non-empty one is full: the advance between neighbours is kChunk
// bytes); sh[] holds the result on return
__device__ __forceinline__ uint32_t scan_crc(uint32_t v, uint32_t *sh, uint32_t lane) {
  sh[lane] = v;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t d = 1u << k;
    const uint32_t o = lane >= d ? sh[lane - d] : 0u;
    __syncthreads();
    if (lane >= d) v ^= zc_mul(kStep.chunk[k], o);
    sh[lane] = v;
    __syncthreads();
  }
  return v;
}

// pass A: from-zero CRC register of every chunk; e0 = the register of the
// tile's bytes before the chunk, agg0 = of the whole tile
template <bool TAB>
__global__ __launch_bounds__(kLanes) void zc_pass_a(const uint8_t *__restrict__ data, const Tile *__restrict__ tiles,
                                                    uint32_t *__restrict__ e0, uint32_t *__restrict__ agg0) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t sh[kLanes];
  const uint32_t lane = threadIdx.x;
  const size_t t = blockIdx.x;
  if (TAB) fill_table<kLanes>(tab);
  const uint32_t len = chunk_len(tiles[t].len, lane);
  const uint4 *src = reinterpret_cast<const uint4 *>(data + t * kTile + (size_t)lane * kChunk);
  uint32_t c = 0;
  walk<false>(src, nullptr, len, [&](uint32_t b) {
    c = crc_step<TAB>(tab, c, b);
    return 0u;
  });
  const uint32_t incl = scan_crc(c, sh, lane);
  e0[t * kLanes + lane] = lane ? sh[lane - 1] : 0u;
  if (lane == kLanes - 1) agg0[t] = incl;
}

// carry of a CRC register over an item's tiles: start[t] = the register at
// tile t's first byte.  One wave per item, 64 tiles per round: lane 0's
// element takes the running register in, an inclusive scan gives the
// registers at the tiles' ends (every tile but an item's last is full).
__global__ __launch_bounds__(64) void zc_carry_crc(const Item *__restrict__ items, const uint32_t *__restrict__ agg,
                                                   uint32_t *__restrict__ start, int which) {
  const Item it = items[blockIdx.x];
  const uint32_t lane = threadIdx.x;
  uint32_t r = it.key[which];
  for (uint64_t base = 0; base < it.ntiles; base += 64) {
    const uint64_t t = base + lane;
    uint32_t v = t < it.ntiles ? agg[it.first_tile + t] : 0u;
    if (lane == 0) v ^= zc_mul(kStep.tile[0], r);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const uint32_t d = 1u << k;
      const uint32_t o = __shfl_up(v, d);
      if (lane >= d) v ^= zc_mul(kStep.tile[k], o);
    }
    const uint32_t prev = __shfl_up(v, 1u);
    if (t < it.ntiles) start[it.first_tile + t] = lane ? prev : r;
    r = __shfl(v, 63);
  }
}

// pass B: key0 at the chunk's start (left in e0), the chunk's key1 map;
// (ea, ec) = the map of the tile's bytes before the chunk, (agg_a, agg_c) = of
// the whole tile
template <bool TAB>
__global__ __launch_bounds__(kLanes) void zc_pass_b(const uint8_t *__restrict__ data, const Tile *__restrict__ tiles,
                                                    const uint32_t *__restrict__ start0, uint32_t *__restrict__ e0,
                                                    uint32_t *__restrict__ ea, uint32_t *__restrict__ ec,
                                                    uint32_t *__restrict__ agg_a, uint32_t *__restrict__ agg_c) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t sha[kLanes], shc[kLanes];
  const uint32_t lane = threadIdx.x;
  const size_t t = blockIdx.x, idx = t * kLanes + lane;
  if (TAB) fill_table<kLanes>(tab);
  const uint32_t len = chunk_len(tiles[t].len, lane);
  const uint4 *src = reinterpret_cast<const uint4 *>(data + t * kTile + (size_t)lane * kChunk);
  uint32_t k0 = zc_mul(kLaneTab.v[lane], start0[t]) ^ e0[idx];
  e0[idx] = k0;
  uint32_t a = 1, c = 0;
  walk<false>(src, nullptr, len, [&](uint32_t b) {
    k0 = crc_step<TAB>(tab, k0, b);
    c = (c + (k0 & 0xFF)) * kMul + 1;
    a *= kMul;
    return 0u;
  });
  sha[lane] = a;
  shc[lane] = c;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t d = 1u << k;
    const uint32_t oa = lane >= d ? sha[lane - d] : 1u, oc = lane >= d ? shc[lane - d] : 0u;
    __syncthreads();
    c = a * oc + c;  // (oa, oc) first, then (a, c)
    a = a * oa;
    sha[lane] = a;
    shc[lane] = c;
    __syncthreads();
  }
  ea[idx] = lane ? sha[lane - 1] : 1u;
  ec[idx] = lane ? shc[lane - 1] : 0u;
  if (lane == kLanes - 1) {
    agg_a[t] = a;
    agg_c[t] = c;
  }
}

// carry of key1 over an item's tiles (maps compose for any tile length)
__global__ __launch_bounds__(64) void zc_carry_affine(const Item *__restrict__ items,
                                                      const uint32_t *__restrict__ agg_a,
                                                      const uint32_t *__restrict__ agg_c,
                                                      uint32_t *__restrict__ start) {
  const Item it = items[blockIdx.x];
  const uint32_t lane = threadIdx.x;
  uint32_t r = it.key[1];
  for (uint64_t base = 0; base < it.ntiles; base += 64) {
    const uint64_t t = base + lane;
    uint32_t a = t < it.ntiles ? agg_a[it.first_tile + t] : 1u;
    uint32_t c = t < it.ntiles ? agg_c[it.first_tile + t] : 0u;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const uint32_t d = 1u << k;
      const uint32_t oa = __shfl_up(a, d), oc = __shfl_up(c, d);
      if (lane >= d) {
        c = a * oc + c;
        a = a * oa;
      }
    }
    uint32_t xa = __shfl_up(a, 1u), xc = __shfl_up(c, 1u);
    if (lane == 0) {
      xa = 1;
      xc = 0;
    }
    if (t < it.ntiles) start[it.first_tile + t] = xa * r + xc;
    r = __shfl(a, 63) * r + __shfl(c, 63);
  }
}

// pass C: key1 at the chunk's start (left in ea), the from-zero CRC register
// of the chunk's key1 >> 24 bytes; e2 / agg2 as pass A's e0 / agg0
template <bool TAB>
__global__ __launch_bounds__(kLanes) void zc_pass_c(const uint8_t *__restrict__ data, const Tile *__restrict__ tiles,
                                                    const uint32_t *__restrict__ start1,
                                                    const uint32_t *__restrict__ e0, uint32_t *__restrict__ ea,
                                                    const uint32_t *__restrict__ ec, uint32_t *__restrict__ e2,
                                                    uint32_t *__restrict__ agg2) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t sh[kLanes];
  const uint32_t lane = threadIdx.x;
  const size_t t = blockIdx.x, idx = t * kLanes + lane;
  if (TAB) fill_table<kLanes>(tab);
  const uint32_t len = chunk_len(tiles[t].len, lane);
  const uint4 *src = reinterpret_cast<const uint4 *>(data + t * kTile + (size_t)lane * kChunk);
  uint32_t k0 = e0[idx];
  uint32_t k1 = ea[idx] * start1[t] + ec[idx];
  ea[idx] = k1;
  uint32_t c2 = 0;
  walk<false>(src, nullptr, len, [&](uint32_t b) {
    k0 = crc_step<TAB>(tab, k0, b);
    k1 = (k1 + (k0 & 0xFF)) * kMul + 1;
    c2 = crc_step<TAB>(tab, c2, k1 >> 24);
    return 0u;
  });
  const uint32_t incl = scan_crc(c2, sh, lane);
  e2[idx] = lane ? sh[lane - 1] : 0u;
  if (lane == kLanes - 1) agg2[t] = incl;
}

// pass D: the cipher, in place
template <bool TAB>
__global__ __launch_bounds__(kLanes) void zc_pass_d(uint8_t *__restrict__ data, const Tile *__restrict__ tiles,
                                                    const uint32_t *__restrict__ start2,
                                                    const uint32_t *__restrict__ e0, const uint32_t *__restrict__ ea,
                                                    const uint32_t *__restrict__ e2) {
  __shared__ uint32_t tab[256];
  const uint32_t lane = threadIdx.x;
  const size_t t = blockIdx.x, idx = t * kLanes + lane;
  if (TAB) fill_table<kLanes>(tab);
  const uint32_t len = chunk_len(tiles[t].len, lane);
  uint4 *p = reinterpret_cast<uint4 *>(data + t * kTile + (size_t)lane * kChunk);
  uint32_t k0 = e0[idx], k1 = ea[idx];
  uint32_t k2 = zc_mul(kLaneTab.v[lane], start2[t]) ^ e2[idx];
  walk<true>(p, p, len, [&](uint32_t b) {
    const uint32_t q = (k2 & 0xFFFF) | 2;
    const uint32_t ks = ((q * (q ^ 1)) >> 8) & 0xFF;
    k0 = crc_step<TAB>(tab, k0, b);
    k1 = (k1 + (k0 & 0xFF)) * kMul + 1;
    k2 = crc_step<TAB>(tab, k2, k1 >> 24);
    return b ^ ks;
  });
}

// decrypt: lane i walks stream i in place
template <bool TAB>
__global__ __launch_bounds__(64) void zipcrypto_decrypt_kernel(uint8_t *__restrict__ data,
                                                               const Stream *__restrict__ streams, uint32_t count) {
  __shared__ uint32_t tab[256];
  if (TAB) fill_table<64>(tab);
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  const Stream st = streams[i];
  uint8_t *p = data + st.off;
  uint64_t n = st.len;
  uint32_t k0 = st.key[0], k1 = st.key[1], k2 = st.key[2];
  auto dec = [&](uint32_t c) {
    const uint32_t q = (k2 & 0xFFFF) | 2;
    const uint32_t b = (c ^ ((q * (q ^ 1)) >> 8)) & 0xFF;
    k0 = crc_step<TAB>(tab, k0, b);
    k1 = (k1 + (k0 & 0xFF)) * kMul + 1;
    k2 = crc_step<TAB>(tab, k2, k1 >> 24);
    return b;
  };
  while (n && (reinterpret_cast<uintptr_t>(p) & 15)) {
    *p = (uint8_t)dec(*p);
    ++p;
    --n;
  }
  while (n >= 16) {
    uint4 *q = reinterpret_cast<uint4 *>(p);
    walk<true>(q, q, 16, dec);
    p += 16;
    n -= 16;
  }
  while (n) {
    *p = (uint8_t)dec(*p);
    ++p;
    --n;
  }
}

bool use_table() {
  static const bool v = [] {
    const char *e = getenv("ZT_ZC_TABLE");
    return !(e && e[0] == '0');
  }();
  return v;
}

struct Work {
  uint32_t *e0, *ea, *ec, *e2;               // per chunk
  uint32_t *agg0, *agg_a, *agg_c, *agg2;     // per tile
  uint32_t *start0, *start1, *start2;        // per tile
};
Work carve(void *d_work, size_t ntiles) {
  uint32_t *p = static_cast<uint32_t *>(d_work);
  const size_t nc = ntiles * kLanes;
  Work w;
  w.e0 = p;
  w.ea = p + nc;
  w.ec = p + 2 * nc;
  w.e2 = p + 3 * nc;
  uint32_t *q = p + 4 * nc;
  w.agg0 = q;
  w.agg_a = q + ntiles;
  w.agg_c = q + 2 * ntiles;
  w.agg2 = q + 3 * ntiles;
  w.start0 = q + 4 * ntiles;
  w.start1 = q + 5 * ntiles;
  w.start2 = q + 6 * ntiles;
  return w;
}

template <bool TAB>
int encrypt_run(uint8_t *d, const Tile *tl, size_t ntiles, const Item *it, size_t nitems, const Work &w,
                hipStream_t s) {
  const dim3 gt((uint32_t)ntiles), gi((uint32_t)nitems);
  hipLaunchKernelGGL(zc_pass_a<TAB>, gt, dim3(kLanes), 0, s, d, tl, w.e0, w.agg0);
  hipLaunchKernelGGL(zc_carry_crc, gi, dim3(64), 0, s, it, w.agg0, w.start0, 0);
  hipLaunchKernelGGL(zc_pass_b<TAB>, gt, dim3(kLanes), 0, s, d, tl, w.start0, w.e0, w.ea, w.ec, w.agg_a, w.agg_c);
  hipLaunchKernelGGL(zc_carry_affine, gi, dim3(64), 0, s, it, w.agg_a, w.agg_c, w.start1);
  hipLaunchKernelGGL(zc_pass_c<TAB>, gt, dim3(kLanes), 0, s, d, tl, w.start1, w.e0, w.ea, w.ec, w.e2, w.agg2);
  hipLaunchKernelGGL(zc_carry_crc, gi, dim3(64), 0, s, it, w.agg2, w.start2, 2);
  hipLaunchKernelGGL(zc_pass_d<TAB>, gt, dim3(kLanes), 0, s, d, tl, w.start2, w.e0, w.ea, w.e2);
  ZT_HIP(hipGetLastError());
  return ZT_OK;
}

}  // namespace

size_t encrypt_work_bytes(size_t ntiles) { return ntiles * (4 * (size_t)kLanes + 7) * sizeof(uint32_t) + 16; }

int encrypt_dev(uint8_t *d_data, const Tile *d_tiles, size_t ntiles, const Item *d_items, size_t nitems,
                void *d_work, hipStream_t s) {
  if (ntiles == 0 || nitems == 0) return ZT_OK;
  if (ntiles > 0x7FFFFFFFull || nitems > 0x7FFFFFFFull) return set_error(ZT_E_ARG, "zipcrypto: batch too large");
  const Work w = carve(d_work, ntiles);
  return use_table() ? encrypt_run<true>(d_data, d_tiles, ntiles, d_items, nitems, w, s)
                     : encrypt_run<false>(d_data, d_tiles, ntiles, d_items, nitems, w, s);
}

int decrypt_dev(uint8_t *d_data, const Stream *d_streams, size_t count, hipStream_t s) {
  if (count == 0) return ZT_OK;
  if (count > 0x7FFFFFFFull) return set_error(ZT_E_ARG, "zipcrypto: batch too large");
  const dim3 g((uint32_t)((count + 63) / 64));
  if (use_table())
    hipLaunchKernelGGL(zipcrypto_decrypt_kernel<true>, g, dim3(64), 0, s, d_data, d_streams, (uint32_t)count);
  else
    hipLaunchKernelGGL(zipcrypto_decrypt_kernel<false>, g, dim3(64), 0, s, d_data, d_streams, (uint32_t)count);
  ZT_HIP(hipGetLastError());
  return ZT_OK;
}

}  // namespace zc
}  // namespace zt
