// zt_internal.h -- shared host/device helpers for libzt (not installed).
#pragma once
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/zt.h"
#include "batch_plan.h"
#include "deflate_index_host.h"
#include "dev_batch_plan.h"
#include "dict_host.h"
#include "inflate_chain.h"

namespace zt {

// ---- error plumbing -------------------------------------------------------
int set_error(int code, const std::string &msg);
int hip_fail(hipError_t e, const char *what);

#define ZT_HIP(call)                                       \
  do {                                                     \
    hipError_t e_ = (call);                                \
    if (e_ != hipSuccess) return ::zt::hip_fail(e_, #call); \
  } while (0)

#define ZT_TRY(call)      \
  do {                    \
    int rc_ = (call);     \
    if (rc_) return rc_;  \
  } while (0)

// ---- per-device context -----------------------------------------------------
// checksum_segments' in-kernel merge (checksum.hip): zero between calls
// checksum merge (checksum.hip): each workgroup's partial sums in its own
// slot, then group tickets (128 bytes apart) and one top ticket -- the last
// workgroup to arrive reduces the slots
constexpr int kCkGroups = 32;
constexpr int kCkMaxWg = 4096;  // checksums_dev's grid: at most num_cu * 8
struct CkPart {
  unsigned long long s1, s2;
  uint32_t crc, pad[3];
};
struct CkAcc {
  uint32_t grp[kCkGroups * 32];
  uint32_t done, pad[31];
  CkPart part[kCkMaxWg];
};

// Device scratch slots (DeviceCtx::d_buf, scratch()).  Per slot: its owner, and
// what a holder of its pointer may call while it still uses that pointer.
enum ScratchSlot : int {
  kIn = 0,          // the host entry points' input on the device; the holder may call any launcher (none asks for it)
  kOut = 1,         // deflate output of the host entry points, and the library-owned inflate output:
                    // inflate_segments_dev / general_dev / the batch decoders hand it out through *d_out_io
                    // or as `d_out`; valid until the next inflate or deflate call on this context
  kSmall = 2,       // a few job / result records of the entry points (and ZT_TOK_CHECK's words); no launcher call between
  kDeflateOrDesc = 3,  // two users, never at once: the deflate pipeline's scratch (deflate_scratch, whole call)
                    // and the two-phase inflate's descriptors (segment and batch paths: resolve only)
  kTokens = 4,      // two-phase tokens (segment and batch paths): from tokenize to the end of resolve
  kSyncCand = 5,    // inflate_segments_dev: sync candidates, steps 1-2 only
  kTokMeta = 6,     // stops | restart flags | TokJob | TokResult (segment path), TokJob | TokResult (batch): whole call
  kChain = 7,       // chain | segments | statuses (| ChainInfo) of the segment and batch paths: resolve only
  kCkSeg = 8,       // checksums_dev's segment partials; inside the call
  kCkBatch = 9,     // checksums_batch_dev's job tables; inside the call
  kGenCand = 10,    // general inflate (inflate_gen.hip), 10-17: inside one general_dev call; it calls
  kGenTokens = 11,  //   no launcher that asks for these or for another path's slots (it may take kOut)
  kGenMeta = 12,
  kGenBitmap = 13,
  kGenChain = 14,
  kGenDesc = 15,
  kGenOut16 = 16,
  kGenWindows = 17,
  kSums = 18,       // per-item (crc, adler) of the batch calls; until they are copied back in the same call
  kContainerIn = 19,  // unzip / gunzip member input (zip_api, container_api) and zt_gunzip_batch's member scan;
                    // the holder may call the inflate and checksum launchers (none asks for it)
  kSyncSort = 20,   // inflate_segments_dev: sort storage | keys | flags | positions | token offsets, up to the device chain
  kDeflateIndex = 21,  // deflate-time index (deflate_api.cpp, container_api.cpp): the entry table of the stream
                    // being written; whole call (the deflate launchers never ask for it)
  kPipeOut = 22,    // pipelined host inflate's output; the holder calls inflate_parallel_dev (never asks for 22-25)
  kPipeRing0 = 23,  // 23-25: its overflow ring, piece i's buffer reused once piece i - 3 has left the device
  kGenJump = 26,    // general inflate's window pointer-jumping buffers
  kFramed = 27,     // framed batch members (batch_api.cpp); inside the call
  kTokOrder = 28,   // segment path: tokenize / expand launch order, up to resolve
  kDict = 29,       // a preset dictionary (zt_dict.h: deflate history | inflate window | the whole dictionary);
                    // the holder may call the batch deflate / inflate launchers
  kIndexPack = 30,  // index build (inflate_seg.hip): on-chain unit ids | packed index entries; after resolve, inside the call
  kRangeIn = 31,    // a range call (range_call.h: the index and checkpoint formats; BGZF's decode_blocks_dev): chain |
                    // segments | ranges | ChainInfo | the format's tables | packed input (one upload), then the
                    // format's device-only results; whole call (it also takes kTokens, kDeflateOrDesc and kOut)
  kRangeOut = 32,   // a range call: packed ranges | statuses (| the format's), one download; whole call
                    // (31, 32: one range call at a time, never inside another)
  kCkptWin = 33,    // checkpoint build (ckpt_api.hip): window offsets | window records; after the general decode, inside the call
  kDevBatch = 34,   // device-resident batch calls (dev_batch_api.cpp): the copy and patch job tables of one launch;
                    // the holder calls the batch deflate / inflate and checksum launchers (none asks for it)
  kSession = 35,    // inflate sessions (stream_api.cpp): the job and result records of one launch; the holder
                    // calls the checksum launcher (it also takes kIn, kOut and kSums for the whole call)
  kScratchSlots
};
// Pinned host staging (DeviceCtx::h_pinned, pinned()).
enum PinnedSlot : int {
  kPinBatch = 0,        // batch data of the host entry points; inside the call
  kPinInflateMeta = 1,  // inflate metadata (coherent): the segment path's tables and resolve_chain_dev's
                        // chain / statuses; the segment path sizes it once for both, so its tables stay valid
  kPinChunk0 = 2,       // 2-3 upload / download chunks (upload, download), 4-5 the three-stage pipeline's
                        // download chunks (pipeline_h2d_d2h)
  kPinGroupIn = 6,      // second input group of a grouped batch (batch_api.cpp)
  kPinGroupOut = 7,     // its output group
  kPinMailbox = 8,      // the readback mailbox (mailbox()): valid until the next mailbox / readback call
  kPinUnused = 9,
  kPinnedSlots
};

// One default stream per device plus grow-only scratch buffers, so the
// host-pointer entry points do not hipMalloc on every call.
struct DeviceCtx {
  // host entry points hold it for their whole call: scratch, pinned staging
  // and the streams are shared by every thread that uses this device
  std::recursive_mutex mu;
  int device = -1;  // logical device (zt_set_device index)
  int phys = -1;    // HIP device it runs on (differs only under ZT_ALIAS_DEVICES)
  hipStream_t stream = nullptr;
  int num_cu = 0;
  // checksum constants (uploaded once)
  uint32_t *d_crc_nib = nullptr;    // nibble tables (ZT_CRC_NIB_N entries)
  uint32_t *d_crc_x2n = nullptr;    // x^(2^k) mod P, k = 0..31
  uint32_t *d_crc_shift = nullptr;  // checksum.hip merge constants (crc_shift_tables)
  CkAcc *d_ck_acc = nullptr;        // checksum merge accumulators (zeroed once, left zeroed by every call)
  // scratch
  static constexpr int kSlots = kScratchSlots;
  void *d_buf[kSlots] = {};  // (ScratchSlot)
  size_t buf_size[kSlots] = {};
  // second stream: checksums run beside the deflate pipeline in the containers
  hipStream_t aux = nullptr;
  hipEvent_t aux_ev = nullptr;
  void *h_pinned[kPinnedSlots] = {};  // (PinnedSlot)
  hipEvent_t xfer_ev[4] = {};  // chunk buffer kPinChunk0 + k's copy has finished
  hipStream_t up = nullptr, dn = nullptr;  // pipeline_h2d_d2h: H2D and D2H copy streams
  // zt_timing_enable: HIP-event kernel timing
  bool timing = false;
  hipEvent_t ev[8] = {};  // [2k, 2k+1]: interval k (0 match, 1 deflate pipeline, 2 inflate)
  zt_kernel_times times = {};
  size_t pinned_size[kPinnedSlots] = {};
};

// Carves one buffer into typed pieces, each 256-byte aligned, so that a
// buffer's size and the pointers into it come from the same lines: with a
// null base take() only counts (bytes() is then the size to allocate), with a
// real base it hands out the pointers.  (align_up, the host code's one
// rounding function, comes from inflate_chain.h.)
class Carve {
 public:
  explicit Carve(void *base = nullptr) : base_(static_cast<uint8_t *>(base)) {}
  template <typename T>
  T *take(size_t count) {
    T *p = base_ ? reinterpret_cast<T *>(base_ + at_) : nullptr;
    at_ += align_up(count * sizeof(T), 256);
    return p;
  }
  size_t bytes() const { return at_; }

 private:
  uint8_t *base_;
  size_t at_ = 0;
};

// Host wall-clock stamps of a host driver's stages on stderr when the
// environment variable `env` is set (measurement only): ZT_INF_TIMING in
// inflate_seg.hip, ZT_BATCH_TIMING in inflate_api.cpp.
double now_ms();                                      // the host's steady clock, in milliseconds
void host_stamp(const char *tag, const char *label);  // "[tag] label  <now_ms()>"
#define ZT_STAMP(env, tag, label)                   \
  do {                                              \
    static const bool on_ = getenv(env) != nullptr; \
    if (on_) ::zt::host_stamp(tag, label);          \
  } while (0)

// a *_stats_read counter: its value, zeroed when `reset`
inline uint64_t stat_take(std::atomic<uint64_t> &a, int reset) { return reset ? a.exchange(0) : a.load(); }

// Records the begin / end event of interval k (0 or 1) when timing is on.
int timing_begin(DeviceCtx *c, hipStream_t s, int k = 0);
int timing_end(DeviceCtx *c, hipStream_t s, int k = 0);
// After the stream is synchronized: adds interval k's elapsed time to *acc.
int timing_collect(DeviceCtx *c, double *acc_ms, uint64_t *count, int k = 0);

// Context of the calling thread's current device (created on first use).
int get_ctx(DeviceCtx **out);
// Grow-only device scratch slot `slot` (a ScratchSlot) to at least `bytes`.
// A slot that grows is freed and allocated again, so every earlier pointer
// into it dies: hold no pointer into slot X across a call that may also ask
// for slot X (the enum says, per slot, which calls a holder may make).  The
// same holds for pinned().
int scratch(DeviceCtx *c, int slot, size_t bytes, void **ptr);
// Grow-only pinned host staging buffer `slot` (a PinnedSlot) of at least `bytes`.
int pinned(DeviceCtx *c, size_t bytes, void **ptr, int slot = kPinBatch);
// Scratch slot `slot` carved by carve(base) -> bytes (a Carve inside): called
// with null for the size, then with the slot's base for the pointers.
template <typename F>
int scratch_carved(DeviceCtx *c, int slot, F &&carve) {
  void *base;
  ZT_TRY(scratch(c, slot, carve(nullptr), &base));
  carve(base);
  return ZT_OK;
}
// Small transfers between the host and the device (counts, per-unit
// results, chain tables) go through pinned memory: a pageable destination
// adds a staging copy inside the runtime.  q_copy(dst, src, n, s): a kernel
// copy (either end device or pinned host memory).  mailbox(c, n): a pinned, coherent region of
// >= n bytes (kPinMailbox), valid until the next mailbox call (one user at
// a time: the context's caller thread).  readback(c, dst, src, n, s): n bytes
// from the device to any host dst through the mailbox, synchronous.
int q_copy(void *dst, const void *src, size_t n, hipStream_t s);
// small transfer into / out of pinned memory: the copy engines
// (hipMemcpyAsync), or with ZT_QCOPY=1 q_copy (A/B: measured slower inside
// the host pipelines, gpurun_out/r06t)
int x_copy(void *dst, const void *src, size_t n, hipStream_t s);
// q_bytes(dst, v, n, s): the n <= 8 low bytes of v (little endian) to device dst, by a kernel
int q_bytes(void *dst, uint64_t v, uint32_t n, hipStream_t s);
int mailbox(DeviceCtx *c, size_t n, void **p);
int readback(DeviceCtx *c, void *h_dst, const void *d_src, size_t n, hipStream_t s);
// Host output buffer the caller frees with zt_free (large ones on huge pages;
// pool = true: from the bounded host output pool, host_mem.cpp); host_release
// is zt_free's second half (back to the pool, or free).  host_direct: [p,
// p + n) lies in a pool buffer registered with HIP, so copies to / from it go
// by DMA without staging.
uint8_t *host_out(size_t n, bool pool = false);
void host_release(void *p);
// host_out_used: the bytes a pooled output actually returns (what zt_free
// registers), when less than requested; host_discard: an output never handed
// out (an error path) freed outright instead of pooled
void host_out_used(void *p, size_t n);
void host_discard(void *p);
bool host_direct(const void *p, size_t n);
void host_pool_drop();  // the pool's free buffers released (zt_release_scratch)
// One host allocation for `items` batch outputs (pointers inside it, each
// released by zt_free; reserve >= 1 byte per item so every pointer is
// distinct).  slab_release: true when p lay in a slab (and was released).
uint8_t *slab_out(size_t total, size_t items, bool pool = false);
// device framing of batch members (member_frame.hip): item k's prefix | body |
// trailer at out + it[k].out_off; the trailer is put_trailer's for `kind`
// (member_frame.h); sums = (crc, adler) per item
struct FrameItem {
  uint64_t body_off;  // in the deflate output
  uint64_t out_off;   // in the framed output
  uint32_t body_len;
  uint32_t isize;
};
// patch > 0 (BGZF's BSIZE, bgzf_api.hip): prefix bytes [patch, patch + 2) of
// item k become its size - 1 (prefix + body + trailer), little endian
int frame_members_dev(const FrameItem *d_items, uint32_t count, const uint8_t *d_prefix, uint32_t plen,
                      MemberKind kind, const uint8_t *d_body, const uint32_t *d_sums, uint8_t *d_out, hipStream_t s,
                      uint32_t patch = 0);
bool slab_release(void *p);
// fn(0 .. count-1) over a few host threads when total_bytes is large.
// memcpy into pinned staging with streaming stores (xfer.cpp)
void copy_to_staging(void *dst, const void *src, size_t n);
void parallel_copy(size_t count, const std::function<void(size_t)> &fn, size_t total_bytes);
// parallel_copy's thread budget on the calling thread (default 8)
void set_copy_threads(size_t k);

// ---- CRC-32 algebra (reflected, P = 0xEDB88320) ------------------------------
// Host and device copies of zlib-style polynomial arithmetic: shifting a raw
// CRC register over n zero bytes is a multiplication by x^(8n) mod P.
#define ZT_CRC_POLY 0xEDB88320u

__host__ __device__ inline uint32_t multmodp(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) {
      p ^= b;
      if ((a & (m - 1)) == 0) break;
    }
    m >>= 1;
    b = (b & 1) ? (b >> 1) ^ ZT_CRC_POLY : b >> 1;
  }
  return p;
}

// x^(n * 2^k) mod P from a table of x^(2^k) (period 32)
__host__ __device__ inline uint32_t x2nmodp(const uint32_t *x2n, uint64_t n, unsigned k) {
  uint32_t p = 1u << 31;  // x^0
  while (n) {
    if (n & 1) p = multmodp(x2n[k & 31], p);
    n >>= 1;
    k++;
  }
  return p;
}

// RFC 1951 3.2.5 length / distance code arithmetic, ALU only (table lookups
// indexed by non-provably-uniform values become dependent global loads).
__host__ __device__ __forceinline__ uint32_t len_base(uint32_t ls) {  // ls = symbol - 257, 0..28
  if (ls < 8) return ls + 3;
  if (ls >= 28) return 258;
  uint32_t e = (ls >> 2) - 1;
  return ((4 + (ls & 3)) << e) + 3;
}
__host__ __device__ __forceinline__ uint32_t len_extra(uint32_t ls) {
  return (ls < 8 || ls >= 28) ? 0 : (ls >> 2) - 1;
}
__host__ __device__ __forceinline__ uint32_t dist_base(uint32_t ds) {  // 0..29
  if (ds < 4) return ds + 1;
  uint32_t e = (ds >> 1) - 1;
  return ((2 + (ds & 1)) << e) + 1;
}
__host__ __device__ __forceinline__ uint32_t dist_extra(uint32_t ds) { return ds < 4 ? 0 : (ds >> 1) - 1; }

// ---- deflate device pipeline ------------------------------------------------------
// What deflate.hip (classify, match, the host driver) and deflate_post.hip
// (price .. encode) share; inflate_seg.hip sizes its units from DF_BLOCK and
// DF_GROUP.
#ifdef ZT_DF_TIME
#define DF_T(v) v = __builtin_readcyclecounter()  // debug: phase cycles (g_df_time, g_bk_time)
#else
#define DF_T(v) (void)0
#endif
#ifndef ZT_DF_BLOCK
#define ZT_DF_BLOCK 32768
#endif
constexpr int DF_BLOCK = ZT_DF_BLOCK;
// DEFLATE blocks (one Huffman code, one header, one sync point) may span
// DF_GROUP consecutive 32 KiB parse blocks of a stream (compile option): the
// match / price / DP / parse kernels keep their 32 KiB granularity,
// block_kernel sums the group's histograms and encode_kernel writes the
// group's tokens as one block.  Inflate units are one DEFLATE block
// (inflate_seg.hip).  Measured at 4 (profiles/r03b_*): wordsalad ratio vs the
// reference 1.0168 -> 1.0145 only, but inflate 10.9 -> 12.2 ms per GiB
// (tokenize and expand get a quarter of the units): kept at 1.
#ifndef ZT_DF_GROUP
#define ZT_DF_GROUP 1
#endif
constexpr int DF_GROUP = ZT_DF_GROUP;
static_assert(DF_GROUP >= 1 && DF_GROUP <= 8 && (32 % DF_GROUP) == 0, "group divides a segment");
// per-block slot: the block's prices (price_kernel -> optparse_kernel), then
// its histograms and token count (parse_kernel -> block_kernel), then its
// dynamic header's complete words (block_kernel -> encode_kernel: at most
// 17 + 19 * 3 + 316 * 14 bits); the coded block itself goes straight into the stream
constexpr int DF_SLOT = 2048;
static_assert(DF_SLOT >= 321 * 4 && DF_SLOT * 8 >= 17 + 19 * 3 + 316 * 14, "slot holds histograms and a header");
// Independent segments of 1 MiB: restart points for segment-parallel inflate,
// each announced by a restart marker (two empty stored blocks, deflate_post.hip)
constexpr uint32_t kRestartBlocks = (1u << 20) / DF_BLOCK;  // 1 MiB
constexpr uint32_t kRestartMarkerLen = 10;

struct BlockPlan;

struct DeflateParams {
  const uint8_t *base;  // stream bytes are base[halo .. halo + n)
  uint64_t halo;
  uint64_t end;         // halo + n
  uint32_t blocks_per_wg;
  uint32_t big_wgs;     // match workgroups [0, big_wgs) take blocks_per_wg blocks, later ones tail_k
  uint32_t tail_k;
  uint32_t nblocks;
  uint32_t restart;     // blocks per independent segment (multiple of blocks_per_wg)
  uint32_t hist_max;    // history bytes a super-chunk loads (multiple of DF_SUB, <= DF_HIST)
  int final_;
  int max_chain;
  int nice_len;
  int lazy;
  int too_far;
  int good;             // a carried match this long cuts the chain walk to a quarter
  int skip_len;         // a carried match at least this long is taken without a search
  int klen;             // chain key length: 3, 4, 6 or 8 bytes (shorter matches come from near probes)
  int probe;            // near distances 1..probe checked for matches shorter than klen
  int ctype;            // 1: fixed codes only; 2: best of dynamic/fixed/stored
  int opt;              // cost-based parse (optparse_kernel) between match and block kernels
  // Per-block search depth (0: off): the block's first sub-chunk is searched
  // with max_chain hops and counts the improvements its walks found at hop
  // adapt_depth or later (and at hop adapt_depth2 or later); when the first
  // are at most adapt_thr per 4096 positions, the rest of the block walks
  // adapt_depth hops, else when the second are at most adapt_thr2,
  // adapt_depth2 hops (match_kernel)
  int adapt_depth, adapt_thr;
  int adapt_depth2, adapt_thr2;
  // Per-block candidate measurement (0: never queued): when the probe
  // sub-chunk measured at least mq_thr candidates per 4096 positions, the
  // rest of the block measures through the waves' queues (mq_pair_loop): the
  // same matches, found with fuller waves
  int mq_thr;
  // chain-head format of match_kernel: 0: per block (u16 while the block's
  // later sub-chunks measure through the queues, else u32), 16 / 32: that
  // format throughout (ZT_DF_HEADS; 32 queues nothing: the host clears mq_thr)
  int heads;
  // 1: parse_kernel and price_kernel walk the path window by window
  // (parse_block_regs) instead of lane-parallel (ZT_PARSE_SERIAL; the streams
  // do not depend on it)
  int parse_serial;
  // 1: match_kernel's link waves take whole groups of steps without bounds
  // selects and publish their progress without draining their LDS queue; 0:
  // the former link throughout (ZT_DF_LINK=0; the streams do not depend on it)
  int link;
  // the producer of res (include/zt_strategy.h): 0: match_kernel, else
  // ZT_STRATEGY_RLE / ZT_STRATEGY_HUFFMAN_ONLY: strategy_kernel
  // (deflate_strategy.hip), which reads none of the search parameters above
  int strategy;
  // batch of independent streams (zt_deflate_batch_dev): stream f occupies
  // whole blocks from a 32 KiB-aligned offset; per block the [start, end) of
  // its stream (relative to halo = 0), or null for one stream of n bytes
  const uint64_t *span;
  // per block: 1 = no match search, a stored block (classify_kernel: bytes
  // that cannot beat stored); null when not classified
  uint8_t *store;
  uint32_t *nstore;     // blocks flagged (one counter, zeroed before classify_kernel)
  uint32_t *res;        // n: per-position match, then (in place) per-block tokens
  uint8_t *slots;       // nblocks x DF_SLOT (prices, histograms, dynamic headers)
  uint32_t *slot_len;   // nblocks: each block's bytes (block_kernel's plan, exact)
  uint8_t *out;         // the stream: encode_kernel writes block b at out + boff[b]
  const uint64_t *boff; // exclusive scan of slot_len (+ restart markers), scan_sizes
  uint32_t *fault;      // encode_kernel: a block's bits differ from its plan
  BlockPlan *plans;     // nblocks
};

// per-block coding decisions (block_kernel -> encode_kernel)
struct BlockPlan {
  uint32_t lit_code[288];  // len << 16 | bit-reversed code
  uint32_t dist_code[32];
  uint32_t ntok;      // tokens of the group
  uint32_t btype;     // 0 stored, 1 fixed, 2 dynamic
  uint32_t hdr_bits;  // header bits (complete words already in the slot)
  uint32_t hdr_tail;  // bits [hdr_bits & ~31, hdr_bits) of the header, not yet stored
  uint32_t blen;      // input bytes of the group
  uint32_t last;
  uint32_t nsub;      // parse blocks in the group (<= DF_GROUP)
  uint32_t pad;
  uint32_t ntok_sub[8];  // tokens per parse block (in res at (leader + k) * DF_BLOCK)
};

// end of the stream block `blk` belongs to (relative to base + halo)
__device__ __forceinline__ uint64_t stream_end(const DeflateParams &P, uint32_t blk) {
  return P.span ? P.span[2 * (uint64_t)blk + 1] : P.end - P.halo;
}

// a DEFLATE block (group) starts at every DF_GROUP-th parse block of its
// stream (batch: counted from the stream's first block)
__device__ __forceinline__ bool group_leader(const DeflateParams &P, uint32_t blk) {
  const uint64_t first = P.span ? P.span[2 * (uint64_t)blk] / DF_BLOCK : 0;
  return ((blk - first) % DF_GROUP) == 0;
}
// parse blocks in the group led by `blk`
__device__ __forceinline__ uint32_t group_size(const DeflateParams &P, uint32_t blk) {
  const uint64_t lo = (uint64_t)blk * DF_BLOCK, n = stream_end(P, blk);
  const uint64_t nb = (n - lo + DF_BLOCK - 1) / DF_BLOCK;
  return nb < (uint64_t)DF_GROUP ? (uint32_t)nb : (uint32_t)DF_GROUP;
}

__device__ __forceinline__ uint64_t lanemask_lt(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

// Per-position match word in res (match_kernel -> price / optparse / parse):
// the byte at the position in bits 24-31 (so the later kernels never read
// the input again), the match length (0 or 3..258) in bits 15-23 and its
// distance (<= DF_MAXDIST < 2^15) in bits 0-14.  optparse_kernel rewrites the
// length with its choice (0 = literal).
__device__ __forceinline__ uint32_t res_pack(uint32_t byte, uint32_t len, uint32_t dist) {
  return (byte << 24) | (len << 15) | dist;
}
__device__ __forceinline__ uint32_t res_len(uint32_t r) { return (r >> 15) & 511u; }
__device__ __forceinline__ uint32_t res_dist(uint32_t r) { return r & 0x7FFFu; }
__device__ __forceinline__ uint32_t res_byte(uint32_t r) { return r >> 24; }

// The post-match stages (deflate_post.hip), launched on s in pipeline order:
// price -> optparse (P.opt) -> parse -> block -> scan_sizes -> encode.  boff is
// P.boff, writable: scan_sizes fills its nblocks + 1 entries.
int deflate_post_run(const DeflateParams &P, uint64_t *boff, hipStream_t s);

typedef __attribute__((address_space(1))) const uint8_t g_u8;
typedef __attribute__((address_space(1))) const uint32_t g_u32;

// nibble tables: 16 x 16 for slice-by-8, then 8 x 16 for the multiplication
// by x^(8 * 1024) (checksum.hip's coalesced lane streams)
#define ZT_CRC_NIB_N 384
void crc_host_tables(uint32_t byte_table[256], uint32_t nib[ZT_CRC_NIB_N], uint32_t x2n[32]);
// x^(8 L) mod P for the checksum kernels: [0, 264) unused, then
// ZT_CRC_DIGITS tables of 64 entries x^(8 v 64^d), then per thread of a whole
// segment the shift of its lane stream to the segment end
#define ZT_CRC_DIGITS 6
#define ZT_CRC_DIG_OFF 264
#define ZT_CRC_LANE_OFF (ZT_CRC_DIG_OFF + 64 * ZT_CRC_DIGITS)
#define ZT_CRC_SHIFT_N (ZT_CRC_LANE_OFF + 512)
void crc_shift_tables(const uint32_t x2n[32], uint32_t shift[ZT_CRC_SHIFT_N]);

// ---- launchers (device-resident) ------------------------------------------------
int checksums_dev(DeviceCtx *c, const uint8_t *d_in, size_t n, bool do_crc, bool do_adler, uint32_t crc_in,
                  uint32_t adler_in, uint32_t *d_result /* [2] */, hipStream_t s);
int checksums_batch_dev(DeviceCtx *c, const uint8_t *frame, size_t count, const uint64_t *off, const uint64_t *len,
                        uint32_t *d_result /* [2 count] */, hipStream_t s);
int current_device();                                                 // this thread's (zt_set_device)
std::vector<int> batch_devices();                                     // zt_set_devices, else {current}
// debug (deflate.hip; exported, not part of include/zt.h): blocks of the
// match kernel that measured their candidates through the queues (out[0]) and
// at once (out[1]) since the last call; reads and clears the device counter
extern "C" int zt_debug_match_modes(uint64_t out[2]);
// debug (deflate.hip): the match stage's result for one stream, n > 0 bytes at
// in + halo with halo <= 32768 bytes of history in front (in holds halo + n
// bytes; `level` as zt_deflate_opts.level, compressionType DYNAMIC).  Runs what
// deflate_dev_run runs up to and including match_kernel -- the same geometry,
// scratch, parameters (environment hooks included) and launches
// (deflate_stream_call, deflate_match_launch) -- over a res filled with
// 0xFFFFFFFF (length 511, which no position can hold: a position the kernel
// never wrote stays visible).  res[n]: the per-position match words
// (res_pack); store[ceil(n / DF_BLOCK)]: classify_kernel's flags (a flagged
// block's positions are not searched); info[kDebugMatchInfo]: the constants
// and the parameters the call used, in this order: DF_BLOCK, DF_SUB,
// DF_MAXDIST, segment bytes, blocks per workgroup, max_chain, nice_len,
// skip_len, good, klen, probe, too_far, ZT_DF_P4FAR, adapt_depth, adapt_thr,
// adapt_depth2, adapt_thr2, mq_thr, blocks, match workgroups
constexpr int kDebugMatchInfo = 20;
extern "C" int zt_debug_match(const uint8_t *in, size_t n, size_t halo, int level, uint32_t *res, uint8_t *store,
                              uint32_t *info);
// debug (deflate.hip): zt_debug_match with a strategy (include/zt_strategy.h):
// the same contract and the same info record; with ZT_STRATEGY_RLE or
// ZT_STRATEGY_HUFFMAN_ONLY the launch is strategy_kernel's, exactly as the
// strategy calls launch it (it writes flagged blocks too: no word stays
// 0xFFFFFFFF); ZT_E_ARG for any other strategy
extern "C" int zt_debug_match_strategy(const uint8_t *in, size_t n, size_t halo, int level, int strategy,
                                       uint32_t *res, uint8_t *store, uint32_t *info);
// The strategies' producer of res (deflate_strategy.hip), launched by
// deflate_match_launch in place of match_kernel when P.strategy != 0: one
// workgroup per block, every block written (flagged ones too)
int deflate_strategy_launch(const DeflateParams &P, hipStream_t s);
// debug (deflate.hip): match workgroups that changed their chain heads from
// u32 to u16 (out[0]) and from u16 to u32 (out[1]) since the last call; reads
// and clears the device counter
extern "C" int zt_debug_head_formats(uint64_t out[2]);
// debug (deflate_post.hip): block_kernel's huff_lengths and huff_codes on
// `count` histograms of n <= 286 frequencies each (freqs[count * n]), one wave
// per histogram: code lengths limited to `limit` (7 or 15; 2^limit >= n) in
// lens[count * n], len << 16 | bit-reversed canonical code (0: unused) in
// codes[count * n].  ZT_E_ARG for a frequency of 2^23 or more (the sort key is
// freq << 9 | symbol) or a histogram summing to 2^27 or more (package weights
// are 32-bit sums); block_kernel's own histograms sum to a block's tokens
extern "C" int zt_debug_huffman(const uint32_t *freqs, uint32_t count, uint32_t n, uint32_t limit, uint8_t *lens,
                                uint32_t *codes);
// deflate (deflate.hip): one stream of n bytes at d_in (halo bytes of history
// in front of it, final_: the last call of the stream) in one pipeline;
// scratch of deflate_scratch_bytes(n), output of at most deflate_bound_bytes(n)
size_t deflate_bound_bytes(size_t n);
size_t deflate_segment_bytes();
size_t deflate_scratch_bytes(const DeviceCtx *c, size_t n);
// The deflate-time index of one deflate_dev_run call (include/zt_index.h; the
// arithmetic: deflate_index_host.h): deflate_index_kernel, launched behind
// encode_kernel, writes the call's dix_call_units entries (a final call: and
// the sentinel) to d_ent; `cap` is that count exactly (dix_layout).  in_base: where the call's
// first stream byte will lie in the caller's buffer; out_base: the output
// offset of its first input byte.  n > 0 and a compressing ctype only.
struct DeflateIndexReq {
  IdxEntry *d_ent;
  uint64_t cap;
  uint64_t in_base, out_base;
};
int deflate_index_launch(const DeflateParams &P, const DeflateIndexReq &ix, hipStream_t s);  // deflate_index.hip
// bits of DeflateParams::fault
constexpr uint32_t kFaultEncode = 1;  // encode_kernel: a block's bits differ from its plan
constexpr uint32_t kFaultIndex = 2;   // deflate_index_kernel: the entry layout disagrees with restart_after
int deflate_dev_run(DeviceCtx *c, const uint8_t *d_in, size_t n, size_t halo, int final_, int ctype, int level,
                    uint8_t *d_out, size_t *out_len, void *scratch_base, size_t scratch_size, hipStream_t s,
                    const DeflateIndexReq *ix = nullptr);
// The host side of a stream's deflate-time index (deflate_api.cpp), shared by
// the raw and the container calls: the table of a stream written as pieces of
// `sizes` input bytes (one piece: a one-call deflate) in scratch slot
// kDeflateIndex; piece i's request for deflate_dev_run (stream_pos: the
// stream bytes written before the piece; input_pos: its first input byte);
// and, once the stream is complete, the table's one download into a blob
// (zt_free) with its header, checked by index_validate.
struct DeflateIndexTable {
  DixLayout L;
  IdxEntry *d_ent = nullptr;
  uint64_t stream_start = 0;
};
int deflate_index_begin(DeviceCtx *c, const std::vector<size_t> &sizes, uint64_t stream_start, DeflateIndexTable *t);
DeflateIndexReq deflate_index_piece(const DeflateIndexTable &t, size_t i, uint64_t stream_pos, uint64_t input_pos);
int deflate_index_finish(DeviceCtx *c, const DeflateIndexTable &t, uint64_t stream_len, uint64_t total_out,
                         uint8_t **idx, size_t *idx_len, hipStream_t s);
// The indexed calls' refusal, before any device work, of a stream without
// sync points: stored blocks only (NONE, level 0), or the empty input's one
// empty stored block -- zt_inflate_index_build finds no sync point in that
// stream either, and the writers answer as it does.  ZT_OK: indexable.
int deflate_index_refuse(int ctype, size_t n);
// batch deflate (deflate.hip): streams packed at 32 KiB boundaries, one pipeline
size_t deflate_batch_scratch_bytes(const DeviceCtx *c, size_t padded);
// a preset dictionary as the match kernel reads it (dict_host.h: dict_layout):
// d_hist[0 .. hist) on the device, 4-byte aligned, data from `floor` on
struct DictHist {
  const uint8_t *d_hist;
  uint32_t hist, floor;
};
int deflate_batch_dev_run(DeviceCtx *c, const uint8_t *d_in, size_t count, const uint64_t *off, const uint64_t *len,
                          int ctype, int level, uint8_t *d_out, uint64_t *out_off, void *scratch_base,
                          size_t scratch_size, hipStream_t s, const DictHist *dict = nullptr);
// The compute step of every member writer: with d_sums, checksums_batch_dev
// over the packed input on c->aux, forked behind `landed` (null: behind what
// c->stream holds now) and c->aux_ev recorded on c->aux behind it; with a
// compressing ctype, deflate_batch_dev_run on c->stream.  join_sums: c->stream
// waits for those sums (the trailers need them).
int deflate_members_dev(DeviceCtx *c, const uint8_t *d_in, size_t count, const uint64_t *off, const uint64_t *len,
                        int ctype, int level, uint8_t *d_body, uint64_t *out_off, void *scratch_base,
                        size_t scratch_size, const DictHist *dict, uint32_t *d_sums, hipEvent_t landed);
inline int join_sums(DeviceCtx *c) {
  ZT_HIP(hipStreamWaitEvent(c->stream, c->aux_ev, 0));
  return ZT_OK;
}
// host dictionary (dict_api.cpp / batch_api.cpp): the batch deflate calls with
// one dictionary for every buffer (dict_len == 0: none), framed as `fr`
// (frame_raw, or frame_zlib_dict with the dictionary's Adler-32)
struct HostDict {
  const uint8_t *dict = nullptr;
  size_t dict_len = 0;
};
int deflate_batch_host(const uint8_t *const *in, const size_t *n, size_t count, const zt_deflate_opts *opts,
                       const HostDict &hd, const MemberFrame &fr, uint8_t **out, size_t *out_len, int *status);
// host streams decoded by one wave each with `hist_len` <= 32768 bytes of
// device history d_hist in front of every stream (inflate_api.cpp)
int inflate_host_batch_hist(const uint8_t *const *in, const size_t *n, const size_t *index, size_t count,
                            const uint8_t *d_hist, uint32_t hist_len, uint8_t **out, size_t *out_len, size_t *end_ip,
                            int *status);

// device-resident streams (stream i at d_in + in_off[i], n[i] bytes, decoded
// from index[i]) through the batch decoder -- two-phase, then one wave per
// stream; with hist_len the one-wave decoder only, the history in front of
// every stream (inflate_api.cpp).  Outputs are library memory (zt_free).
// extras (optional): what the container batch calls need beside the bytes.
struct BatchExtras {
  uint32_t *sums = nullptr;  // [2 count]: CRC-32 and Adler-32 of every finished output, from its device copy
  int *detail = nullptr;     // [count]: inflate_error's second argument for status[i]
  // [count] or null: a stream with speculative[i] != 0 that the two-phase pass
  // cannot finish is not decoded again by one wave; it gets ZT_E_INPUT_BROKEN,
  // which is then no more than "failed" (not the reference's status)
  const uint8_t *speculative = nullptr;
  // The device sink (zt_inflate_dev_batch, dev_batch_api.cpp): finished
  // outputs are not downloaded.  Both decoder routes hand every batch of
  // finished streams to sink->put while their bytes still lie in the decode
  // buffer; out[i] stays null and out_len[i] is the stream's length.  With a
  // sink and no sums, batches of fewer than 8 streams go to the one-wave
  // decoder as the host call's do.
  const struct DevSink *sink = nullptr;
};
// a finished stream: `len` bytes at d_base + off belong to item `item`
struct SinkPiece {
  size_t item;
  uint64_t off, len;
};
struct DevSink {
  // queues the copies on s (ordered behind the decode); the pieces' bytes may
  // be overwritten by whatever s runs next
  std::function<int(const uint8_t *d_base, const std::vector<SinkPiece> &pieces, hipStream_t s)> put;
};
// the copy jobs' tiles (dev_batch.hip) and the patch jobs (member_frame.hip),
// tables (dev_batch_plan.h) on the device
int dev_copy_dev(const DevCopyJob *d_jobs, uint32_t njobs, uint64_t tiles, hipStream_t s);
int dev_patch_dev(const DevPatchJob *d_jobs, uint32_t njobs, const uint32_t *d_sums, hipStream_t s);
// Decode `count` device-resident streams (stream i at d_in + in_off[i],
// n[i] bytes, from index[i]); outputs are malloc'd.
int inflate_batch_dev_streams(DeviceCtx *c, const void *d_in, const std::vector<size_t> &in_off, const size_t *n,
                              const size_t *index, size_t count, uint8_t **out, size_t *out_len, size_t *end_ip,
                              int *status);
int inflate_batch_dev_streams_ex(DeviceCtx *c, const void *d_in, const std::vector<size_t> &in_off, const size_t *n,
                                 const size_t *index, size_t count, uint8_t **out, size_t *out_len, size_t *end_ip,
                                 int *status, const uint8_t *d_hist, uint32_t hist_len, const BatchExtras *extras);

// candidate gzip member starts of a packed batch (container.hip)
struct MemberCand {
  uint64_t off;   // offset in its item (> 0: the host adds every item's offset 0)
  uint32_t item;
  uint32_t pad;
};
int find_members_dev(const uint8_t *d_in, uint64_t total, const uint64_t *d_item_off, const uint64_t *d_item_len,
                     uint32_t count, MemberCand *d_list, uint32_t cap, uint32_t *d_found, hipStream_t s);

// ---- inflate jobs (one stream per wavefront) -----------------------------------
struct InfJob {
  const uint8_t *in;  // whole input array (RawInflate's `input`)
  uint64_t n;         // its length
  uint64_t start;     // RawInflate `index`
  uint8_t *out;       // output buffer (device)
  uint64_t cap;       // output capacity; decoding continues past it, counting only
  int32_t strict;     // stop with 'input buffer is broken' where the reference's EOF test throws
  int32_t resume;     // on an error, still write the output of the blocks that decoded completely
  uint32_t start_bit;      // resume: bits of in[start] already used
  uint32_t hist_len;       // resume: output already produced (match history), <= 32 KiB ...
  const uint8_t *hist;     // ... its bytes (device); `out` receives only the new bytes
  uint32_t stop_first;        // segment decode: first candidate index to test
  const uint64_t *stops;      // sorted segment starts (byte positions in `in`), or null
  uint64_t stop_count;
};

struct InfResult {
  uint64_t out_len;     // bytes produced (may exceed cap)
  uint64_t end_ip;      // reference .ip after decompress
  int32_t status;
  int32_t detail;       // code length / BTYPE for the message
  int32_t strict_fail;  // reference's readBits EOF check would throw
  int32_t stop_idx;     // segment decode: index of the segment start where decoding stopped, -1 at BFINAL
  // resumable decode (zt_inflate_raw_resume): the bit position (relative to
  // `in`) right after the last block that decoded completely and the output
  // length there; the reader's bit position when decoding stopped
  uint64_t blk_bits;
  uint64_t blk_op;
  uint64_t stop_bits;
};

// segment-parallel inflate (restart markers written by deflate); returns 1 when
// the stream has no usable segments (caller decodes it with one wave)
// (*d_out_io null: the output goes to scratch slot kOut, returned in *d_out_io;
// a caller-owned output too small for the stream: ZT_E_ARG with *out_len = the
// bytes it needs).  boundary (a byte position, or ~0: none): the decode must
// have a block boundary there -- a unit of the chain starts at it -- or the
// call returns 1 (the pipelined host inflate's certificate that a cut is a
// real block boundary of the whole stream)
int inflate_segments_dev(DeviceCtx *c, const uint8_t *d_in, size_t n, size_t index, uint8_t **d_out_io,
                         size_t out_cap, size_t *out_len, size_t *end_ip, hipStream_t s, uint64_t boundary = ~0ull);
// The index build (include/zt_index.h): the stages of inflate_segments_dev
// with no minimum stream size, the chain always walked on the host and the
// output library-owned (kOut, returned in *d_out); after expand and copy have
// proved the chain, index_pack_kernel packs the on-chain units and *blob
// receives the finished index.  Returns 0, 1 or 2 (the stream is off the
// sync-point path: no index) or a negative status.
int inflate_index_build_dev(DeviceCtx *c, const uint8_t *d_in, size_t n, size_t index, uint8_t **d_out,
                            size_t *out_len, size_t *end_ip, std::vector<uint8_t> *blob, hipStream_t s);
// The large-stream cascade (inflate_api.cpp): the segment path, then -- unless
// allow_general is false or the segment path returned 2 (its chain ran out of
// input: the general path cannot finish either) -- the general path.  A
// library-owned output (*d_out_io null on entry) is reset between the two:
// the segment path may have placed one before it gave up, and with that
// pointer and no capacity the general path would refuse the stream.  A
// caller-owned output is never reset.  Returns 0, 1 (decode with one wave), 2
// or a negative status, as the two paths do.
int inflate_parallel_dev(DeviceCtx *c, const uint8_t *d_in, size_t n, size_t index, uint8_t **d_out_io,
                         size_t out_cap, size_t *out_len, size_t *end_ip, hipStream_t s, uint64_t boundary = ~0ull,
                         bool allow_general = true);

// ---- two-phase token inflate (inflate_tok.hip) ----------------------------------
// (TokJob, TokResult, ChainUnit, SegJob, ChainInfo: inflate_chain.h)
struct TokParams {
  const uint8_t *in;
  uint64_t n;
  const uint32_t *order;  // workgroup g decodes unit order[g] (null: unit g)
  const uint64_t *stops;  // sorted sync points
  uint64_t nstops;
  const TokJob *jobs;
  TokResult *res;
  uint32_t *tokens;
  uint32_t count;
  int simt;           // 0: one-lane (scalar) body decode only
  uint64_t *dbg;      // debug: per unit 8 words comparing the SIMT and scalar body decodes, or null
  uint32_t dump_unit; // debug: unit whose first SIMT block dumps per-round lane state after dbg[count * 8]
  uint32_t dump_once;
  // stored payloads of >= kStoredRunMin bytes become three *run tokens*
  // (len << 16 with distance 0, then the payload's input offset, low and high
  // words) whose literal descriptors expand_kernel writes straight from the
  // input; 0: the tokenizer writes a literal token per stored byte
  int run_tokens;
};
struct ResolveParams {
  const uint32_t *tokens;
  const ChainUnit *units;
  const SegJob *segs;
  uint8_t *out;
  uint16_t *desc;        // one descriptor per output byte (expand -> copy)
  int32_t *unit_status;  // expand
  int32_t *seg_status;   // copy
  uint32_t nunits;
  uint32_t nseg;
  int32_t marker;        // expand: segments after the first may reach up to 32 KiB behind their start
  const uint8_t *in;     // expand: the compressed input (payloads of run tokens)
  const ChainInfo *info = nullptr;  // device-built chain: nothing to do unless info->ok; nseg = info->nseg
  const uint32_t *order = nullptr;  // expand: workgroup g takes unit order[g] (null: unit g)
};
// TokParams::simt of every caller: ZT_TOK_SIMT=0 selects the one-lane body decode (A/B)
inline int tok_simt_env() {
  static const char *e = getenv("ZT_TOK_SIMT");
  return e ? atoi(e) != 0 : 1;
}
// `count` units planned on the host (the range calls): every unit's job is
// uploaded, no launch order, no debug words, stored runs as run tokens
inline TokParams tok_params_planned(const uint8_t *in, uint64_t n, const uint64_t *stops, uint64_t nstops,
                                    const TokJob *jobs, TokResult *res, uint32_t *tokens, uint32_t count) {
  TokParams tp;
  tp.in = in;
  tp.n = n;
  tp.order = nullptr;
  tp.stops = stops;
  tp.nstops = nstops;
  tp.jobs = jobs;
  tp.res = res;
  tp.tokens = tokens;
  tp.count = count;
  tp.simt = tok_simt_env();
  tp.dbg = nullptr;
  tp.dump_unit = 0xFFFFFFFFu;
  tp.dump_once = 0;
  tp.run_tokens = 1;
  return tp;
}
int tokenize_units_dev(const TokParams &p, hipStream_t s);
int resolve_segments_dev(const ResolveParams &p, hipStream_t s);
int expand_units_dev(const ResolveParams &p, hipStream_t s);
// One requested range with bytes (the range calls: range_call.h, bgzf_api.hip):
// dec[src .. src + len) -> out[dst ..]; its tiles are workgroups [tile0, tile0
// + ceil(len / kGatherTile)) of range_gather_kernel (range_call.hip), which
// does nothing unless info->ok.
struct RangeJob {
  uint64_t src, dst, len;
  uint32_t tile0, pad;
};
constexpr uint32_t kGatherTile = 32768;
// the next job of a call's list; *tiles: the workgroups so far (the caller
// holds them to 0x7FFFFFFF before the launch)
inline void range_job_add(std::vector<RangeJob> &jobs, uint64_t *tiles, uint64_t src, uint64_t dst, uint64_t len) {
  jobs.push_back(RangeJob{src, dst, len, (uint32_t)*tiles, 0});
  *tiles += (len + kGatherTile - 1) / kGatherTile;
}
// a status slot nobody has written (the verify kernels of the range calls set
// it; expand / copy returned at once)
constexpr int32_t kNotRun = 1;
int range_gather_dev(const RangeJob *d_jobs, uint32_t njobs, uint32_t tiles, const uint8_t *d_dec, uint8_t *d_out,
                     const ChainInfo *d_info, hipStream_t s);
// expand_kernel (p.marker = 1), then copy_window_kernel: segment g's 32 KiB
// history ring starts as the 32768 bytes at wins + 32768 * seg_win[g]
// (seg_win[g] < 0: the stream's first segment, no history) -- the checkpoint
// range decode (ckpt_api.hip)
int resolve_segments_window_dev(const ResolveParams &p, const uint8_t *wins, const int32_t *seg_win, hipStream_t s);

// A chain buffer, in a device scratch slot or its mirror in pinned staging:
// [chain units | segment jobs | extra | unit statuses | segment statuses | tail]
// (extra: the general path's GenSeg table; tail: the device chain's ChainInfo
// and boundary flag, read back with the statuses in one copy).
struct ChainBuf {
  ChainUnit *units;
  SegJob *segs;
  uint8_t *extra;
  int32_t *unit_status;
  int32_t *seg_status;
  uint8_t *tail;
  size_t bytes;  // all of it
};
inline ChainBuf chain_buf(void *base, size_t units, size_t segs, size_t extra_bytes = 0, size_t tail_bytes = 0) {
  Carve cv(base);
  ChainBuf b;
  b.units = cv.take<ChainUnit>(units);
  b.segs = cv.take<SegJob>(segs);
  b.extra = cv.take<uint8_t>(extra_bytes);
  b.unit_status = cv.take<int32_t>(units);
  b.seg_status = cv.take<int32_t>(segs);
  b.tail = cv.take<uint8_t>(tail_bytes);
  b.bytes = cv.bytes();
  return b;
}
// A host-built chain on its way through the resolve kernels (inflate_resolve.cpp).
struct ChainRun {
  // dev: in a scratch slot.  host: its mirror in kPinInflateMeta, set by
  // resolve_chain_dev alone (chain_statuses needs it); general_dev, which
  // keeps its own transfers, leaves it empty
  ChainBuf dev, host;
  uint32_t nunits, nseg;
};
ResolveParams resolve_params(const ChainRun &run, const uint32_t *tokens, uint16_t *desc, uint8_t *out,
                             int32_t marker, const uint8_t *in);
// resolve_chain_dev: carves kChain and the mirror, copies chain and segments
// to the device (x_copy from the mirror), takes descriptors for desc_total
// output bytes in kDeflateOrDesc, then expand and copy (resolve_segments_dev).
// pin_front: bytes at the front of kPinInflateMeta that the caller still
// reads (it has sized the slot for both, so the slot does not move).
int resolve_chain_dev(DeviceCtx *c, const std::vector<ChainUnit> &chain, const std::vector<SegJob> &segs,
                      uint64_t desc_total, const uint32_t *tokens, uint8_t *out, int32_t marker, const uint8_t *in,
                      size_t pin_front, ChainRun *run, hipStream_t s);
// chain_statuses: both status arrays into the mirror (run.host.unit_status /
// seg_status), then waits for the stream.
int chain_statuses(const ChainRun &run, hipStream_t s);
// debug (inflate_seg.hip; exported, not part of include/zt.h): chain_kernel on
// host tables of `units` units (restart: units - 1 flags) with the given
// capacities; info, and when info->ok the `units` chain units and info->nseg
// segment jobs, come back (cu: room for units, sj: for max_seg)
extern "C" int zt_debug_chain(const TokResult *res, const uint8_t *restart, const uint64_t *tok_off, uint32_t units,
                              uint64_t out_cap, uint64_t desc_cap, uint32_t max_seg, ChainInfo *info, ChainUnit *cu,
                              SegJob *sj);
// debug: seg_chain_host on the same tables, in the same shape (cu and sj: room
// for `units`; *nchain: units on the chain; *outcome: ChainPlan::Outcome)
extern "C" int zt_debug_chain_host(const TokResult *res, const uint8_t *restart, const uint64_t *tok_off,
                                   uint32_t units, ChainInfo *info, ChainUnit *cu, SegJob *sj, uint32_t *nchain,
                                   int *outcome);

// ---- general speculative inflate (inflate_gen.hip) ---------------------------------
// A stream without sync points is cut at fixed bit positions; each *unit* is
// decoded by one wave from a start state that is exact (the stream start, a
// redo) or guessed (a candidate block header, a stored block's LEN field, or
// a position inside a block whose header is guessed), up to a stop position.
enum : uint32_t { GK_BLOCK = 0, GK_HUFF = 1, GK_STORED = 2, GK_SHDR = 3, GK_FINAL = 4 };
struct GenState {
  uint64_t pos;     // bit position relative to `in`
  uint64_t hdr;     // GK_HUFF: bit position of the block's header
  uint32_t kind;    // GK_*: a block start, a token start inside a Huffman body,
                    // a byte inside a stored payload, a stored LEN field, the end
  uint32_t rem;     // GK_STORED: payload bytes left
  uint32_t bfinal;  // GK_STORED / GK_SHDR: the block is the last one
  uint32_t pad;
};
struct GenJob {
  GenState st;       // start state
  uint64_t stop;     // the unit ends at the first block / token / payload byte at or after this bit (~0: none)
  uint64_t tok_off;  // token slot
  uint32_t tok_cap;
  uint32_t spec;     // guessed start: record the path's first token starts
};
struct GenResult {
  GenState end;        // state where the unit stopped (GK_FINAL: the stream ended)
  uint64_t out_len;    // bytes its tokens produce
  uint64_t dec_start;  // bit where the recorded token path starts
  uint64_t tab_id;     // tables of that path: its block's header position, or kFixedHdr
  uint64_t out_stop;   // bytes of the tokens before the end state
  uint32_t ntok;       // tokens, including the overlap decoded past the end state
  uint32_t ntok_stop;  // tokens before the end state
  int32_t status;
  int32_t detail;
  uint32_t recorded;   // the token-start bitmap of the first round is valid
  uint32_t tab_final;  // BFINAL of that path's block
  uint32_t tail_ok;    // an overlap past a GK_HUFF end state was decoded (its token starts recorded)
  uint32_t pad;
};
// GenState::hdr of a fixed-code block: every fixed block has the same tables
constexpr uint64_t kFixedHdr = 1ull << 62;
struct GenLink {       // unit k against unit k-1's end state
  uint64_t bytes;      // output bytes of unit k's tokens before the join
  uint64_t prev_bytes; // output bytes of unit k-1's tokens before the join
  uint32_t ok;         // 1: unit k continues unit k-1's path
  uint32_t t;          // unit k's first token on the joint path
  uint32_t prev_cut;   // unit k-1's tokens before the join
  uint32_t pad;
};
struct GenSeg {        // copy segment of the general path
  uint64_t base16;     // its u16 output (byte or window marker) in the staging array
  uint64_t out_off;    // final output offset
  uint64_t len;
};
int inflate_general_dev(DeviceCtx *c, const uint8_t *d_in, size_t n, size_t index, uint8_t **d_out_io,
                        size_t out_cap, size_t *out_len, size_t *end_ip, hipStream_t s);

// The checkpoint build (include/zt_checkpoint.h, ckpt_api.hip): the general
// path with its converged chain kept -- *entries receives one entry per unit
// boundary (positions, kinds, output offsets, token counts; windows not yet
// placed) and the sentinel; the output is library-owned (kOut, in *d_out).
// Returns as inflate_general_dev does.
struct CkEntry;
int inflate_general_ckpt_dev(DeviceCtx *c, const uint8_t *d_in, size_t n, size_t index, uint8_t **d_out, size_t *out_len,
                             size_t *end_ip, std::vector<CkEntry> *entries, hipStream_t s);
// gen_tokenize_kernel over `count` units that all start exactly (spec = 0), one
// wave each, without the overlap past a stop: a unit's token slot need only
// hold its own tokens
int gen_tokenize_exact_dev(const uint8_t *d_in, uint64_t n, const GenJob *d_jobs, GenResult *d_res, uint32_t *d_tokens,
                           uint32_t count, hipStream_t s);

int inflate_jobs_dev(const InfJob *d_jobs, InfResult *d_res, int count, hipStream_t s);
// one device-resident stream from `index`, output malloc'd (inflate_api.cpp)
int inflate_dev_member(DeviceCtx *c, const uint8_t *d_in, size_t n, size_t index, uint8_t **out, size_t *out_len,
                       size_t *end_ip);
// host -> device copy of n bytes: large buffers through two pinned staging
// chunks (parallel memcpy overlapped with the DMA), small ones directly
int upload(DeviceCtx *c, void *d_dst, const void *h_src, size_t n, hipStream_t s);
// device -> host, the same way; returns after the bytes are in h_dst
int download(DeviceCtx *c, void *h_dst, const void *d_src, size_t n, hipStream_t s);
// Three-stage host pipeline over np pieces, three engines busy at once: piece
// i + 1 crosses PCIe to the device (pinned chunks, stream c->up, one host
// thread) while compute(i) runs on the caller's thread (after piece i's upload
// has landed; it returns the device bytes of its result) and piece i - 1's
// result comes back (stream c->dn, one host thread: straight into a
// registered pool buffer by DMA, else through pinned chunks) to out.base +
// the sum of the earlier results' lengths.
struct PipePiece {
  const void *h_src;  // host bytes of piece i
  void *d_dst;        // where they go on the device
  size_t n;
};
struct PipeOut {
  // host output of `cap` bytes; null: the download stage takes a pooled
  // host_out(cap_fn()) once piece 0 is computed (cap_fn may look at it).  A
  // result that does not fit moves the bytes so far into a larger buffer.  On
  // return -- error or not, every copy finished -- `base` is the caller's.
  uint8_t *base = nullptr;
  size_t cap = 0;
  std::function<size_t()> cap_fn;
  size_t total = 0;  // out: bytes written
  // set by the pipeline for compute(i): drain(j), j < i, makes the compute
  // stream wait until piece j's result has left the device (before compute
  // reuses its device buffer); waits on the host until that copy is issued.
  // Only pieces from drain_from on can be drained: compute sets it (before
  // it returns piece drain_from) when it starts reusing buffers -- an event
  // recorded behind every download cost the inflate pipeline ~3 ms per GiB
  // (gpurun_out/r06u).
  std::function<int(size_t)> drain;
  size_t drain_from = SIZE_MAX;
};
int pipeline_h2d_d2h(DeviceCtx *c, size_t np, const std::function<PipePiece(size_t)> &input,
                     const std::function<int(size_t, const void **d_res, size_t *n_res)> &compute, PipeOut &out);
// The skeleton of a three-stage host pipeline over np pieces (xfer.cpp): run()
// calls up(i) and dn(i) in order on a thread each (the context's device
// current) and compute(i) on the caller's.  up(i) enqueues piece i's upload
// on c->up; the pipeline records landed(i) behind it and makes c->stream wait
// for it before compute(i); dn(i) runs once compute(i) has returned.  The
// first stage to fail stops the others, and its code and message are the
// caller's (zt_last_error_message() on the caller's thread).  On every
// return after the threads started, c->up, c->dn, c->aux and c->stream are
// drained: nothing still reads the caller's input or staging, or writes its
// output.  Users: pipeline_h2d_d2h, the grouped batch (batch_api.cpp).
class StagePipe {
 public:
  typedef std::function<int(size_t)> Stage;
  StagePipe(DeviceCtx *c, size_t np) : c_(c), np_(np) {}
  ~StagePipe();
  int run(const Stage &up, const Stage &compute, const Stage &dn);
  hipEvent_t landed(size_t i) const { return landed_[i]; }
  // waits until dn(j) has returned; false: the pipeline stopped
  bool wait_downloaded(size_t j) { return wait(downloaded_, j); }
  std::function<void(const char *)> trace;  // "joined", "drained" (measurement only)

 private:
  void fail(int rc);
  bool stopped();
  bool wait(const size_t &counter, size_t i);
  void done(size_t &counter, size_t i);
  DeviceCtx *c_;
  size_t np_;
  std::mutex mu_;
  std::condition_variable cv_;
  // pieces whose upload is enqueued / whose result is on the device / whose
  // download stage has returned
  size_t uploaded_ = 0, computed_ = 0, downloaded_ = 0;
  int err_ = 0;
  std::string err_msg_;
  std::vector<hipEvent_t> landed_;
};

// ---- the host batch layer (host_batch.cpp; its arithmetic: batch_plan.h) ----------
// Waits for a stream on every return of its scope (the checksums on c->aux
// beside a deflate pipeline: both read the input, so neither may outlive it)
struct AuxWait {
  hipStream_t s;
  ~AuxWait() { (void)hipStreamSynchronize(s); }
};
inline size_t deflate_out_bound(int ctype, size_t n) { return deflate_out_bound(ctype, n, deflate_bound_bytes(n)); }
// resolve_deflate_opts with the reference's message set.  The internal level
// it returns carries the calling thread's strategy (StrategyScope) above the
// level's four bits: every call site passes the (ctype, level) pair on as it
// is, and deflate_params -- the one reader -- takes the two apart again.
int resolve_opts(const zt_deflate_opts *o, int *ctype, int *level);
inline int level_with_strategy(int level, int strategy) { return (level & 15) | (strategy << 4); }
inline int level_plain(int level) { return level & 15; }
inline int level_strategy(int level) { return level >> 4; }
// ZT_E_ARG "invalid strategy: N" unless `strategy` is one of include/zt_strategy.h's
int strategy_check(int strategy);
// The strategy entry points (strategy_api.cpp) are the plain ones run inside
// this scope: resolve_opts on this thread hands out levels with the strategy.
class StrategyScope {
 public:
  explicit StrategyScope(int strategy);
  ~StrategyScope();
  StrategyScope(const StrategyScope &) = delete;
  StrategyScope &operator=(const StrategyScope &) = delete;

 private:
  int prev_;
};
// The batch devices a call of `count` items spreads over: the first
// min(devices, count) of batch_devices(), at least one.
std::vector<int> fanout_devices(size_t count);
// fn(d, context of devs[d], shares[d]) for every non-empty share: on the
// caller's thread when there is one share, else on a thread each, with that
// device current and its context locked.  Each share's code and -- read in
// one place, on its thread -- message come back; the caller's device is
// restored.  With several shares the host's copy threads (parallel_copy;
// ZT_BATCH_COPY_THREADS in all, default 32) are split between the threads.
std::vector<ShareResult> for_each_device(const std::vector<int> &devs, const std::vector<std::vector<size_t>> &shares,
                                         const std::function<int(size_t, DeviceCtx *, const std::vector<size_t> &)> &fn);
// Items `ids` of (in, n) packed by layout L (pack_layout) into the pinned batch
// staging and uploaded to scratch slot kIn (*d_in) on c->stream: in chunks of
// about 32 MiB as they are packed (the copy engine moves chunk k while the
// host packs chunk k + 1), or all at once.
struct PackMode {
  bool zero_pad;   // the bytes between an item's end and the next 32 KiB boundary zeroed (L aligned to 32768)
  bool chunked;
  size_t copy_bytes = 0;      // parallel_copy's thread budget; 0: L.total
  double *pack_ms = nullptr;  // += the host's packing time
};
int pack_upload(DeviceCtx *c, const uint8_t *const *in, const size_t *n, const std::vector<size_t> &ids,
                const PackLayout &L, const PackMode &mode, void **d_in);
// the packing alone: items [a, b) of the layout to stage + L.off[k] - L.off[a]
void pack_items(uint8_t *stage, const uint8_t *const *in, const size_t *n, const std::vector<size_t> &ids,
                const PackLayout &L, size_t a, size_t b, bool zero_pad, size_t copy_bytes);
int inflate_error(int status, int detail);

}  // namespace zt
