// dev_batch_plan.h -- the arithmetic of the device-resident batch calls
// (include/zt_dev_batch.h), no HIP: the copy jobs and their tile table for the
// gather and scatter kernels (dev_batch.hip), the patch jobs (prefixes,
// trailers, stored-block headers: member_frame.h's bytes, written by
// member_frame.hip's dev_patch_kernel), the stored-block job list of compression
// type NONE, the output bound, the groups a large batch is cut into and the
// capacity masking.  Pointers are carried as integers and never dereferenced
// here.  Pure functions, checked on the CPU under ASan / UBSan by
// tools/dev_batch_host_check.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "batch_plan.h"
#include "member_frame.h"

namespace zt {

// One workgroup of dev_copy_kernel moves one tile of one job.  32 KiB: the
// deflate pipeline's grid, so the zeroed tail of an item's last cell lies in
// the tile that holds its last byte; 256 threads x 8 stores of 16 bytes.
constexpr uint32_t kDevTile = 32768;
// the launcher's grid limit (as range_gather_dev's callers hold theirs)
constexpr uint64_t kDevMaxTiles = 0x7FFFFFFFull;
// A batch is cut into groups of at most this many packed input bytes (an item
// larger than it is a group of its own): what bounds a call's device memory
// for any count (zt_dev_batch.h states the bound).
constexpr uint64_t kDevGroupBytes = 128ull << 20;
// The inflate side's groups are twice as large: the batch decoder runs one
// tokenize wave per stream and is bound by a wave's latency, so two groups
// cost almost twice one (C2's 149 MiB of streams in two groups of 2048:
// tokenize 4.9 + 4.1 ms against 5.3 ms for the 4096 at once), and its scratch
// per input byte -- 16 bytes of token slots -- is what zt_inflate_raw_batch
// already takes for a whole batch.
constexpr uint64_t kDevInflateGroupBytes = 256ull << 20;
// the deflate pipeline's parse block (DF_BLOCK) and packing grid
constexpr uint32_t kDevBlk = 32768;

// src[0 .. len) -> dst[0 .. len), then `zero` zero bytes behind them (written
// by the job's last tile; zero < kDevTile and, with zero > 0, dst + len + zero
// on the tile grid of dst).  Its tiles are workgroups [tile0, tile0 +
// ceil(len / kDevTile)); len > 0.
struct DevCopyJob {
  uint64_t src, dst, len;
  uint32_t tile0, zero;
};
// A few bytes written by one thread.  kind kPatchBytes: the `len` <= 8 low
// bytes of `value`, little endian.  kind kFmtGzip or kFmtZlib: that member
// kind's trailer (put_trailer) with CRC-32 sums[2 sum], Adler-32
// sums[2 sum + 1] and the low 32 bits of value as ISIZE.
struct DevPatchJob {
  uint64_t dst, value;
  uint32_t len, kind, sum, pad;
};
constexpr uint32_t kPatchBytes = kFmtRaw;  // (a raw member has no trailer job)

struct DevCopyPlan {
  std::vector<DevCopyJob> jobs;
  uint64_t tiles = 0;
  // false: the job would take the launch past kDevMaxTiles (nothing added)
  bool add(uint64_t src, uint64_t dst, uint64_t len, uint32_t zero = 0) {
    if (len == 0) return true;
    const uint64_t t = (len + kDevTile - 1) / kDevTile;
    if (tiles + t > kDevMaxTiles) return false;
    jobs.push_back(DevCopyJob{src, dst, len, (uint32_t)tiles, zero});
    tiles += t;
    return true;
  }
};

// the job that owns workgroup `tile`: the last one with tile0 <= tile (the
// kernel's binary search, restated for the host check)
inline size_t dev_copy_find(const std::vector<DevCopyJob> &jobs, uint32_t tile) {
  size_t lo = 0, hi = jobs.size();
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) / 2;
    if (jobs[mid].tile0 <= tile)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// ---- the jobs of a frame (member_frame.h) --------------------------------------
// `len` bytes at dst: a byte patch per 8
inline void dev_patch_bytes(std::vector<DevPatchJob> &pj, uint64_t dst, const uint8_t *p, uint32_t len) {
  for (uint32_t a = 0; a < len; a += 8) {
    const uint32_t l = len - a < 8 ? len - a : 8;
    uint64_t v = 0;
    for (uint32_t k = 0; k < l; ++k) v |= (uint64_t)p[a + k] << (8 * k);
    pj.push_back(DevPatchJob{dst + a, v, l, kPatchBytes, 0, 0});
  }
}
// the trailer of a member of isize > 0 input bytes, its checksums at sums[2 sum ..]
inline void dev_patch_trailer(std::vector<DevPatchJob> &pj, MemberKind kind, uint64_t dst, uint64_t isize,
                              uint32_t sum) {
  if (kind != kFmtRaw)
    pj.push_back(DevPatchJob{dst, isize & 0xFFFFFFFFull, member_trailer_len(kind), (uint32_t)kind, sum, 0});
}

// n bytes at src as stored blocks of <= 65535 bytes at dst (what stored_write
// writes, stored_len(n) bytes): a header patch and, unless it is empty, a copy
// job per block.  false: past the tile limit.
inline bool dev_stored_jobs(uint64_t src, uint64_t n, uint64_t dst, DevCopyPlan &cp, std::vector<DevPatchJob> &pj) {
  uint64_t p = 0;
  do {
    const uint32_t l = (uint32_t)(n - p < 65535 ? n - p : 65535);
    pj.push_back(DevPatchJob{dst, stored_header(l, p + l == n), 5, kPatchBytes, 0, 0});
    if (!cp.add(src + p, dst + 5, l)) return false;
    dst += 5 + (uint64_t)l;
    p += l;
  } while (p < n);
  return true;
}

// ---- the bound ----------------------------------------------------------------
// Upper bound of one item's output (zt_deflate_dev_batch_bound), proven from
// what the pipeline can write.  A stream of n > 0 bytes is nb = ceil(n /
// 32768) parse blocks and (nb - 1) / 32 restart markers of 10 bytes
// (restart_after: counted from the stream's own first block).  Compression
// type 2: block_kernel takes the smallest of stored, fixed and dynamic, never
// more than stored_bits = blen + 5 ceil(blen / 65535) + 5 = blen + 10 bytes
// (blen <= 32768; the sync point included, which carries BFINAL on the last
// block, so the stream's end adds nothing).  Type 1: fixed codes spend at
// most 9 bits per input byte (a literal: 8 or 9 bits; a match of l >= 3 bytes:
// at most 8 + 5 + 5 + 13 = 31 bits, and 7 + 5 + 13 = 25 <= 27 for l = 3..10
// where the length has no extra bits), 7 for the end of block, 3 + 3 header
// bits, the padding and the 4 sync bytes: at most blen + blen / 8 + 7 bytes a
// block -- inside (blen + 10) + the n / 8 + 64 allowance deflate_out_bound
// carries for fixed codes.  Type 0: stored_len(n).  n == 0: 5 bytes.
inline uint64_t dev_batch_bound(uint64_t n, int ctype, MemberKind fmt) {
  const MemberFrame fr = frame_of(fmt, 0);
  const uint64_t frame = fr.prefix_len() + fr.trailer_len();
  if (n == 0 || ctype == 0) return stored_len(n) + frame;
  const uint64_t nb = (n + kDevBlk - 1) / kDevBlk;
  return n + 10 * nb + 10 * ((nb - 1) / 32) + (ctype == 1 ? n / 8 + 64 : 0) + frame;
}

// ---- groups -------------------------------------------------------------------
// Items `ids` in order, item k costing align_up(max(n, 1), align) bytes: group
// g is ids[cut[g] .. cut[g + 1]); a group ends before the item that would
// take it past `budget` (so only a single larger item exceeds it).
inline std::vector<size_t> dev_group_cuts(const size_t *n, const std::vector<size_t> &ids, size_t align,
                                          uint64_t budget) {
  std::vector<size_t> cut{0};
  uint64_t acc = 0;
  for (size_t k = 0; k < ids.size(); ++k) {
    const uint64_t cost = align_up(std::max<size_t>(n[ids[k]], 1), align);
    if (k > cut.back() && acc + cost > budget) {
      cut.push_back(k);
      acc = 0;
    }
    acc += cost;
  }
  cut.push_back(ids.size());
  return cut;
}

// ---- capacity -----------------------------------------------------------------
// item i fits: its `need` bytes go to the caller's buffer; else it is left out
// of the scatter's job table (ZT_E_ARG, out_len = need, no byte written)
inline bool dev_fits(uint64_t need, const size_t *out_cap, size_t i) { return need <= out_cap[i]; }

// The gather of items `ids` into the packed layout L at `base`: one copy job
// per non-empty item; zero_pad: the rest of its last 32 KiB cell zeroed
// (PackMode::zero_pad; L aligned to 32768).  ZT_OK, or ZT_E_ARG past the
// tile limit.
inline int dev_gather_plan(const uint64_t *src, const size_t *n, const std::vector<size_t> &ids, const PackLayout &L,
                           uint64_t base, bool zero_pad, DevCopyPlan &cp) {
  for (size_t k = 0; k < ids.size(); ++k) {
    const uint64_t len = n[ids[k]];
    const uint32_t zero = zero_pad ? (uint32_t)(align_up(len, kDevBlk) - len) : 0u;
    if (!cp.add(src[ids[k]], base + L.off[k], len, zero)) return ZT_E_ARG;
  }
  return ZT_OK;
}

}  // namespace zt
