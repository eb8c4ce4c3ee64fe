// stream_host.h -- the arithmetic of the inflate sessions (include/zt_stream.h),
// no HIP: the records the host and session_kernel (inflate_stream.hip) share,
// the pending-tail bookkeeping, the decode limit of a feed, the output slots of
// a launch and of its relaunches, the trailing-byte count, the checksum
// combination and the duplicate-session check.  Pure functions, checked on the
// CPU by tools/stream_host_check.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace zt {

// ---- records shared with the kernel -------------------------------------------
enum SessPhase : uint32_t {
  SP_HEADER = 0,  // at a block header (the stream start included)
  SP_HUFF = 1,    // at a token of a Huffman body
  SP_STORED = 2,  // at a byte of a stored body
  SP_DONE = 3,    // the BFINAL block's end was decoded
};
enum SessStop : int32_t {
  SS_NEED_INPUT = 0,  // the next token / header is not complete (or lies in the last 8 bytes of a non-final feed)
  SS_OUT_FULL = 1,    // fewer than 258 bytes of room in the output slot
  SS_FINISHED = 2,
  SS_ERROR = 3,
};
constexpr uint32_t kSessRing = 32768;
// One session's device state.  The ring holds output position p (the preset
// window counted) at ring[p & (kSessRing - 1)].
struct SessRec {
  uint8_t ring[kSessRing];
  uint8_t lens[320];     // SP_HUFF, BTYPE 2: the block's hlit + hdist code lengths
  uint64_t op;           // preset window + bytes produced
  uint32_t phase;        // SessPhase
  uint32_t bfinal, btype;
  uint32_t stored_left;  // SP_STORED: payload bytes still to copy
  uint32_t hlit, hdist;  // SP_HUFF, BTYPE 2
  uint32_t bit_off;      // bits of the first pending byte already consumed
  int32_t status, detail;  // sticky
  uint32_t pad[37];
};
static_assert(sizeof(SessRec) == kSessRing + 320 + 192 && sizeof(SessRec) % 256 == 0, "records tile a slab");
struct SessJob {
  SessRec *rec;
  const uint8_t *in;  // pending | new bytes (16-byte aligned)
  uint64_t n;
  uint8_t *out;       // this launch's output slot
  uint64_t cap;
  int32_t last;
  int32_t pad;
};
struct SessResult {
  uint64_t end_bits;   // bits of `in` consumed by what was decoded (the record's bit_off included)
  uint64_t out_len;    // bytes written to the slot
  uint64_t read_bits;  // bits the reader went over in this launch
  int32_t stop;        // SessStop
  int32_t status, detail;
  int32_t pad;
};

// ---- a feed ------------------------------------------------------------------
constexpr size_t kSessLag = 8;          // a non-final feed starts no token in its last 8 bytes (zt.h's convention)
constexpr size_t kSessHeaderMax = 1024; // a block header is shorter: the cap of the pending tail
// bits of a slot of m bytes below which a token may start
inline uint64_t sess_limit_bits(size_t m, int last) {
  if (last) return (uint64_t)m * 8;
  return m > kSessLag ? (uint64_t)(m - kSessLag) * 8 : 0;
}
// a launch can decode something: a final feed always runs (it settles the
// stream's end), another one when a token may start
inline bool sess_has_work(size_t m, uint32_t bit_off, int last) { return last || sess_limit_bits(m, 0) > bit_off; }
// After a launch over a slot of m bytes that consumed end_bits bits: the bytes
// to drop from its front, the bits used of the first byte kept, the tail kept.
struct SessTail {
  size_t drop;
  uint32_t bit_off;
  size_t pending;
};
inline SessTail sess_tail(size_t m, uint64_t end_bits) {
  SessTail t;
  t.drop = (size_t)(end_bits >> 3);
  if (t.drop > m) t.drop = m;
  t.bit_off = t.drop < m ? (uint32_t)(end_bits & 7) : 0;
  t.pending = m - t.drop;
  return t;
}
// fed bytes behind the stream's end (a container's trailer)
inline uint64_t sess_unused(uint64_t total_in, uint64_t end_bits) { return total_in - (end_bits + 7) / 8; }

// ---- output slots ----------------------------------------------------------------
// The slot of a session's launch: eight times its input (at least 4 KiB),
// doubled with every relaunch after an output-full stop up to 4 MiB, plus the
// 258 bytes of room a match needs, 256-aligned.  No size is guessed: a slot
// that fills stops the kernel at a token, and the host launches again.
constexpr size_t kSessSlotMax = 4u << 20;
inline size_t sess_out_cap(size_t m, unsigned relaunch) {
  size_t c = std::max<size_t>(m * 8, 4096);
  for (unsigned r = 0; r < relaunch && c < kSessSlotMax; ++r) c *= 2;
  c = std::min(c, kSessSlotMax);
  return (c + 258 + 255) & ~size_t(255);
}
// One launch round: job k (of `m` pending-and-new bytes, relaunched r[k]
// times) writes to [off[k], off[k] + cap[k]) of the output buffer.
struct SessOutPlan {
  std::vector<size_t> off, cap;
  size_t total = 0;
};
inline SessOutPlan sess_out_plan(const std::vector<size_t> &m, const std::vector<unsigned> &relaunch) {
  SessOutPlan p;
  p.off.resize(m.size());
  p.cap.resize(m.size());
  for (size_t k = 0; k < m.size(); ++k) {
    p.off[k] = p.total;
    p.cap[k] = sess_out_cap(m[k], relaunch[k]);
    p.total += p.cap[k];
  }
  return p;
}
// the jobs of the next round: those that stopped on a full slot
inline std::vector<size_t> sess_relaunch(const std::vector<int32_t> &stop) {
  std::vector<size_t> again;
  for (size_t k = 0; k < stop.size(); ++k)
    if (stop[k] == SS_OUT_FULL) again.push_back(k);
  return again;
}

// ---- checksums -----------------------------------------------------------------
// Adler-32 of A | B from Adler-32(A), Adler-32(B) and len(B)
inline uint32_t adler_combine(uint32_t a, uint32_t b, uint64_t len_b) {
  const uint32_t M = 65521;
  const uint32_t rem = (uint32_t)(len_b % M);
  uint32_t s1 = a & 0xFFFF, s2 = (uint32_t)(((uint64_t)rem * s1) % M);
  s1 += (b & 0xFFFF) + M - 1;
  s2 += ((a >> 16) & 0xFFFF) + ((b >> 16) & 0xFFFF) + M - rem;
  if (s1 >= M) s1 -= M;
  if (s1 >= M) s1 -= M;
  if (s2 >= (M << 1)) s2 -= (M << 1);
  if (s2 >= M) s2 -= M;
  return s1 | (s2 << 16);
}

// ---- a batch call's sessions -----------------------------------------------------
inline bool sess_has_duplicates(const void *const *s, size_t count) {
  std::vector<const void *> v(s, s + count);
  std::sort(v.begin(), v.end());
  return std::adjacent_find(v.begin(), v.end()) != v.end();
}

}  // namespace zt
