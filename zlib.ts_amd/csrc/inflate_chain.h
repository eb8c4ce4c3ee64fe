// inflate_chain.h -- host-only logic of the two-phase inflate: the tables the
// tokenizer fills (inflate_tok.hip), the chain units and segment jobs the
// resolve kernels read, and the two host functions that turn the first into
// the second -- seg_chain_host for one large stream (inflate_seg.hip; its
// device twin is chain_kernel there) and batch_chain_host for a batch of
// small streams (inflate_api.cpp) -- and SegLayout, the segment rule that
// seg_chain_host and the range planners (index_host.h, ckpt_host.h) lay their
// chains out by.  No device code and no HIP types:
// tools/inflate_chain_check.cpp runs it under ASan / UBSan.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/zt.h"

namespace zt {

// phase A: one unit = blocks from one sync point to the next
struct TokJob {
  uint64_t start;       // byte position (relative to `in`) of the unit's first block
  uint64_t tok_off;     // first token slot
  uint32_t tok_cap;     // token capacity
  uint32_t stop_first;  // index of the first sync point after `start`
  uint64_t end;         // end of the unit's input (batch: its stream's end), 0: TokParams::n
};
struct TokResult {
  uint64_t out_len;   // bytes the unit's tokens produce
  uint64_t end_bits;  // bit position after the unit's last block
  uint32_t ntok;
  int32_t status;
  int32_t detail;
  int32_t stop_idx;   // sync point where the unit stopped, -1 at BFINAL
};
// stored payloads of at least this many bytes become run tokens (TokParams::run_tokens)
constexpr uint32_t kStoredRunMin = 1024;
// phase B: units of the chain, grouped by segment
struct ChainUnit {
  uint64_t tok_off;
  uint64_t out_off;  // absolute output offset
  uint64_t seg_off;  // output offset of the unit's segment
  uint64_t desc_off; // its descriptors (segments start 512-aligned)
  uint32_t ntok;
  uint32_t out_len;
};
struct SegJob {
  uint32_t first, count;  // chain units [first, first + count)
};
// the chain built on the device (inflate_seg.hip chain_kernel); ok == 0: not
// the common case, expand / copy return at once and the host walks the chain
struct ChainInfo {
  int32_t ok;
  uint32_t nseg;
  uint64_t total;       // output bytes
  uint64_t end_bits;    // bit after the last unit's last block
  uint64_t desc_total;  // descriptors
};

// v rounded up to a multiple of a (every host file's one rounding function)
inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// The segment layout of a run of units that follow each other in one output
// buffer, appended to a chain unit by unit: a segment starts with the first
// unit and at every later start entry that has output since the previous
// start, and its descriptors start 512-aligned.
// (A start entry right after another -- the empty stored blocks of a restart
// marker -- leaves the segment before it empty: that one simply starts here
// instead.  Empty copy waves would sit between the full ones in the launch,
// and the workgroup -> XCD round robin would then give half of the XCDs every
// 1 MiB segment: two rounds of copy waves.)
struct SegLayout {
  std::vector<ChainUnit> &chain;
  std::vector<SegJob> &segs;
  uint64_t &desc_total;
  bool open = false;
  uint64_t seg_start = 0, desc_seg = 0;  // of the current segment: output offset, descriptors
  SegLayout(std::vector<ChainUnit> &c, std::vector<SegJob> &s, uint64_t &d) : chain(c), segs(s), desc_total(d) {}
  // out_off: the unit's place in the buffer; returns true when the unit opened a segment
  bool add(uint64_t tok_off, uint64_t out_off, uint32_t ntok, uint32_t out_len, bool start_entry) {
    const bool opens = !open || (start_entry && out_off != seg_start);
    if (opens) {
      desc_total = align_up(desc_total, 512);
      desc_seg = desc_total;
      seg_start = out_off;
      segs.push_back(SegJob{(uint32_t)chain.size(), 0});
      open = true;
    }
    chain.push_back(ChainUnit{tok_off, out_off, seg_start, desc_seg + (out_off - seg_start), ntok, out_len});
    segs.back().count++;
    desc_total = desc_seg + (out_off + out_len - seg_start);
    return opens;
  }
};

// What the host makes of one stream's unit tables.
struct ChainPlan {
  enum Outcome {
    kBuilt,      // chain and segs are ready for the resolve kernels
    kFallback,   // not a stream for this path: `why` says what stopped the walk
    kTruncated,  // the chain reached the last unit and that one ran out of input
  };
  Outcome outcome = kFallback;
  std::string why;                // one line, no prefix, newline-terminated
  std::vector<ChainUnit> chain;
  std::vector<SegJob> segs;
  std::vector<uint32_t> on_chain; // chain[k] is unit on_chain[k] of the tables
  uint64_t total = 0;             // output bytes
  uint64_t desc_total = 0;        // descriptors
  size_t last = 0;                // the unit the walk ended on
};

// The chain from the stream start: unit -> the sync point it stopped on ->
// the unit starting there ..., so candidates that lie inside data are never
// used; cut into segments at restart points (restart[u - 1] != 0: unit u
// follows a restart marker).  res / tok_off hold `units` entries, restart
// units - 1.  Output offsets are the prefix sums of the units' output lengths;
// each segment's descriptors start 512-aligned.
inline ChainPlan seg_chain_host(const TokResult *res, const uint8_t *restart, const uint64_t *tok_off, size_t units) {
  ChainPlan p;
  char msg[160];
  uint64_t total = 0, desc_total = 0;
  SegLayout lay(p.chain, p.segs, desc_total);
  size_t u = 0;
  for (;;) {
    const TokResult &r = res[u];
    p.last = u;
    // the chain reached the last unit (which runs to the end of the input)
    // and that one ran out of input: a window that cuts a longer stream
    // (inflate_dev_member grows it) -- or a truncated stream
    if (u + 1 == units && u > 0 && (r.status == ZT_E_INPUT_BROKEN || r.status == ZT_E_STORED_LEN)) {
      snprintf(msg, sizeof msg, "chain ran out of input in its last unit %zu\n", u);
      p.why = msg;
      p.outcome = ChainPlan::kTruncated;
      return p;
    }
    if (r.status != ZT_OK || r.out_len > 0xFFFFFFFFull) {
      snprintf(msg, sizeof msg, "unit %zu (chain %zu): status %d detail %d ntok %u out %llu\n", u, p.chain.size(),
               r.status, r.detail, r.ntok, (unsigned long long)r.out_len);
      p.why = msg;
      return p;
    }
    lay.add(tok_off[u], total, r.ntok, (uint32_t)r.out_len, u == 0 || restart[u - 1]);
    p.on_chain.push_back((uint32_t)u);
    total += r.out_len;
    if (r.stop_idx < 0) break;
    const size_t nx = (size_t)r.stop_idx + 1;
    if (nx <= u || nx >= units) {
      snprintf(msg, sizeof msg, "unit %zu: bad stop %d\n", u, r.stop_idx);
      p.why = msg;
      return p;
    }
    u = nx;
  }
  // a segment of units that hold stored runs only (TokResult ntok bit 30;
  // or nothing) is written by expand_kernel straight from the input and
  // skipped by copy_kernel (SegJob count bit 31); elsewhere bit 30 is cleared
  for (SegJob &sj : p.segs) {
    bool direct = true;
    for (uint32_t k = 0; k < sj.count; ++k) {
      const ChainUnit &cu = p.chain[sj.first + k];
      direct = direct && ((cu.ntok >> 30) == 3u || cu.out_len == 0);  // (empty units: the restart markers)
    }
    for (uint32_t k = 0; k < sj.count && !direct; ++k) p.chain[sj.first + k].ntok &= ~0x40000000u;
    if (direct) sj.count |= 0x80000000u;
  }
  p.total = total;
  p.desc_total = desc_total;
  p.outcome = ChainPlan::kBuilt;
  return p;
}

// The batch chain: one unit and one segment per stream that decoded to BFINAL
// (res[k] / tok_off[k]: stream k's one unit).  Every output starts 256-aligned
// in one buffer (an empty one reserves 256 bytes, so every pointer is
// distinct), every stream's descriptors 512-aligned.  A stream the two-phase
// pass cannot finish goes to `failed`; who[j] is chain[j]'s stream.
struct BatchChain {
  std::vector<ChainUnit> chain;
  std::vector<SegJob> segs;
  std::vector<size_t> who, failed;
  uint64_t out_total = 0;   // bytes of the shared output buffer
  uint64_t desc_total = 0;  // descriptors
};
inline BatchChain batch_chain_host(const TokResult *res, const uint64_t *tok_off, size_t streams) {
  BatchChain b;
  for (size_t k = 0; k < streams; ++k) {
    const TokResult &r = res[k];
    if (r.status != ZT_OK || r.stop_idx >= 0 || r.out_len > 0xFFFFFFFFull) {
      b.failed.push_back(k);
      continue;
    }
    b.desc_total = align_up(b.desc_total, 512);
    // (a stream of stored runs only: expand_kernel writes it straight from
    // the input, copy_kernel skips its segment)
    const bool direct = (r.ntok >> 30) == 3u;
    b.segs.push_back(SegJob{(uint32_t)b.chain.size(), direct ? 0x80000001u : 1u});
    b.chain.push_back(ChainUnit{tok_off[k], b.out_total, b.out_total, b.desc_total, r.ntok, (uint32_t)r.out_len});
    b.who.push_back(k);
    b.out_total += align_up(r.out_len ? r.out_len : 1, 256);
    b.desc_total += r.out_len;
  }
  return b;
}

}  // namespace zt
