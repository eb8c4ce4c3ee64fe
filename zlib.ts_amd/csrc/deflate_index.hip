// deflate_index.hip -- the deflate-time index (include/zt_index.h:
// zt_deflate_raw_indexed and the container forms).
//
// When encode_kernel returns, everything an index entry holds is on the
// device: the scanned block offsets (boff), every block's type and token
// count (BlockPlan), and the rule that places the restart markers
// (restart_after).  deflate_index_kernel, launched behind encode_kernel on
// the same stream, turns them into the entries zt_inflate_index_build would
// find by decoding the stream again: one lane writes one entry, nothing is
// read back in between, and the plain deflate launches nothing of this.
//
// The units of a call, in stream order (deflate_index_host.h: dix_unit_at):
// every block, then -- where restart_after holds -- the two empty stored
// blocks of the marker behind it, each a unit of its own (they end on a sync
// point like every block).  A final call adds the sentinel.
#include "deflate_index_host.h"
#include "zt_internal.h"

namespace zt {

namespace {

static_assert(DF_GROUP == 1, "one unit per parse block: a grouped build needs the group's leader and its ntok_sub sum");
static_assert(DF_BLOCK <= 65535, "a stored block is one payload");

struct DeflateIndexParams {
  const uint8_t *out;       // the call's stream
  const uint64_t *boff;     // nblocks + 1 block offsets in it (scan_sizes)
  const BlockPlan *plans;   // nblocks
  uint32_t *fault;
  uint32_t nblocks, restart;
  int final_;
  uint32_t nent;            // dix_call_units(nblocks, restart, final_)
  uint64_t n;               // the call's input bytes
  uint64_t in_base, out_base;
  IdxEntry *ent;            // nent entries, and the sentinel of a final call
};

// Does the layout dix_unit_at states agree with restart_after around entry e?
// Entry 0 is block 0; an entry follows its predecessor as the rule says (a
// block is followed by its marker's first half where restart_after holds, else
// by the next block); the last entry is the last block or its marker's second
// half.  All lanes together: the layout is the rule's.
__device__ __forceinline__ bool layout_holds(const DeflateIndexParams &P, uint32_t e, DixUnit u) {
  if (u.block >= P.nblocks || u.kind > 2) return false;
  const bool mark = restart_after(u.block, P.nblocks, P.restart, P.final_, nullptr);
  if (u.kind && !mark) return false;
  if (e + 1 == P.nent && (u.block + 1 != P.nblocks || u.kind != (mark ? 2u : 0u))) return false;
  if (e == 0) return u.block == 0 && u.kind == 0;
  const DixUnit p = dix_unit_at(e - 1, P.nblocks, P.restart);
  if (u.kind) return p.block == u.block && p.kind + 1 == u.kind;
  if (p.block + 1 != u.block) return false;
  return p.kind == (restart_after(p.block, P.nblocks, P.restart, P.final_, nullptr) ? 2u : 0u);
}

__global__ __launch_bounds__(256) void deflate_index_kernel(DeflateIndexParams P) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e > P.nent) return;
  if (e == P.nent) {
    if (P.final_) P.ent[e] = IdxEntry{P.in_base + P.boff[P.nblocks], P.out_base + P.n, 0u, 0u};
    return;
  }
  const DixUnit u = dix_unit_at(e, P.nblocks, P.restart);
  if (!layout_holds(P, e, u)) {
    atomicOr(P.fault, kFaultIndex);
    return;
  }
  uint64_t start, out_off;
  uint32_t ntok;
  if (u.kind == 0) {
    const BlockPlan *plan = P.plans + u.block;
    start = P.boff[u.block];
    out_off = (uint64_t)u.block * DF_BLOCK;
    // what tokenize_kernel counts: a Huffman block's literals and matches; a
    // stored payload's run tokens, or its bytes
    ntok = plan->btype == 0 ? dix_stored_tokens(plan->blen) : plan->ntok;
  } else {
    // the marker's halves lie 10 and 5 bytes before the next block (boff
    // counts the marker to the block it follows); both carry its output offset
    start = P.boff[u.block + 1] - (u.kind == 1 ? kRestartMarkerLen : kRestartMarkerLen / 2);
    const uint64_t nx = (uint64_t)(u.block + 1) * DF_BLOCK;
    out_off = nx < P.n ? nx : P.n;
    ntok = 0;
  }
  // a segment start, as find_syncs (inflate_seg.hip) decides it from the
  // stream's bytes: the ten before the unit are the marker.  A call's first
  // unit is one: the stream's first, or behind the marker the previous piece
  // ended with.
  uint32_t flag = e == 0 ? 1u : 0u;
  if (e && start >= kRestartMarkerLen) {
    const uint8_t *q = P.out + start - kRestartMarkerLen;
    bool m = true;
#pragma unroll
    for (uint32_t k = 0; k < kRestartMarkerLen; ++k) m = m && q[k] == ((k % 5) < 3 ? 0u : 0xFFu);
    flag = m ? 1u : 0u;
  }
  P.ent[e] = IdxEntry{P.in_base + start, P.out_base + out_off, ntok, flag};
}

}  // namespace

int deflate_index_launch(const DeflateParams &P, const DeflateIndexReq &ix, hipStream_t s) {
  if (P.span || P.nblocks == 0 || P.end <= P.halo || !ix.d_ent)
    return set_error(ZT_E_INTERNAL, "deflate index: not a single non-empty stream");
  const uint64_t nent = dix_call_units(P.nblocks, P.restart, P.final_ != 0);
  // (the caller laid the table out with dix_layout: the same count, or the two have drifted apart)
  if (nent + (P.final_ ? 1 : 0) != ix.cap || nent >= 0x7FFFFFFFull)
    return set_error(ZT_E_INTERNAL, "deflate index: the call's entries are not what the table was laid out for");
  DeflateIndexParams K;
  K.out = P.out;
  K.boff = P.boff;
  K.plans = P.plans;
  K.fault = P.fault;
  K.nblocks = P.nblocks;
  K.restart = P.restart;
  K.final_ = P.final_;
  K.nent = (uint32_t)nent;
  K.n = P.end - P.halo;
  K.in_base = ix.in_base;
  K.out_base = ix.out_base;
  K.ent = ix.d_ent;
  deflate_index_kernel<<<(uint32_t)((nent + 1 + 255) / 256), 256, 0, s>>>(K);
  ZT_HIP(hipGetLastError());
  return ZT_OK;
}

}  // namespace zt
