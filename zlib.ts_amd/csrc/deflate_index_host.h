// deflate_index_host.h -- the arithmetic of the deflate-time index
// (include/zt_index.h: zt_deflate_raw_indexed and the container forms): which
// units a deflate call writes, where each call's entries lie in the table of a
// pieced stream, and the blob's header.  deflate_index_kernel
// (deflate_index.hip) fills the entries; everything here runs on the host as
// well, without HIP types: tools/deflate_index_host_check.cpp runs it under
// ASan / UBSan.
//
// A deflate call of `nblocks` blocks writes, in stream order, one unit per
// block and two empty units (the halves of the restart marker) after every
// block for which restart_after holds.  restart_after is the rule the encoder
// and scan_sizes place the markers by (deflate_post.hip); it lives here so
// that the index and the stream share one function.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "index_host.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define ZT_DIX_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ZT_DIX_HD inline
#endif
#ifndef ZT_DF_BLOCK
#define ZT_DF_BLOCK 32768  // (zt_internal.h: DF_BLOCK)
#endif

namespace zt {

// A restart point (segment boundary) follows block b of n: inside a call at
// every `restart`-th block; a non-final call (a shard, a piece) also ends with
// the marker.  Batch (span: per block the [start, end) of its stream): inside
// a stream only (its last block carries BFINAL).
ZT_DIX_HD bool restart_after(uint32_t b, uint32_t n, uint32_t restart, int final_, const uint64_t *span) {
  if (span) {
    const uint64_t nx = (uint64_t)(b + 1) * ZT_DF_BLOCK;
    return nx < span[2 * (uint64_t)b + 1] && ((nx - span[2 * (uint64_t)b]) / ZT_DF_BLOCK) % restart == 0;
  }
  return (b + 1 < n) ? ((b + 1) % restart) == 0 : !final_;
}

// units of one call's blocks and the markers between them (the marker a
// non-final call ends with not counted)
ZT_DIX_HD uint64_t dix_inner_units(uint64_t nblocks, uint32_t restart) {
  return nblocks + 2 * ((nblocks - 1) / restart);
}
// units of one call of nblocks >= 1 blocks (without a sentinel)
ZT_DIX_HD uint64_t dix_call_units(uint64_t nblocks, uint32_t restart, bool final_) {
  return dix_inner_units(nblocks, restart) + (final_ ? 0 : 2);
}

// Unit e of a call: block `block` itself (kind 0), or the first / second empty
// unit of the marker behind it (kind 1 / 2).
struct DixUnit {
  uint32_t block, kind;
};
ZT_DIX_HD DixUnit dix_unit_at(uint32_t e, uint32_t nblocks, uint32_t restart) {
  const uint32_t inner = (uint32_t)dix_inner_units(nblocks, restart);
  if (e >= inner) return DixUnit{nblocks - 1, e - inner + 1};  // (the marker that ends a non-final call)
  const uint32_t per = restart + 2, seg = e / per, r = e % per;
  if (r < restart) return DixUnit{seg * restart + r, 0};
  return DixUnit{seg * restart + restart - 1, r - restart + 1};
}

// tokens tokenize_kernel counts for a stored payload of len bytes
ZT_DIX_HD uint32_t dix_stored_tokens(uint32_t len) { return len >= kStoredRunMin ? 3u : len; }

// A stream written as pieces (deflate_raw_pipelined; one piece: the one-call
// path): piece i's first entry in the table, from the piece sizes alone.  Every
// piece but the last is non-final.
struct DixLayout {
  std::vector<uint64_t> first;  // np + 1: piece i's entries are [first[i], first[i + 1])
  uint64_t nunits = 0;          // = first[np]; the table holds nunits + 1 entries (the sentinel)
};
inline DixLayout dix_layout(const std::vector<size_t> &sizes, uint32_t restart) {
  DixLayout L;
  L.first.assign(sizes.size() + 1, 0);
  for (size_t i = 0; i < sizes.size(); ++i) {
    const uint64_t nb = (sizes[i] + ZT_DF_BLOCK - 1) / ZT_DF_BLOCK;
    L.first[i + 1] = L.first[i] + dix_call_units(nb ? nb : 1, restart, i + 1 == sizes.size());
  }
  L.nunits = L.first[sizes.size()];
  return L;
}

// The header of a blob whose nunits + 1 entries are in place: the segment count
// from the entries' flags, then the whole blob through index_validate against
// an input that ends where the stream ends.  Returns null, or the validator's
// reason (an engine fault: the compressor's own index must pass).
inline const char *dix_finish(uint8_t *blob, size_t nunits, uint64_t stream_start, uint64_t stream_len,
                              uint64_t total_out) {
  uint32_t nseg = 0;
  for (size_t k = 0; k < nunits; ++k) nseg += idx_get32(blob + kIdxHeader + k * kIdxEntry + 20) & 1u;
  index_write_header(blob, (uint32_t)nunits, nseg, stream_start, stream_start + stream_len, total_out);
  IndexView v;
  return index_validate(blob, index_blob_bytes(nunits), (size_t)(stream_start + stream_len), &v);
}

}  // namespace zt
