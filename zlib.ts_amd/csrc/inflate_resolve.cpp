// inflate_resolve.cpp -- a host-built chain on its way through the resolve
// kernels (zt_internal.h: ChainBuf, ChainRun): the one place that carves the
// chain buffer, uploads chain and segments from pinned staging, fills
// ResolveParams and brings the statuses back.  Used by the segment path's host
// walk (inflate_seg.hip) and the batch decoder (inflate_api.cpp); the general
// path (inflate_gen.hip) shares chain_buf and resolve_params and keeps its own
// transfers (measured faster there: profiles/inflate_driver_ab.txt).
#include <algorithm>
#include <cstring>

#include "zt_internal.h"

namespace zt {

static int chain_upload(DeviceCtx *c, const std::vector<ChainUnit> &chain, const std::vector<SegJob> &segs,
                        size_t pin_front, ChainRun *run, hipStream_t s) {
  void *d_chain, *hp;
  const size_t bytes = chain_buf(nullptr, chain.size(), segs.size()).bytes;
  ZT_TRY(scratch(c, kChain, bytes, &d_chain));
  ZT_TRY(pinned(c, pin_front + bytes, &hp, kPinInflateMeta));
  run->dev = chain_buf(d_chain, chain.size(), segs.size());
  run->host = chain_buf(static_cast<uint8_t *>(hp) + pin_front, chain.size(), segs.size());
  run->nunits = (uint32_t)chain.size();
  run->nseg = (uint32_t)segs.size();
  memcpy(run->host.units, chain.data(), chain.size() * sizeof(ChainUnit));
  memcpy(run->host.segs, segs.data(), segs.size() * sizeof(SegJob));
  ZT_TRY(x_copy(run->dev.units, run->host.units, chain.size() * sizeof(ChainUnit), s));
  return x_copy(run->dev.segs, run->host.segs, segs.size() * sizeof(SegJob), s);
}

ResolveParams resolve_params(const ChainRun &run, const uint32_t *tokens, uint16_t *desc, uint8_t *out,
                             int32_t marker, const uint8_t *in) {
  ResolveParams rp;
  rp.tokens = tokens;
  rp.units = run.dev.units;
  rp.segs = run.dev.segs;
  rp.out = out;
  rp.desc = desc;
  rp.unit_status = run.dev.unit_status;
  rp.seg_status = run.dev.seg_status;
  rp.nunits = run.nunits;
  rp.nseg = run.nseg;
  rp.marker = marker;
  rp.in = in;
  return rp;
}

int resolve_chain_dev(DeviceCtx *c, const std::vector<ChainUnit> &chain, const std::vector<SegJob> &segs,
                      uint64_t desc_total, const uint32_t *tokens, uint8_t *out, int32_t marker, const uint8_t *in,
                      size_t pin_front, ChainRun *run, hipStream_t s) {
  void *d_desc;
  ZT_TRY(scratch(c, kDeflateOrDesc, (desc_total + 1024) * 2, &d_desc));  // + slack: chunked descriptor reads
  ZT_TRY(chain_upload(c, chain, segs, pin_front, run, s));
  return resolve_segments_dev(resolve_params(*run, tokens, static_cast<uint16_t *>(d_desc), out, marker, in), s);
}

int chain_statuses(const ChainRun &run, hipStream_t s) {
  ZT_TRY(x_copy(run.host.unit_status, run.dev.unit_status, run.nunits * 4ull, s));
  ZT_TRY(x_copy(run.host.seg_status, run.dev.seg_status, run.nseg * 4ull, s));
  ZT_HIP(hipStreamSynchronize(s));
  return ZT_OK;
}

// seg_chain_host on host tables, in zt_debug_chain's shape (no device)
extern "C" int zt_debug_chain_host(const TokResult *res, const uint8_t *restart, const uint64_t *tok_off,
                                   uint32_t units, ChainInfo *info, ChainUnit *cu, SegJob *sj, uint32_t *nchain,
                                   int *outcome) {
  if (!res || !restart || !tok_off || !info || !cu || !sj || !nchain || !outcome || units == 0)
    return set_error(ZT_E_ARG, "zt_debug_chain_host: bad argument");
  const ChainPlan p = seg_chain_host(res, restart, tok_off, units);
  *outcome = (int)p.outcome;
  *nchain = (uint32_t)p.chain.size();
  *info = ChainInfo{p.outcome == ChainPlan::kBuilt, (uint32_t)p.segs.size(), p.total, res[p.last].end_bits,
                    p.desc_total};
  if (p.outcome != ChainPlan::kBuilt) return ZT_OK;
  std::copy(p.chain.begin(), p.chain.end(), cu);
  std::copy(p.segs.begin(), p.segs.end(), sj);
  return ZT_OK;
}

}  // namespace zt
