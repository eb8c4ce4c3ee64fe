// range_call.h -- the driver of a range call, shared by the formats whose plan
// is made on the host before anything runs (index_api.hip, ckpt_api.hip), and
// the slab of a call's outputs (bgzf_api.hip uses it too).
//
// One upload carries the chain, its segments, the gather's jobs, the format's
// own tables and the packed input; then, without the host waiting in between,
// the format's tokenizer, its verify kernel (which clears ChainInfo::ok when
// the blob does not hold), expand + copy and range_gather_kernel
// (range_call.hip); one download brings the packed ranges and every status
// back.
//
// A format F hands the driver
//   plan            its plan (a RangePlanCore with `spans`, RangeSpan or derived)
//   counters        its RangeCounters
//   kTag, kUpload   the tag of its ZT_INDEX_TIMING stamps, the text of a failed upload
//   Tables, Out     its own pointers into kRangeIn and kRangeOut, set by
//                   carve_upload (part of the upload), carve_device (device-only)
//                   and carve_out (part of the download): called through the
//                   driver's Carve pass, so that the device layout, its pinned
//                   mirror and the sizes (null base) come from one function
//   admit           refuses a call before any allocation, or says whether the
//                   packed input is staged with the tables (one copy) or goes
//                   up from the caller's buffer (upload())
//   span_src        where a span's compressed bytes lie in the caller's input
//   fill            fills its tables in the mirror (and, staged, what it keeps
//                   in the packed input besides the spans)
//   enqueue         its tokenizer, its verify kernel and its resolve variant
//   downloaded      after the download: failures that are no unit's own
//                   (pre-marked in `ust`), counters of its own
//   error           sets the error of a failed range
#pragma once
#include <cstring>
#include <mutex>
#include <vector>

#include "range_plan.h"
#include "zt_internal.h"

namespace zt {

// A call's outputs: one slab, a pointer into it for every range that succeeds.
struct RangeSlab {
  uint8_t *base;
  size_t count;
  uint8_t **out;
  size_t *out_len;
  // the call fails as a whole
  int give_up(int rc) const {
    for (size_t i = 0; i < count; ++i) slab_release(base);
    for (size_t i = 0; i < count; ++i) out[i] = nullptr, out_len[i] = 0;
    return rc;
  }
  // range i with status[i] == ZT_OK gets len(i) bytes at base + dst(i); any
  // other gives its share of the slab back.  Returns fail(i) of the first
  // failed range (which sets the error), or ZT_OK.
  template <class Dst, class Len, class Fail>
  int hand_out(const int *status, Dst dst, Len len, std::atomic<uint64_t> &returned, Fail fail) const {
    int rc = ZT_OK;
    for (size_t i = 0; i < count; ++i) {
      if (status[i] != ZT_OK) {
        slab_release(base);
        out[i] = nullptr;
        out_len[i] = 0;
        if (rc == ZT_OK) rc = fail(i);
        continue;
      }
      out[i] = base + dst(i);
      out_len[i] = (size_t)len(i);
      returned += len(i);
    }
    return rc;
  }
};

struct RangeCounters {
  std::atomic<uint64_t> range_calls{0}, ranges{0}, units_tokenized{0}, in_bytes_uploaded{0}, out_bytes_decoded{0},
      out_bytes_returned{0};
};

// the one upload's layout (kRangeIn and its pinned mirror), then the device-only results
struct RangeTables {
  ChainUnit *chain;
  SegJob *segs;
  RangeJob *rjobs;
  ChainInfo *info;
  size_t table_bytes;   // the tables alone
  uint8_t *in;
  size_t upload_bytes;  // tables and packed input
  size_t bytes;
};
template <class F>
RangeTables range_tables(void *base, const F &f, size_t njobs, typename F::Tables *x) {
  Carve cv(base);
  RangeTables t;
  t.chain = cv.take<ChainUnit>(f.plan.chain.size());
  t.segs = cv.take<SegJob>(f.plan.segs.size());
  t.rjobs = cv.take<RangeJob>(njobs);
  t.info = cv.take<ChainInfo>(1);
  f.carve_upload(cv, x);
  t.table_bytes = cv.bytes();
  t.in = cv.take<uint8_t>(f.plan.in_total + 256);  // + slack: the reader's aligned loads
  t.upload_bytes = cv.bytes();
  f.carve_device(cv, x);
  t.bytes = cv.bytes();
  return t;
}
// the one download's layout (kRangeOut; the host slab mirrors it)
struct RangeOut {
  uint8_t *bytes;
  int32_t *vstatus;  // [2 u]: unit u's verdict, [2 u + 1]: its detail (inflate_error's second argument)
  int32_t *unit_status, *seg_status;
  size_t total;
};
template <class F>
RangeOut range_out(void *base, const F &f, typename F::Out *x) {
  Carve cv(base);
  RangeOut o;
  const size_t nu = f.plan.chain.size();
  o.bytes = cv.take<uint8_t>(f.plan.dst_total);
  o.vstatus = cv.take<int32_t>(2 * nu);
  o.unit_status = cv.take<int32_t>(nu);
  o.seg_status = cv.take<int32_t>(f.plan.segs.size());
  f.carve_out(cv, x);
  o.total = cv.bytes();
  return o;
}

template <class F>
int range_call(const F &f, size_t count, uint8_t **out, size_t *out_len, int *status) {
  const auto &plan = f.plan;
  f.counters.ranges += count;
  for (size_t i = 0; i < count; ++i) {
    out[i] = nullptr;
    out_len[i] = 0;
    status[i] = plan.ranges[i].status;
  }
  const size_t nu = plan.chain.size(), ns = plan.segs.size();
  std::vector<RangeJob> rjobs;
  uint64_t tiles = 0;
  for (const PlannedRange &r : plan.ranges)
    if (r.span >= 0) range_job_add(rjobs, &tiles, r.src, r.dst, r.len);
  if (tiles > 0x7FFFFFFFull || nu > 0x7FFFFFFFull) return set_error(ZT_E_ARG, "too many ranges for one call");
  typename F::Tables dx, hx;
  typename F::Out dox, hox;
  const RangeTables lay = range_tables(nullptr, f, rjobs.size(), &dx);
  const RangeOut ho_layout = range_out(nullptr, f, &dox);
  bool staged = true;
  ZT_TRY(f.admit(lay, &staged));
  const RangeSlab slab{slab_out(nu ? ho_layout.total : plan.dst_total, count, true), count, out, out_len};
  if (!slab.base) return set_error(ZT_E_NOMEM, "host allocation failed");
  int first = ZT_OK, first_detail = 0;
  if (nu) {  // (nothing to decode: no GPU touched)
    DeviceCtx *c;
    if (const int rc = get_ctx(&c)) return slab.give_up(rc);
    std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
    hipStream_t s = c->stream;
    // ZT_INDEX_TIMING=1: host wall time of a range call's stages on stderr (measurement only)
#define XT(label) ZT_STAMP("ZT_INDEX_TIMING", F::kTag, label)
#define RT(call)                                          \
  do {                                                    \
    if (const int rc_ = (call)) return slab.give_up(rc_); \
  } while (0)
    XT("planned");
    void *d_tab, *h_tab, *d_tok, *d_desc, *d_dec, *d_ro;
    RT(scratch(c, kRangeIn, lay.bytes, &d_tab));
    RT(pinned(c, staged ? lay.upload_bytes : lay.table_bytes, &h_tab, kPinBatch));
    RT(scratch(c, kTokens, ((size_t)plan.tok_total + 256) * 4, &d_tok));  // + slack: chunked token reads
    RT(scratch(c, kDeflateOrDesc, ((size_t)plan.desc_total + 1024) * 2, &d_desc));  // + slack: chunked descriptor reads
    RT(scratch(c, kOut, (size_t)plan.dec_total + 256, &d_dec));
    RT(scratch(c, kRangeOut, ho_layout.total, &d_ro));
    const RangeTables D = range_tables(d_tab, f, rjobs.size(), &dx), H = range_tables(h_tab, f, rjobs.size(), &hx);
    const RangeOut DO = range_out(d_ro, f, &dox);
    // the one upload: [chain | segments | ranges | chain summary | the format's tables | packed spans]
    // (not staged: the mirror ends with the tables, H.in lies behind it)
    for (const auto &sp : plan.spans)
      if (staged) copy_to_staging(H.in + sp.in_pos, f.span_src(sp), sp.in_len);
    memcpy(H.chain, plan.chain.data(), nu * sizeof(ChainUnit));
    memcpy(H.segs, plan.segs.data(), ns * sizeof(SegJob));
    if (!rjobs.empty()) memcpy(H.rjobs, rjobs.data(), rjobs.size() * sizeof(RangeJob));
    *H.info = ChainInfo{1, (uint32_t)ns, plan.dec_total, 0, plan.desc_total};
    f.fill(H, hx);
    {
      const hipError_t e = hipMemcpyAsync(d_tab, h_tab, staged ? lay.upload_bytes : lay.table_bytes,
                                          hipMemcpyHostToDevice, s);
      if (e != hipSuccess) return slab.give_up(hip_fail(e, F::kUpload));
    }
    if (!staged)
      for (const auto &sp : plan.spans) RT(upload(c, D.in + sp.in_pos, f.span_src(sp), sp.in_len, s));
    XT("uploaded");
    ResolveParams rp;
    rp.tokens = static_cast<const uint32_t *>(d_tok);
    rp.units = D.chain;
    rp.segs = D.segs;
    rp.out = static_cast<uint8_t *>(d_dec);
    rp.desc = static_cast<uint16_t *>(d_desc);
    rp.unit_status = DO.unit_status;
    rp.seg_status = DO.seg_status;
    rp.nunits = (uint32_t)nu;
    rp.nseg = (uint32_t)ns;
    rp.info = D.info;
    rp.order = nullptr;
    // (the format sets rp.marker and rp.in for its resolve variant)
    RT(f.enqueue(c, D, dx, hx, DO, dox, static_cast<uint32_t *>(d_tok), rp, s));
    RT(range_gather_dev(D.rjobs, (uint32_t)rjobs.size(), (uint32_t)tiles, static_cast<const uint8_t *>(d_dec), DO.bytes,
                        D.info, s));
    XT("launched");
    // the one download: the packed ranges and every status
    RT(download(c, slab.base, d_ro, ho_layout.total, s));
#undef RT
    XT("downloaded");
#undef XT
    f.counters.range_calls++;
    f.counters.units_tokenized += nu;
    f.counters.in_bytes_uploaded += plan.in_bytes;
    f.counters.out_bytes_decoded += plan.dec_bytes;
    const RangeOut HO = range_out(slab.base, f, &hox);
    // a unit's or segment's failure, in stream order: what the format
    // pre-marks, the tokenizer's status or the mismatch, then expand's, then
    // copy's
    std::vector<int32_t> ust(nu, ZT_OK);
    f.downloaded(hox, ust, &first);
    for (size_t u = 0; u < nu; ++u) {
      if (ust[u] == ZT_OK)
        ust[u] = HO.vstatus[2 * u] != ZT_OK ? HO.vstatus[2 * u] : HO.unit_status[u] < 0 ? HO.unit_status[u] : ZT_OK;
      if (ust[u] != ZT_OK && first == ZT_OK) {
        first = ust[u];
        first_detail = HO.vstatus[2 * u] != ZT_OK ? HO.vstatus[2 * u + 1] : 0;
      }
    }
    for (size_t g = 0; g < ns && first == ZT_OK; ++g)
      if (HO.seg_status[g] != ZT_OK) first = HO.seg_status[g] < 0 ? HO.seg_status[g] : ZT_E_INTERNAL;
    if (first != ZT_OK) {
      // the decode was abandoned (ChainInfo::ok): every range with bytes
      // fails, with its own span's first failure where it has one
      for (size_t i = 0; i < count; ++i) {
        const PlannedRange &r = plan.ranges[i];
        if (r.span < 0) continue;
        const auto &sp = plan.spans[r.span];
        status[i] = first;
        for (uint32_t k = 0; k <= sp.last - sp.first; ++k)
          if (ust[sp.unit0 + k] != ZT_OK) {
            status[i] = ust[sp.unit0 + k];
            break;
          }
      }
    }
  }
  return slab.hand_out(
      status, [&](size_t i) { return plan.ranges[i].dst; }, [&](size_t i) { return plan.ranges[i].len; },
      f.counters.out_bytes_returned, [&](size_t i) {
        return status[i] == ZT_E_ARG ? set_error(ZT_E_ARG, "range starts past the end of the output")
                                     : f.error(status[i], status[i] == first ? first_detail : 0);
      });
}

}  // namespace zt
