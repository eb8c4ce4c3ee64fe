// index_api.hip -- indexed random access (include/zt_index.h): the build call's
// host side, and the range calls with their two kernels.
//
// A range call plans everything on the host (index_host.h): the index already
// holds every unit's input position, output offset and token count, so the
// packed input, the stops, the TokJobs, the chain and its segments are known
// before anything runs.  The driver (range_call.h) carries them up in one
// upload; then, without the host waiting in between,
//   1. tokenize_kernel (inflate_tok.hip, unchanged) decodes the planned units,
//   2. range_verify_kernel compares every unit with what the index promised,
//   3. expand_kernel + copy_kernel (unchanged) write the spans to scratch --
//      or return at once when a unit failed its check (ChainInfo::ok),
//   4. range_gather_kernel (range_call.hip) copies the requested sub-ranges
//      into one packed buffer,
// and one download brings the ranges and every status back.  The scan, the
// sorts and the readbacks of the whole-stream path (inflate_seg.hip) are what
// the index replaces.
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "index_host.h"
#include "range_call.h"

namespace zt {

namespace {

struct RangeVerify {
  const uint8_t *in;       // the packed input
  const TokJob *jobs;
  const TokResult *res;
  const uint64_t *stops;   // stops[u]: where the index says unit u ends
  ChainUnit *cu;
  ChainInfo *info;
  int32_t *vstatus;        // [2 u]: unit u's verdict, [2 u + 1]: its detail (inflate_error's second argument)
  int32_t *unit_status;
  int32_t *seg_status;
  uint32_t nunits, nseg;
  uint32_t final_unit;     // the planned unit that ends at BFINAL (0xFFFFFFFF: none)
};

// One lane per planned unit: its tokenize result against the index.  A unit
// that is not the stream's last must have stopped on its own stop, which must
// be a sync point of this input (00 00 FF FF before it: the tokenizer does not
// look at a stored block's NLEN); the last one must have ended at BFINAL on
// the index's end position.  Output length and token count must be the
// index's (the uploaded chain unit holds both): the chain and the token slots
// were laid out from them.  A unit in
// order gets its tokenize flags into the chain (bit 31: run tokens; never bit
// 30: no segment is copied by expand here); one out of order loses its
// tokens and clears ChainInfo::ok, so that expand and copy do nothing.
__global__ __launch_bounds__(256) void range_verify_kernel(RangeVerify P) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  if (u < P.nseg) P.seg_status[u] = kNotRun;
  if (u >= P.nunits) return;
  P.unit_status[u] = kNotRun;
  const TokResult r = P.res[u];
  const TokJob j = P.jobs[u];
  const uint64_t end = P.stops[u];
  int32_t st = ZT_OK;
  if (r.status != ZT_OK) {
    // (a full token slot: the unit holds more tokens than the index's count and one stored payload)
    st = r.status == ZT_E_NOMEM ? ZT_E_INDEX_MISMATCH : r.status;
  } else {
    bool ok;
    if (u == P.final_unit) {
      ok = r.stop_idx < 0 && ((r.end_bits + 7) >> 3) == end;
    } else {
      ok = r.stop_idx == (int32_t)u && r.end_bits == end * 8 && end >= j.start + 4;
      if (ok) {
        const uint8_t *q = P.in + end - 4;
        ok = q[0] == 0 && q[1] == 0 && q[2] == 0xFF && q[3] == 0xFF;
      }
    }
    ok = ok && r.out_len == P.cu[u].out_len && (r.ntok & 0x3FFFFFFFu) == P.cu[u].ntok;
    if (!ok) st = ZT_E_INDEX_MISMATCH;
  }
  P.vstatus[2 * u] = st;
  P.vstatus[2 * u + 1] = r.detail;
  if (st != ZT_OK) {
    P.cu[u].ntok = 0;
    P.info->ok = 0;
  } else {
    P.cu[u].ntok = r.ntok & ~0x40000000u;
  }
}

struct IndexCounters : RangeCounters {
  std::atomic<uint64_t> builds{0};
};
IndexCounters g_ix;

int index_error(int status, int detail) {
  if (status == ZT_E_INDEX_MISMATCH) return set_error(status, "index does not match the stream");
  return inflate_error(status, detail);
}

// inputs up to this size are staged with the tables and go up in one copy;
// larger spans are uploaded from the caller's buffer (chunked, upload())
constexpr size_t kRangeStageMax = 32u << 20;

// what the sync-point index hands the range-call driver (range_call.h)
struct IndexFormat {
  static constexpr const char *kTag = "index", *kUpload = "hipMemcpyAsync (range tables)";
  const uint8_t *in;
  const IndexView &v;
  const RangePlan &plan;
  RangeCounters &counters;
  // in the upload: stops | jobs; device-only: the unit results
  struct Tables {
    uint64_t *stops;
    TokJob *jobs;
    TokResult *res;
  };
  struct Out {};
  void carve_upload(Carve &cv, Tables *t) const {
    t->stops = cv.take<uint64_t>(plan.stops.size());
    t->jobs = cv.take<TokJob>(plan.jobs.size());
  }
  void carve_device(Carve &cv, Tables *t) const { t->res = cv.take<TokResult>(plan.jobs.size()); }
  void carve_out(Carve &, Out *) const {}
  int admit(const RangeTables &, bool *staged) const {
    // every span but the stream's first starts at a sync point of this input
    for (const RangeSpan &s : plan.spans) {
      if (s.first == 0) continue;
      const uint64_t p = v.in_off[s.first];
      static const uint8_t kSync[4] = {0, 0, 0xFF, 0xFF};
      if (p < v.stream_start + 4 || memcmp(in + p - 4, kSync, 4) != 0) return index_error(ZT_E_INDEX_MISMATCH, 0);
    }
    *staged = plan.in_total <= kRangeStageMax;
    return ZT_OK;
  }
  const uint8_t *span_src(const RangeSpan &sp) const { return in + v.in_off[sp.first]; }
  void fill(const RangeTables &, const Tables &H) const {
    memcpy(H.stops, plan.stops.data(), plan.stops.size() * sizeof(uint64_t));
    memcpy(H.jobs, plan.jobs.data(), plan.jobs.size() * sizeof(TokJob));
  }
  int enqueue(DeviceCtx *, const RangeTables &D, const Tables &X, const Tables &, const RangeOut &DO, const Out &,
              uint32_t *d_tok, ResolveParams rp, hipStream_t s) const {
    const size_t nu = plan.jobs.size();
    ZT_TRY(tokenize_units_dev(tok_params_planned(D.in, plan.in_total, X.stops, nu, X.jobs, X.res, d_tok, (uint32_t)nu), s));
    RangeVerify rv;
    rv.in = D.in;
    rv.jobs = X.jobs;
    rv.res = X.res;
    rv.stops = X.stops;
    rv.cu = D.chain;
    rv.info = D.info;
    rv.vstatus = DO.vstatus;
    rv.unit_status = DO.unit_status;
    rv.seg_status = DO.seg_status;
    rv.nunits = (uint32_t)nu;
    rv.nseg = rp.nseg;
    rv.final_unit = plan.final_unit;
    range_verify_kernel<<<(uint32_t)((nu + 255) / 256), 256, 0, s>>>(rv);
    if (hipGetLastError() != hipSuccess) return set_error(ZT_E_HIP, "range_verify_kernel launch failed");
    rp.marker = 0;
    rp.in = D.in;
    return resolve_segments_dev(rp, s);
  }
  void downloaded(const Out &, std::vector<int32_t> &, int *) const {}
  int error(int status, int detail) const { return index_error(status, detail); }
};

int ranges_impl(const uint8_t *in, size_t n, const uint8_t *idx, size_t idx_len, const uint64_t *off,
                const uint64_t *len, size_t count, uint8_t **out, size_t *out_len, int *status) {
  IndexView v;
  if (const char *why = index_validate(idx, idx_len, n, &v))
    return set_error(ZT_E_INDEX, std::string("invalid index: ") + why);
  const RangePlan plan = index_plan(v, off, len, count);
  return range_call(IndexFormat{in, v, plan, g_ix}, count, out, out_len, status);
}

}  // namespace

}  // namespace zt

using namespace zt;

extern "C" {

int zt_inflate_index_build(const uint8_t *in, size_t n, size_t index, uint8_t **idx, size_t *idx_len, uint8_t **out,
                           size_t *out_len, size_t *end_ip) {
  if (!idx || !idx_len || (out && !out_len)) return set_error(ZT_E_ARG, "null output");
  if (!in && n) return set_error(ZT_E_ARG, "null input");
  *idx = nullptr;
  *idx_len = 0;
  if (out) *out = nullptr;
  int rc = 1;
  if (n > index) {
    DeviceCtx *c;
    ZT_TRY(get_ctx(&c));
    std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
    void *d_in;
    ZT_TRY(scratch(c, kIn, n, &d_in));
    ZT_TRY(upload(c, d_in, in, n, c->stream));
    uint8_t *d_out = nullptr;
    size_t ol = 0, eip = 0;
    std::vector<uint8_t> blob;
    rc = inflate_index_build_dev(c, static_cast<const uint8_t *>(d_in), n, index, &d_out, &ol, &eip, &blob, c->stream);
    if (rc < 0) return rc;
    if (rc == 0) {
      uint8_t *hb = host_out(blob.size());
      if (!hb) return set_error(ZT_E_NOMEM, "host allocation failed");
      memcpy(hb, blob.data(), blob.size());
      if (out) {
        uint8_t *h = host_out(ol, true);
        if (!h) {
          zt_free(hb);
          return set_error(ZT_E_NOMEM, "host allocation failed");
        }
        if (const int drc = download(c, h, d_out, ol, c->stream)) {
          zt_free(h);
          zt_free(hb);
          return drc;
        }
        *out = h;
        *out_len = ol;
      } else if (out_len) {
        *out_len = ol;
      }
      if (end_ip) *end_ip = eip;
      *idx = hb;
      *idx_len = blob.size();
      g_ix.builds++;
      return ZT_OK;
    }
  }
  // off the sync-point path: a corrupt stream reports its own status (the
  // whole-stream call finds it), any other has no index
  uint8_t *o = nullptr;
  size_t ol = 0, eip = 0;
  const int wrc = zt_inflate_raw(in, n, index, nullptr, &o, &ol, &eip);
  if (wrc != ZT_OK) return wrc;
  zt_free(o);
  return set_error(ZT_E_NO_INDEX, "stream has no usable sync points");
}

int zt_inflate_ranges(const uint8_t *in, size_t n, const uint8_t *idx, size_t idx_len, const uint64_t *off,
                      const uint64_t *len, size_t count, uint8_t **out, size_t *out_len, int *status) {
  if (count == 0) return ZT_OK;
  if (!off || !len || !out || !out_len || !status) return set_error(ZT_E_ARG, "null argument");
  if ((!in && n) || !idx) return set_error(ZT_E_ARG, "null input");
  return ranges_impl(in, n, idx, idx_len, off, len, count, out, out_len, status);
}

int zt_inflate_range(const uint8_t *in, size_t n, const uint8_t *idx, size_t idx_len, uint64_t off, uint64_t len,
                     uint8_t **out, size_t *out_len) {
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if ((!in && n) || !idx) return set_error(ZT_E_ARG, "null input");
  int st = ZT_OK;
  return ranges_impl(in, n, idx, idx_len, &off, &len, 1, out, out_len, &st);
}

int zt_index_stats_read(zt_index_stats *out, int reset) {
  if (!out) return set_error(ZT_E_ARG, "null output");
  out->builds = stat_take(g_ix.builds, reset);
  out->range_calls = stat_take(g_ix.range_calls, reset);
  out->ranges = stat_take(g_ix.ranges, reset);
  out->units_tokenized = stat_take(g_ix.units_tokenized, reset);
  out->in_bytes_uploaded = stat_take(g_ix.in_bytes_uploaded, reset);
  out->out_bytes_decoded = stat_take(g_ix.out_bytes_decoded, reset);
  out->out_bytes_returned = stat_take(g_ix.out_bytes_returned, reset);
  return ZT_OK;
}

}  // extern "C"
