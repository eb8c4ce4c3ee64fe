// index_api.hip -- indexed random access (include/zt_index.h): the build call's
// host side, and the range calls with their two kernels.
//
// A range call plans everything on the host (index_host.h): the index already
// holds every unit's input position, output offset and token count, so the
// packed input, the stops, the TokJobs, the chain and its segments are known
// before anything runs.  One upload carries them; then, without the host
// waiting in between,
//   1. tokenize_kernel (inflate_tok.hip, unchanged) decodes the planned units,
//   2. range_verify_kernel compares every unit with what the index promised,
//   3. expand_kernel + copy_kernel (unchanged) write the spans to scratch --
//      or return at once when a unit failed its check (ChainInfo::ok),
//   4. range_gather_kernel copies the requested sub-ranges into one packed
//      buffer,
// and one download brings the ranges and every status back.  The scan, the
// sorts and the readbacks of the whole-stream path (inflate_seg.hip) are what
// the index replaces.
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "index_host.h"
#include "zt_internal.h"

namespace zt {

namespace {

// a status slot nobody has written (expand / copy returned at once)
constexpr int32_t kNotRun = 1;

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

// (RangeJob, kGatherTile: zt_internal.h -- the checkpoint range decode gathers the same way)
typedef unsigned int u32x4g __attribute__((ext_vector_type(4)));

// One workgroup per range and tile.  The destination is 16-byte aligned at
// every tile start, so the body goes out as 16-byte stores; each comes from
// the two aligned 16-byte source words around it, shifted by the range's
// source misalignment (uniform in the workgroup).  The last len % 16 bytes of
// a range go byte by byte.  (A job whose destination is not 16-byte aligned --
// the pieces of a BGZF range, packed back to back: bgzf_api.hip -- sends the
// bytes up to the next 16-byte boundary one by one first; `out` itself is
// aligned, so the ranges of the index calls have none.)
__global__ __launch_bounds__(256) void range_gather_kernel(const RangeJob *__restrict__ jobs, uint32_t njobs,
                                                           const uint8_t *__restrict__ dec, uint8_t *__restrict__ out,
                                                           const ChainInfo *__restrict__ info) {
  if (!info->ok) return;
  uint32_t lo = 0, hi = njobs;  // the last job with tile0 <= blockIdx.x
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (jobs[mid].tile0 <= blockIdx.x)
      lo = mid;
    else
      hi = mid;
  }
  const RangeJob j = jobs[lo];
  const uint64_t o0 = (uint64_t)(blockIdx.x - j.tile0) * kGatherTile;
  if (o0 >= j.len) return;
  uint32_t n = (uint32_t)(j.len - o0 < kGatherTile ? j.len - o0 : kGatherTile);
  const uint8_t *s = dec + j.src + o0;
  uint8_t *d = out + j.dst + o0;
  const uint32_t to16 = (uint32_t)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15);
  const uint32_t lead = to16 < n ? to16 : n;
  for (uint32_t i = threadIdx.x; i < lead; i += 256) d[i] = s[i];
  s += lead;
  d += lead;
  n -= lead;
  const uint32_t body = n & ~15u;
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 15);
  const u32x4g *sa = reinterpret_cast<const u32x4g *>(s - sh);
  const uint32_t q = sh >> 2, r = sh & 3;
  for (uint32_t i = threadIdx.x * 16; i < body; i += 256 * 16) {
    // (sh != 0: the second word starts before s + i + 16 <= s + n, inside the span)
    const u32x4g a = sa[i / 16];
    const u32x4g b = sh ? sa[i / 16 + 1] : a;
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t v[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = q == 0 ? w[k] : q == 1 ? w[k + 1] : q == 2 ? w[k + 2] : w[k + 3];
    u32x4g o;
    o.x = __builtin_amdgcn_alignbyte(v[1], v[0], r);
    o.y = __builtin_amdgcn_alignbyte(v[2], v[1], r);
    o.z = __builtin_amdgcn_alignbyte(v[3], v[2], r);
    o.w = __builtin_amdgcn_alignbyte(v[4], v[3], r);
    *reinterpret_cast<u32x4g *>(d + i) = o;
  }
  for (uint32_t i = body + threadIdx.x; i < n; i += 256) d[i] = s[i];
}

struct IndexCounters {
  std::atomic<uint64_t> builds{0}, range_calls{0}, ranges{0}, units_tokenized{0}, in_bytes_uploaded{0},
      out_bytes_decoded{0}, out_bytes_returned{0};
};
IndexCounters g_ix;

// ZT_INDEX_TIMING=1: host wall time of a range call's stages on stderr (measurement only)
#define XT(label) ZT_STAMP("ZT_INDEX_TIMING", "index", label)

int index_error(int status, int detail) {
  if (status == ZT_E_INDEX_MISMATCH) return set_error(status, "index does not match the stream");
  return inflate_error(status, detail);
}

// the one upload's layout (kRangeIn and its pinned mirror), then the device-only unit results
struct RangeTables {
  uint64_t *stops;
  TokJob *jobs;
  ChainUnit *chain;
  SegJob *segs;
  RangeJob *rjobs;
  ChainInfo *info;
  size_t table_bytes;   // the tables alone
  uint8_t *in;
  size_t upload_bytes;  // tables and packed input
  TokResult *res;
  size_t bytes;
};
RangeTables range_tables(void *base, const RangePlan &p, size_t njobs) {
  Carve cv(base);
  RangeTables t;
  t.stops = cv.take<uint64_t>(p.stops.size());
  t.jobs = cv.take<TokJob>(p.jobs.size());
  t.chain = cv.take<ChainUnit>(p.chain.size());
  t.segs = cv.take<SegJob>(p.segs.size());
  t.rjobs = cv.take<RangeJob>(njobs);
  t.info = cv.take<ChainInfo>(1);
  t.table_bytes = cv.bytes();
  t.in = cv.take<uint8_t>(p.in_total + 256);  // + slack: the reader's aligned loads
  t.upload_bytes = cv.bytes();
  t.res = cv.take<TokResult>(p.jobs.size());
  t.bytes = cv.bytes();
  return t;
}
// the one download's layout (kRangeOut; the host slab mirrors it)
struct RangeOut {
  uint8_t *bytes;
  int32_t *vstatus, *unit_status, *seg_status;
  size_t total;
};
RangeOut range_out(void *base, const RangePlan &p) {
  Carve cv(base);
  RangeOut o;
  o.bytes = cv.take<uint8_t>(p.dst_total);
  o.vstatus = cv.take<int32_t>(2 * p.jobs.size());
  o.unit_status = cv.take<int32_t>(p.jobs.size());
  o.seg_status = cv.take<int32_t>(p.segs.size());
  o.total = cv.bytes();
  return o;
}

// inputs up to this size are staged with the tables and go up in one copy;
// larger spans are uploaded from the caller's buffer (chunked, upload())
constexpr size_t kRangeStageMax = 32u << 20;

int ranges_impl(const uint8_t *in, size_t n, const uint8_t *idx, size_t idx_len, const uint64_t *off,
                const uint64_t *len, size_t count, uint8_t **out, size_t *out_len, int *status) {
  IndexView v;
  if (const char *why = index_validate(idx, idx_len, n, &v))
    return set_error(ZT_E_INDEX, std::string("invalid index: ") + why);
  const RangePlan plan = index_plan(v, off, len, count);
  g_ix.ranges += count;
  for (size_t i = 0; i < count; ++i) {
    out[i] = nullptr;
    out_len[i] = 0;
    status[i] = plan.ranges[i].status;
  }
  // every span but the stream's first starts at a sync point of this input
  for (const IdxSpan &s : plan.spans) {
    if (s.first == 0) continue;
    const uint64_t p = v.in_off[s.first];
    static const uint8_t kSync[4] = {0, 0, 0xFF, 0xFF};
    if (p < v.stream_start + 4 || memcmp(in + p - 4, kSync, 4) != 0) return index_error(ZT_E_INDEX_MISMATCH, 0);
  }
  const size_t nu = plan.jobs.size(), ns = plan.segs.size();
  std::vector<RangeJob> rjobs;
  uint64_t tiles = 0;
  for (const IdxRange &r : plan.ranges) {
    if (r.span < 0) continue;
    rjobs.push_back(RangeJob{r.src, r.dst, r.len, (uint32_t)tiles, 0});
    tiles += (r.len + kGatherTile - 1) / kGatherTile;
  }
  if (tiles > 0x7FFFFFFFull || nu > 0x7FFFFFFFull) return set_error(ZT_E_ARG, "too many ranges for one call");
  const RangeOut ho_layout = range_out(nullptr, plan);
  uint8_t *slab = slab_out(nu ? ho_layout.total : plan.dst_total, count, true);
  if (!slab) return set_error(ZT_E_NOMEM, "host allocation failed");
  auto give_up = [&](int rc) {
    for (size_t i = 0; i < count; ++i) slab_release(slab);
    for (size_t i = 0; i < count; ++i) out[i] = nullptr, out_len[i] = 0;
    return rc;
  };
  int first = ZT_OK, first_detail = 0;
  if (nu) {  // (nothing to decode: no GPU touched)
    DeviceCtx *c;
    if (const int rc = get_ctx(&c)) return give_up(rc);
    std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
    hipStream_t s = c->stream;
    XT("planned");
    const RangeTables lay = range_tables(nullptr, plan, rjobs.size());
    const bool staged = plan.in_total <= kRangeStageMax;
    void *d_tab, *h_tab, *d_tok, *d_desc, *d_dec, *d_ro;
#define RT(call)                            \
  do {                                      \
    if (const int rc_ = (call)) return give_up(rc_); \
  } while (0)
    RT(scratch(c, kRangeIn, lay.bytes, &d_tab));
    RT(pinned(c, staged ? lay.upload_bytes : lay.table_bytes, &h_tab, kPinBatch));
    RT(scratch(c, kTokens, ((size_t)plan.tok_total + 256) * 4, &d_tok));  // + slack: chunked token reads
    RT(scratch(c, kDeflateOrDesc, ((size_t)plan.desc_total + 1024) * 2, &d_desc));  // + slack: chunked descriptor reads
    RT(scratch(c, kOut, (size_t)plan.dec_total + 256, &d_dec));
    RT(scratch(c, kRangeOut, ho_layout.total, &d_ro));
    const RangeTables D = range_tables(d_tab, plan, rjobs.size()), H = range_tables(h_tab, plan, rjobs.size());
    const RangeOut DO = range_out(d_ro, plan);
    // the one upload: [stops | jobs | chain | segments | ranges | chain summary | packed spans]
    for (const IdxSpan &sp : plan.spans)
      if (staged) copy_to_staging(H.in + sp.in_pos, in + v.in_off[sp.first], sp.in_len);
    memcpy(H.stops, plan.stops.data(), nu * sizeof(uint64_t));
    memcpy(H.jobs, plan.jobs.data(), nu * sizeof(TokJob));
    memcpy(H.chain, plan.chain.data(), nu * sizeof(ChainUnit));
    memcpy(H.segs, plan.segs.data(), ns * sizeof(SegJob));
    if (!rjobs.empty()) memcpy(H.rjobs, rjobs.data(), rjobs.size() * sizeof(RangeJob));
    *H.info = ChainInfo{1, (uint32_t)ns, plan.dec_total, 0, plan.desc_total};
    {
      const hipError_t e = hipMemcpyAsync(d_tab, h_tab, staged ? lay.upload_bytes : lay.table_bytes,
                                          hipMemcpyHostToDevice, s);
      if (e != hipSuccess) return give_up(hip_fail(e, "hipMemcpyAsync (range tables)"));
    }
    if (!staged)
      for (const IdxSpan &sp : plan.spans) RT(upload(c, D.in + sp.in_pos, in + v.in_off[sp.first], sp.in_len, s));
    XT("uploaded");
    TokParams tp;
    tp.in = D.in;
    tp.n = plan.in_total;
    tp.order = nullptr;
    tp.stops = D.stops;
    tp.nstops = nu;
    tp.jobs = D.jobs;
    tp.res = D.res;
    tp.tokens = static_cast<uint32_t *>(d_tok);
    tp.count = (uint32_t)nu;
    tp.simt = tok_simt_env();
    tp.dbg = nullptr;
    tp.dump_unit = 0xFFFFFFFFu;
    tp.dump_once = 0;
    tp.run_tokens = 1;
    RT(tokenize_units_dev(tp, s));
    RangeVerify rv;
    rv.in = D.in;
    rv.jobs = D.jobs;
    rv.res = D.res;
    rv.stops = D.stops;
    rv.cu = D.chain;
    rv.info = D.info;
    rv.vstatus = DO.vstatus;
    rv.unit_status = DO.unit_status;
    rv.seg_status = DO.seg_status;
    rv.nunits = (uint32_t)nu;
    rv.nseg = (uint32_t)ns;
    rv.final_unit = plan.final_unit;
    range_verify_kernel<<<(uint32_t)((nu + 255) / 256), 256, 0, s>>>(rv);
    if (hipGetLastError() != hipSuccess) return give_up(set_error(ZT_E_HIP, "range_verify_kernel launch failed"));
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
    rp.marker = 0;
    rp.in = D.in;
    rp.info = D.info;
    rp.order = nullptr;
    RT(resolve_segments_dev(rp, s));
    if (tiles) {
      range_gather_kernel<<<(uint32_t)tiles, 256, 0, s>>>(D.rjobs, (uint32_t)rjobs.size(),
                                                          static_cast<const uint8_t *>(d_dec), DO.bytes, D.info);
      if (hipGetLastError() != hipSuccess) return give_up(set_error(ZT_E_HIP, "range_gather_kernel launch failed"));
    }
    XT("launched");
    // the one download: the packed ranges and every status
    RT(download(c, slab, d_ro, ho_layout.total, s));
#undef RT
    XT("downloaded");
    g_ix.range_calls++;
    g_ix.units_tokenized += nu;
    g_ix.in_bytes_uploaded += plan.in_bytes;
    g_ix.out_bytes_decoded += plan.dec_bytes;
    const RangeOut HO = range_out(slab, plan);
    // a unit's or segment's failure, in stream order: the tokenizer's status
    // or the index mismatch, then expand's, then copy's
    std::vector<int32_t> ust(nu, ZT_OK);
    for (size_t u = 0; u < nu; ++u) {
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
        const IdxRange &r = plan.ranges[i];
        if (r.span < 0) continue;
        const IdxSpan &sp = plan.spans[r.span];
        status[i] = first;
        for (uint32_t k = 0; k <= sp.last - sp.first; ++k)
          if (ust[sp.unit0 + k] != ZT_OK) {
            status[i] = ust[sp.unit0 + k];
            break;
          }
      }
    }
  }
  int rc = ZT_OK;
  for (size_t i = 0; i < count; ++i) {
    if (status[i] != ZT_OK) {
      slab_release(slab);
      if (rc == ZT_OK)
        rc = status[i] == ZT_E_ARG ? set_error(ZT_E_ARG, "range starts past the end of the output")
                                   : index_error(status[i], status[i] == first ? first_detail : 0);
      continue;
    }
    out[i] = slab + plan.ranges[i].dst;
    out_len[i] = (size_t)plan.ranges[i].len;
    g_ix.out_bytes_returned += plan.ranges[i].len;
  }
  return rc;
}

}  // namespace

int range_gather_dev(const RangeJob *d_jobs, uint32_t njobs, uint32_t tiles, const uint8_t *d_dec, uint8_t *d_out,
                     const ChainInfo *d_info, hipStream_t s) {
  if (tiles == 0) return ZT_OK;
  range_gather_kernel<<<tiles, 256, 0, s>>>(d_jobs, njobs, d_dec, d_out, d_info);
  ZT_HIP(hipGetLastError());
  return ZT_OK;
}

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
  auto take = [&](std::atomic<uint64_t> &a) { return reset ? a.exchange(0) : a.load(); };
  out->builds = take(g_ix.builds);
  out->range_calls = take(g_ix.range_calls);
  out->ranges = take(g_ix.ranges);
  out->units_tokenized = take(g_ix.units_tokenized);
  out->in_bytes_uploaded = take(g_ix.in_bytes_uploaded);
  out->out_bytes_decoded = take(g_ix.out_bytes_decoded);
  out->out_bytes_returned = take(g_ix.out_bytes_returned);
  return ZT_OK;
}

}  // extern "C"
