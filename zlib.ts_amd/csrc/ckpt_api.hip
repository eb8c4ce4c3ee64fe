// ckpt_api.hip -- the checkpoint index (include/zt_checkpoint.h): random access
// into streams without sync points.
//
// The build runs the general decode once (inflate_gen.hip) and keeps what it
// used to throw away: every chain unit's exact end state and that state's
// output offset.  ckpt_window_kernel then copies the 32 KiB of output in front
// of every window checkpoint into the blob's window table, the checksum
// kernels (checksum.hip) give each its CRC-32, and one download brings the
// table back.
//
// A range call plans everything on the host (ckpt_host.h): the blob holds
// every unit's start state, end state, output offset and token count, so the
// packed input, the relocated block headers, the units, the chain and its
// segments are known before anything runs.  The driver (range_call.h) carries
// them and the windows the segments start from up in one upload; then, without
// the host waiting in between,
//   1. the checksum kernels give every uploaded window its CRC-32,
//   2. gen_tokenize_kernel (inflate_gen.hip) decodes the planned units, each an
//      exact start, one wave per unit, all in parallel,
//   3. ckpt_verify_kernel holds every unit to the next entry and every window
//      to its CRC,
//   4. expand_kernel + copy_window_kernel (inflate_tok.hip) write the spans to
//      scratch -- or return at once when anything failed (ChainInfo::ok),
//   5. range_gather_kernel (range_call.hip) packs the requested sub-ranges,
// and one download brings the ranges and every status back.  Candidate
// search, speculation, link passes and the window chain of the whole-stream
// path are what the blob replaces.
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "ckpt_host.h"
#include "range_call.h"

namespace zt {

static_assert(CK_BLOCK == GK_BLOCK && CK_HUFF == GK_HUFF && CK_STORED == GK_STORED && CK_SHDR == GK_SHDR &&
                  CK_FINAL == GK_FINAL && kCkFixedHdr == kFixedHdr,
              "the blob's kinds are the general tokenizer's");
static_assert(kCkWindow == 32768, "a window is the copy kernels' history ring");

namespace {

// ---- the build's window table ----------------------------------------------------
// One workgroup per window checkpoint: out[off - 32768, off) into the window's
// record, the record's tail zeroed (ckpt_crc_place_kernel fills the CRC in).
// The source is not aligned; the record is (16 bytes).
__global__ __launch_bounds__(256) void ckpt_window_kernel(const uint8_t *__restrict__ out,
                                                          const uint64_t *__restrict__ offs,
                                                          uint8_t *__restrict__ table) {
  const uint32_t w = blockIdx.x;
  const uint8_t *s = out + (offs[w] - kCkWindow);
  uint32_t *d = reinterpret_cast<uint32_t *>(table + (size_t)w * kCkWinRec);
  for (uint32_t i = threadIdx.x; i < (uint32_t)kCkWinRec / 4; i += 256) {
    uint32_t v = 0;
    if (i < (uint32_t)kCkWindow / 4)
      v = (uint32_t)s[4 * i] | ((uint32_t)s[4 * i + 1] << 8) | ((uint32_t)s[4 * i + 2] << 16) |
          ((uint32_t)s[4 * i + 3] << 24);
    d[i] = v;
  }
}
// crc[2 w] (checksums_batch_dev's layout) into record w
__global__ __launch_bounds__(256) void ckpt_crc_place_kernel(const uint32_t *__restrict__ crc, uint32_t nwin,
                                                             uint8_t *__restrict__ table) {
  const uint32_t w = blockIdx.x * 256 + threadIdx.x;
  if (w < nwin) *reinterpret_cast<uint32_t *>(table + (size_t)w * kCkWinRec + kCkWindow) = crc[2 * w];
}

// ---- the range decode's check -------------------------------------------------------
// what the next entry says a planned unit ends in (packed-input positions)
struct CkExpect {
  uint64_t pos, hdr;
  uint32_t kind, rem, bfinal, ntok, out_len, pad;
};
struct CkVerify {
  const GenResult *res;
  const CkExpect *exp;
  ChainUnit *cu;
  ChainInfo *info;
  const uint32_t *crc_got;   // [2 w]: uploaded window w's CRC-32 as computed here
  const uint32_t *crc_want;  // [w]: the blob's
  int32_t *vstatus;          // [2 u]: unit u's verdict, [2 u + 1]: its detail
  int32_t *unit_status;
  int32_t *seg_status;
  int32_t *win_status;
  uint32_t nunits, nseg, nwin;
};

// One lane per planned unit: its end state must be the next entry's (kind and
// bit position; header and BFINAL inside a Huffman body, bytes left and BFINAL
// inside a stored payload, BFINAL at a stored length field; the stream's last
// unit must have reached BFINAL on the sentinel's bit), its output length the
// difference of the two out_offs and its token count the entry's: the chain
// and the token slots were laid out from them.  One lane per uploaded window:
// its CRC-32 must be the blob's.  Anything out of order clears ChainInfo::ok,
// so that expand, copy and gather do nothing; a unit out of order also loses
// its tokens.
__global__ __launch_bounds__(256) void ckpt_verify_kernel(CkVerify P) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  if (u < P.nseg) P.seg_status[u] = kNotRun;
  if (u < P.nwin) {
    const bool ok = P.crc_got[2 * u] == P.crc_want[u];
    P.win_status[u] = ok ? ZT_OK : ZT_E_INDEX;
    if (!ok) P.info->ok = 0;
  }
  if (u >= P.nunits) return;
  P.unit_status[u] = kNotRun;
  const GenResult r = P.res[u];
  const CkExpect x = P.exp[u];
  int32_t st = ZT_OK;
  if (r.status != ZT_OK) {
    // (a full token slot: the unit holds more tokens than the entry's count)
    st = r.status == ZT_E_NOMEM ? ZT_E_INDEX_MISMATCH : r.status;
  } else {
    const GenState e = r.end;
    bool ok = e.kind == x.kind && e.pos == x.pos;
    if (x.kind == GK_HUFF) ok = ok && e.hdr == x.hdr && e.bfinal == x.bfinal;
    if (x.kind == GK_STORED) ok = ok && e.rem == x.rem && e.bfinal == x.bfinal;
    if (x.kind == GK_SHDR) ok = ok && e.bfinal == x.bfinal;
    ok = ok && r.out_stop == x.out_len && r.out_len == x.out_len && r.ntok_stop == x.ntok && r.ntok == x.ntok;
    if (!ok) st = ZT_E_INDEX_MISMATCH;
  }
  P.vstatus[2 * u] = st;
  P.vstatus[2 * u + 1] = r.detail;
  if (st != ZT_OK) {
    P.cu[u].ntok = 0;
    P.info->ok = 0;
  }
}

struct CkptCounters : RangeCounters {
  std::atomic<uint64_t> builds{0}, window_bytes_uploaded{0};
};
CkptCounters g_ck;

int ckpt_error(int status, int detail) {
  if (status == ZT_E_INDEX_MISMATCH) return set_error(status, "checkpoint blob does not match the stream");
  if (status == ZT_E_INDEX) return set_error(status, "invalid checkpoint blob: a window fails its CRC-32");
  return inflate_error(status, detail);
}

// one call's upload is staged whole; a call that asks for more is refused
constexpr size_t kCkptStageMax = 1u << 30;

// what the checkpoint blob hands the range-call driver (range_call.h)
struct CkptFormat {
  static constexpr const char *kTag = "ckpt", *kUpload = "hipMemcpyAsync (checkpoint range tables)";
  const uint8_t *in;
  const CkptView &v;
  const CkptPlan &plan;
  RangeCounters &counters;
  // in the upload: units | end states | the segments' windows | CRCs | windows
  // (the packed input holds the block headers, then the spans); device-only:
  // the unit results and the windows' CRCs as computed
  struct Tables {
    GenJob *jobs;
    CkExpect *exp;
    int32_t *seg_win;
    uint32_t *crc_want;
    uint64_t *win_off, *win_len;  // checksums_batch_dev reads these on the host: the mirror's only
    uint8_t *wins;
    GenResult *res;
    uint32_t *crc_got;
  };
  struct Out {
    int32_t *win_status;
  };
  void carve_upload(Carve &cv, Tables *t) const {
    const size_t nu = plan.units.size(), nw = plan.wins.size();
    t->jobs = cv.take<GenJob>(nu);
    t->exp = cv.take<CkExpect>(nu);
    t->seg_win = cv.take<int32_t>(plan.segs.size());
    t->crc_want = cv.take<uint32_t>(nw);
    t->win_off = cv.take<uint64_t>(nw);
    t->win_len = cv.take<uint64_t>(nw);
    t->wins = cv.take<uint8_t>(nw * kCkWindow);
  }
  void carve_device(Carve &cv, Tables *t) const {
    t->res = cv.take<GenResult>(plan.units.size());
    t->crc_got = cv.take<uint32_t>(2 * plan.wins.size());
  }
  void carve_out(Carve &cv, Out *o) const { o->win_status = cv.take<int32_t>(plan.wins.size()); }
  int admit(const RangeTables &lay, bool *staged) const {
    if (lay.upload_bytes > kCkptStageMax) return set_error(ZT_E_ARG, "ranges too large for one call");
    *staged = true;
    return ZT_OK;
  }
  const uint8_t *span_src(const CkSpan &sp) const { return in + sp.byte0; }
  void fill(const RangeTables &T, const Tables &H) const {
    for (size_t u = 0; u < plan.units.size(); ++u) {
      const CkUnit &j = plan.units[u];
      GenJob g{};
      g.st.pos = j.pos;
      g.st.hdr = j.hdr;
      g.st.kind = j.kind;
      g.st.rem = j.rem;
      g.st.bfinal = j.bfinal;
      g.stop = j.stop;
      g.tok_off = j.tok_off;
      g.tok_cap = j.tok_cap;
      g.spec = 0;
      H.jobs[u] = g;
      H.exp[u] = CkExpect{j.e_pos, j.e_hdr, j.e_kind, j.e_rem, j.e_bfinal, j.ntok, j.out_len, 0};
    }
    memcpy(H.seg_win, plan.seg_win.data(), plan.seg_win.size() * sizeof(int32_t));
    for (const CkHdr &h : plan.hdrs) {
      memcpy(T.in + h.slot, in + h.src, h.len);
      memset(T.in + h.slot + h.len, 0, kCkHdrSlot - h.len);
    }
    for (size_t w = 0; w < plan.wins.size(); ++w) {
      copy_to_staging(H.wins + w * kCkWindow, v.wins + (size_t)plan.wins[w] * kCkWinRec, kCkWindow);
      H.crc_want[w] = ckpt_window_crc(v, plan.wins[w]);
      H.win_off[w] = (uint64_t)w * kCkWindow;
      H.win_len[w] = kCkWindow;
    }
  }
  int enqueue(DeviceCtx *c, const RangeTables &D, const Tables &X, const Tables &H, const RangeOut &DO, const Out &DX,
              uint32_t *d_tok, ResolveParams rp, hipStream_t s) const {
    const size_t nu = plan.units.size(), nw = plan.wins.size();
    // (the checksum launcher's own small tables go up with blocking copies: it
    // comes first, so that those wait for the upload and for no kernel)
    if (nw) ZT_TRY(checksums_batch_dev(c, X.wins, nw, H.win_off, H.win_len, X.crc_got, s));
    ZT_TRY(gen_tokenize_exact_dev(D.in, plan.in_total, X.jobs, X.res, d_tok, (uint32_t)nu, s));
    CkVerify cv;
    cv.res = X.res;
    cv.exp = X.exp;
    cv.cu = D.chain;
    cv.info = D.info;
    cv.crc_got = X.crc_got;
    cv.crc_want = X.crc_want;
    cv.vstatus = DO.vstatus;
    cv.unit_status = DO.unit_status;
    cv.seg_status = DO.seg_status;
    cv.win_status = DX.win_status;
    cv.nunits = (uint32_t)nu;
    cv.nseg = rp.nseg;
    cv.nwin = (uint32_t)nw;
    const size_t lanes = std::max(nu, std::max<size_t>(rp.nseg, nw));
    ckpt_verify_kernel<<<(uint32_t)((lanes + 255) / 256), 256, 0, s>>>(cv);
    if (hipGetLastError() != hipSuccess) return set_error(ZT_E_HIP, "ckpt_verify_kernel launch failed");
    rp.marker = 1;  // a segment that is not the stream's first reaches into its window
    rp.in = nullptr;  // (the general tokenizer writes no run tokens)
    return resolve_segments_window_dev(rp, X.wins, X.seg_win, s);
  }
  // a window that fails its CRC fails the first unit of its segment
  void downloaded(const Out &HO, std::vector<int32_t> &ust, int *first) const {
    g_ck.window_bytes_uploaded += plan.wins.size() * kCkWindow;
    for (size_t g = 0; g < plan.segs.size(); ++g) {
      const int32_t w = plan.seg_win[g];
      if (w >= 0 && HO.win_status[w] != ZT_OK) {
        ust[plan.segs[g].first] = ZT_E_INDEX;
        if (*first == ZT_OK) *first = ZT_E_INDEX;
      }
    }
  }
  int error(int status, int detail) const { return ckpt_error(status, detail); }
};

int ckpt_ranges_impl(const uint8_t *in, size_t n, const uint8_t *idx, size_t idx_len, const uint64_t *off,
                     const uint64_t *len, size_t count, uint8_t **out, size_t *out_len, int *status) {
  CkptView v;
  if (const char *why = ckpt_validate(idx, idx_len, n, &v))
    return set_error(ZT_E_INDEX, std::string("invalid checkpoint blob: ") + why);
  const CkptPlan plan = ckpt_plan(v, n, off, len, count);
  return range_call(CkptFormat{in, v, plan, g_ck}, count, out, out_len, status);
}

// the blob of converged entries `e` (windows placed, nwin of them) with its
// window table filled from the decoded output, validated against the input
int ckpt_finish(DeviceCtx *c, std::vector<CkEntry> &e, uint32_t nwin, const uint8_t *d_out, size_t n, size_t index,
                size_t end_ip, size_t total, uint64_t span, uint8_t **blob_out, size_t *blob_len, hipStream_t s) {
  const size_t nunits = e.size() - 1;
  const size_t bytes = ckpt_blob_bytes(nunits, nwin);
  uint8_t *blob = host_out(bytes);
  if (!blob) return set_error(ZT_E_NOMEM, "host allocation failed");
  auto fail = [&](int rc) {
    zt_free(blob);
    return rc;
  };
  ckpt_write_header(blob, (uint32_t)nunits, nwin, index, end_ip, total, span);
  for (size_t k = 0; k <= nunits; ++k) ckpt_write_entry(blob, k, e[k]);
  if (nwin) {
    std::vector<uint64_t> offs, woff(nwin), wlen(nwin, kCkWindow);
    for (const CkEntry &x : e)
      if (x.flags & 1u) offs.push_back(x.out_off);
    for (uint32_t w = 0; w < nwin; ++w) woff[w] = (uint64_t)w * kCkWinRec;
    uint64_t *d_offs = nullptr;
    uint32_t *d_crc = nullptr;
    uint8_t *d_table = nullptr;
    if (const int rc = scratch_carved(c, kCkptWin, [&](void *base) {
          Carve cv(base);
          d_offs = cv.take<uint64_t>(nwin);
          d_crc = cv.take<uint32_t>(2 * (size_t)nwin);
          d_table = cv.take<uint8_t>((size_t)nwin * kCkWinRec);
          return cv.bytes();
        }))
      return fail(rc);
    if (hipMemcpyAsync(d_offs, offs.data(), (size_t)nwin * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)  // (offs is pageable and leaves scope)
      return fail(set_error(ZT_E_HIP, "hipMemcpyAsync (window offsets)"));
    ckpt_window_kernel<<<nwin, 256, 0, s>>>(d_out, d_offs, d_table);
    if (hipGetLastError() != hipSuccess) return fail(set_error(ZT_E_HIP, "ckpt_window_kernel launch failed"));
    if (const int rc = checksums_batch_dev(c, d_table, nwin, woff.data(), wlen.data(), d_crc, s)) return fail(rc);
    ckpt_crc_place_kernel<<<(nwin + 255) / 256, 256, 0, s>>>(d_crc, nwin, d_table);
    if (hipGetLastError() != hipSuccess) return fail(set_error(ZT_E_HIP, "ckpt_crc_place_kernel launch failed"));
    // the one download: the finished window table, straight into the blob
    if (const int rc = download(c, ckpt_window_at(blob, nunits, 0), d_table, (size_t)nwin * kCkWinRec, s)) return fail(rc);
  }
  CkptView v;
  if (const char *why = ckpt_validate(blob, bytes, n, &v))
    return fail(set_error(ZT_E_INTERNAL, std::string("built checkpoint blob fails its validation: ") + why));
  *blob_out = blob;
  *blob_len = bytes;
  return ZT_OK;
}

}  // namespace

}  // namespace zt

using namespace zt;

extern "C" {

int zt_inflate_ckpt_build(const uint8_t *in, size_t n, size_t index, uint64_t span, uint8_t **idx, size_t *idx_len,
                          uint8_t **out, size_t *out_len, size_t *end_ip) {
  if (!idx || !idx_len || (out && !out_len)) return set_error(ZT_E_ARG, "null output");
  if (!in && n) return set_error(ZT_E_ARG, "null input");
  if (span == 0) span = ZT_CKPT_SPAN_DEFAULT;
  if (span < ZT_CKPT_SPAN_MIN) return set_error(ZT_E_ARG, "checkpoint span below 64 KiB");
  *idx = nullptr;
  *idx_len = 0;
  if (out) *out = nullptr;
  if (n > index) {
    DeviceCtx *c;
    ZT_TRY(get_ctx(&c));
    std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
    hipStream_t s = c->stream;
    void *d_in;
    ZT_TRY(scratch(c, kIn, n, &d_in));
    ZT_TRY(upload(c, d_in, in, n, s));
    std::vector<CkEntry> e;
    uint8_t *d_out = nullptr;
    size_t ol = 0, eip = 0;
    int rc;
    const bool small = n < index + (1u << 14);  // below the general path's minimum: one exact unit
    if (small) {
      const uint64_t bits = (uint64_t)(n - index) * 8;
      void *d_tok;
      GenJob *d_job = nullptr;
      GenResult *d_res = nullptr;
      ZT_TRY(scratch(c, kGenTokens, (bits + 256) * 4, &d_tok));
      ZT_TRY(scratch_carved(c, kGenMeta, [&](void *base) {
        Carve cv(base);
        d_job = cv.take<GenJob>(1);
        d_res = cv.take<GenResult>(1);
        return cv.bytes();
      }));
      GenJob j{};
      j.st.kind = GK_BLOCK;
      j.st.pos = (uint64_t)index * 8;
      j.stop = kCkNoStop;
      j.tok_cap = (uint32_t)bits;  // one token per bit: the format's maximum
      ZT_HIP(hipMemcpyAsync(d_job, &j, sizeof j, hipMemcpyHostToDevice, s));
      ZT_HIP(hipStreamSynchronize(s));
      ZT_TRY(gen_tokenize_exact_dev(static_cast<const uint8_t *>(d_in), n, d_job, d_res, static_cast<uint32_t *>(d_tok),
                                    1, s));
      GenResult r;
      ZT_TRY(readback(c, &r, d_res, sizeof r, s));
      rc = r.status == ZT_OK && r.end.kind == GK_FINAL ? 0 : 1;
      if (rc == 0) {
        e.assign(2, CkEntry{});
        e[0].pos = j.st.pos;
        e[0].kind = CK_BLOCK;
        e[0].ntok = r.ntok_stop;
        e[1].pos = r.end.pos;
        e[1].kind = CK_FINAL;
        e[1].out_off = r.out_stop;
        ol = (size_t)r.out_stop;
        eip = (size_t)((r.end.pos + 7) >> 3);
      }
    } else {
      rc = inflate_general_ckpt_dev(c, static_cast<const uint8_t *>(d_in), n, index, &d_out, &ol, &eip, &e, s);
    }
    if (rc < 0) return rc;
    if (rc == 0) {
      // the sentinel: the end state's bit, nothing else
      CkEntry &se = e.back();
      se.kind = CK_FINAL;
      se.hdr = 0;
      se.rem = se.flags = se.ntok = se.win = 0;
      const uint32_t nwin = ckpt_place_windows(e, span);
      uint8_t *blob = nullptr;
      size_t blob_len = 0;
      ZT_TRY(ckpt_finish(c, e, nwin, d_out, n, index, eip, ol, span, &blob, &blob_len, s));
      if (out) {
        uint8_t *h = nullptr;
        if (small) {
          // the one unit again through the range path: the blob's first use
          uint64_t o0 = 0, l0 = ol;
          int st = ZT_OK;
          size_t hl = 0;
          if (const int drc = ckpt_ranges_impl(in, n, blob, blob_len, &o0, &l0, 1, &h, &hl, &st)) {
            zt_free(blob);
            return drc;
          }
        } else {
          h = host_out(ol, true);
          if (!h) {
            zt_free(blob);
            return set_error(ZT_E_NOMEM, "host allocation failed");
          }
          if (const int drc = download(c, h, d_out, ol, s)) {
            zt_free(h);
            zt_free(blob);
            return drc;
          }
        }
        *out = h;
        *out_len = ol;
      } else if (out_len) {
        *out_len = ol;
      }
      if (end_ip) *end_ip = eip;
      *idx = blob;
      *idx_len = blob_len;
      g_ck.builds++;
      return ZT_OK;
    }
  }
  // the general path did not finish: a corrupt stream reports its own status
  // (the whole-stream call finds it), any other has no checkpoint index
  uint8_t *o = nullptr;
  size_t ol = 0, eip = 0;
  const int wrc = zt_inflate_raw(in, n, index, nullptr, &o, &ol, &eip);
  if (wrc != ZT_OK) return wrc;
  zt_free(o);
  return set_error(ZT_E_NO_INDEX, "the general decode does not finish this stream: no checkpoint index");
}

int zt_inflate_ckpt_ranges(const uint8_t *in, size_t n, const uint8_t *idx, size_t idx_len, const uint64_t *off,
                           const uint64_t *len, size_t count, uint8_t **out, size_t *out_len, int *status) {
  if (count == 0) return ZT_OK;
  if (!off || !len || !out || !out_len || !status) return set_error(ZT_E_ARG, "null argument");
  if ((!in && n) || !idx) return set_error(ZT_E_ARG, "null input");
  return ckpt_ranges_impl(in, n, idx, idx_len, off, len, count, out, out_len, status);
}

int zt_inflate_ckpt_range(const uint8_t *in, size_t n, const uint8_t *idx, size_t idx_len, uint64_t off, uint64_t len,
                          uint8_t **out, size_t *out_len) {
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if ((!in && n) || !idx) return set_error(ZT_E_ARG, "null input");
  int st = ZT_OK;
  return ckpt_ranges_impl(in, n, idx, idx_len, &off, &len, 1, out, out_len, &st);
}

int zt_ckpt_stats_read(zt_ckpt_stats *out, int reset) {
  if (!out) return set_error(ZT_E_ARG, "null output");
  out->builds = stat_take(g_ck.builds, reset);
  out->range_calls = stat_take(g_ck.range_calls, reset);
  out->ranges = stat_take(g_ck.ranges, reset);
  out->units_tokenized = stat_take(g_ck.units_tokenized, reset);
  out->in_bytes_uploaded = stat_take(g_ck.in_bytes_uploaded, reset);
  out->out_bytes_decoded = stat_take(g_ck.out_bytes_decoded, reset);
  out->out_bytes_returned = stat_take(g_ck.out_bytes_returned, reset);
  out->window_bytes_uploaded = stat_take(g_ck.window_bytes_uploaded, reset);
  return ZT_OK;
}

}  // extern "C"
