// dev_batch_api.cpp -- host side of the device-resident batch calls
// (include/zt_dev_batch.h): zt_deflate_dev_batch, zt_inflate_dev_batch and
// zt_deflate_dev_batch_bound.
//
// What the host batch calls do with pinned staging and PCIe copies happens on
// the device here.  Per group of items (dev_group_cuts: a call's scratch is
// bounded for any count): dev_copy_kernel (dev_batch.hip) gathers the caller's
// buffers into scratch slot kIn in the layout the pipelines read (pack_layout:
// the 32 KiB grid with zeroed cell tails for deflate, 256-byte offsets for
// inflate); the batch pipeline runs as in the host calls
// (deflate_batch_dev_run with checksums_batch_dev beside it on the second
// stream; the batch decoder of inflate_api.cpp, both routes, through its
// device sink); dev_copy_kernel scatters the results to the caller's pointers
// and dev_patch_kernel (member_frame.hip) writes prefixes, trailers and
// stored-block headers around them.  Items whose result does not fit are masked out on the host,
// where every length is known before the scatter is planned
// (dev_batch_plan.h: the arithmetic, checked by tools/dev_batch_host_check.cpp).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <list>
#include <vector>

#include "../../include/zt_dev_batch.h"
#include "zt_internal.h"

namespace zt {

namespace {

const char *const kCapMsg = "output capacity too small";  // (zt_inflate_dev's)

// The library's stream ordered against the caller's, in both directions.
struct StreamBridge {
  DeviceCtx *c;
  hipStream_t user;
  hipEvent_t ev = nullptr;
  StreamBridge(DeviceCtx *ctx, void *stream) : c(ctx), user(static_cast<hipStream_t>(stream)) {
    if (user == c->stream) user = nullptr;
  }
  ~StreamBridge() {
    if (ev) (void)hipEventDestroy(ev);
  }
  int enter() {  // the library's work waits for what the caller's stream holds
    if (!user) return ZT_OK;
    ZT_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    ZT_HIP(hipEventRecord(ev, user));
    ZT_HIP(hipStreamWaitEvent(c->stream, ev, 0));
    return ZT_OK;
  }
  int leave() {  // the caller's stream waits for the library's work
    if (!user || !ev) return ZT_OK;
    ZT_HIP(hipEventRecord(ev, c->stream));
    ZT_HIP(hipStreamWaitEvent(user, ev, 0));
    return ZT_OK;
  }
};

// The job tables of one launch pair: uploaded to scratch slot kDevBatch and
// run on s (copies, then patches).  The host vectors stay alive in `keep`
// until the call's next wait for the stream.
struct Launch {
  DevCopyPlan cp;
  std::vector<DevPatchJob> pj;
};
// zt_debug_dev_batch_times: HIP-event time of the gather (0) and scatter (1)
// launches, tables' upload excluded.  Measurement only: when on, every launch
// is waited for.
enum { kGather = 0, kScatter = 1 };
bool g_times_on = false;
double g_times_ms[2] = {0, 0};

int run_launch_untimed(DeviceCtx *c, std::list<Launch> &keep, Launch &&l, const uint32_t *d_sums, hipStream_t s,
                       hipEvent_t *ev);
int run_launch(DeviceCtx *c, std::list<Launch> &keep, Launch &&l, const uint32_t *d_sums, hipStream_t s, int kind) {
  if (!g_times_on) return run_launch_untimed(c, keep, std::move(l), d_sums, s, nullptr);
  hipEvent_t ev[2];
  ZT_HIP(hipEventCreate(&ev[0]));
  ZT_HIP(hipEventCreate(&ev[1]));
  int rc = run_launch_untimed(c, keep, std::move(l), d_sums, s, ev);
  float ms = 0;
  if (rc == 1) {  // (launched: both events recorded)
    rc = ZT_OK;
    if (hipEventSynchronize(ev[1]) == hipSuccess && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
      g_times_ms[kind] += ms;
  }
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  return rc;
}
// (ev non-null: the events around the kernels; then 1 = launched)
int run_launch_untimed(DeviceCtx *c, std::list<Launch> &keep, Launch &&l, const uint32_t *d_sums, hipStream_t s,
                       hipEvent_t *ev) {
  if (l.cp.jobs.empty() && l.pj.empty()) return ZT_OK;
  keep.push_back(std::move(l));
  const Launch &L = keep.back();
  DevCopyJob *d_cj = nullptr;
  DevPatchJob *d_pj = nullptr;
  ZT_TRY(scratch_carved(c, kDevBatch, [&](void *base) {
    Carve cv(base);
    d_cj = cv.take<DevCopyJob>(L.cp.jobs.size());
    d_pj = cv.take<DevPatchJob>(L.pj.size());
    return cv.bytes() + 256;
  }));
  if (!L.cp.jobs.empty())
    ZT_HIP(hipMemcpyAsync(d_cj, L.cp.jobs.data(), L.cp.jobs.size() * sizeof(DevCopyJob), hipMemcpyHostToDevice, s));
  if (!L.pj.empty())
    ZT_HIP(hipMemcpyAsync(d_pj, L.pj.data(), L.pj.size() * sizeof(DevPatchJob), hipMemcpyHostToDevice, s));
  if (ev) ZT_HIP(hipEventRecord(ev[0], s));
  ZT_TRY(dev_copy_dev(d_cj, (uint32_t)L.cp.jobs.size(), L.cp.tiles, s));
  ZT_TRY(dev_patch_dev(d_pj, (uint32_t)L.pj.size(), d_sums, s));
  if (ev) ZT_HIP(hipEventRecord(ev[1], s));
  return ev ? 1 : ZT_OK;
}

// tuning hook: ZT_DEV_BATCH_GROUP_BYTES = packed input bytes per group (read
// at every call; the results do not depend on it)
uint64_t group_bytes(uint64_t dflt = kDevGroupBytes) {
  const char *e = getenv("ZT_DEV_BATCH_GROUP_BYTES");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? (uint64_t)v : dflt;
}

int too_many_tiles() { return set_error(ZT_E_ARG, "batch too large for one launch"); }

// ---- deflate ------------------------------------------------------------------
// ct: the resolved compression type (0 for level 0)
int deflate_groups(DeviceCtx *c, const uint64_t *src, const size_t *n, size_t count, int ct, int lv,
                   const MemberFrame &fr, const uint64_t *dst, const size_t *out_cap, size_t *out_len, int *status) {
  hipStream_t s = c->stream;
  const bool sums = fr.kind != kFmtRaw;
  const uint32_t plen = fr.prefix_len(), tl = fr.trailer_len();
  uint8_t empty_trailer[8];  // CRC-32 0, ISIZE 0; Adler-32 1
  put_trailer(empty_trailer, fr.kind, 0, 1, 0);
  const std::vector<size_t> all = iota_ids(count);
  const std::vector<size_t> cut = dev_group_cuts(n, all, kDevBlk, group_bytes());
  std::list<Launch> keep;
  AuxWait aux_wait{c->aux};  // (the checksums read the gathered input: they never outlive the call)
  for (size_t g = 0; g + 1 < cut.size(); ++g) {
    // the group's items that go through the gather: the pipeline's, and with
    // a checksum in the trailer the stored ones too (the checksum kernels read
    // the packed copy)
    std::vector<size_t> pk;
    for (size_t i = cut[g]; i < cut[g + 1]; ++i)
      if (n[i] && (ct != 0 || sums)) pk.push_back(i);
    const size_t m = pk.size();
    std::vector<uint64_t> oo(m + 1, 0), len(m);
    void *d_in = nullptr, *d_body = nullptr, *d_sums = nullptr;
    if (m) {
      const PackLayout L = pack_layout(n, pk, kDevBlk, 1);
      for (size_t k = 0; k < m; ++k) len[k] = n[pk[k]];
      ZT_TRY(scratch(c, kIn, L.total + 64, &d_in));
      Launch ga;
      if (dev_gather_plan(src, n, pk, L, reinterpret_cast<uint64_t>(d_in), true, ga.cp)) return too_many_tiles();
      ZT_TRY(run_launch(c, keep, std::move(ga), nullptr, s, kGather));
      void *d_scr = nullptr;
      size_t ss = 0;
      if (sums) ZT_TRY(scratch(c, kSums, 8 * m, &d_sums));
      if (ct != 0) {
        ZT_TRY(scratch(c, kOut, batch_out_bound(L.total), &d_body));
        ss = deflate_batch_scratch_bytes(c, L.total);
        ZT_TRY(scratch(c, kDeflateOrDesc, ss, &d_scr));
      }
      ZT_TRY(deflate_members_dev(c, static_cast<const uint8_t *>(d_in), m, L.off.data(), len.data(), ct, lv,
                                 static_cast<uint8_t *>(d_body), oo.data(), d_scr, ss, nullptr,
                                 static_cast<uint32_t *>(d_sums), nullptr));
    }
    // the scatter: prefix | body | trailer of every item that fits
    Launch sc;
    size_t k = 0;  // the item's place in pk
    for (size_t i = cut[g]; i < cut[g + 1]; ++i) {
      const bool packed = n[i] && (ct != 0 || sums);
      const size_t kk = packed ? k++ : 0;
      const bool piped = n[i] && ct != 0;
      const uint64_t body = piped ? oo[kk + 1] - oo[kk] : stored_len(n[i]);
      const uint64_t need = plen + body + tl;
      out_len[i] = need;
      status[i] = ZT_OK;
      if (!dev_fits(need, out_cap, i)) {
        status[i] = ZT_E_ARG;
        continue;
      }
      if (!dst[i]) return set_error(ZT_E_ARG, "null output");
      dev_patch_bytes(sc.pj, dst[i], fr.prefix.data(), plen);
      if (piped) {
        if (!sc.cp.add(reinterpret_cast<uint64_t>(d_body) + oo[kk], dst[i] + plen, body)) return too_many_tiles();
      } else if (!dev_stored_jobs(src[i], n[i], dst[i] + plen, sc.cp, sc.pj)) {
        return too_many_tiles();
      }
      if (n[i])
        dev_patch_trailer(sc.pj, fr.kind, dst[i] + plen + body, n[i], (uint32_t)kk);
      else  // (no sums: the empty input goes through no gather)
        dev_patch_bytes(sc.pj, dst[i] + plen + body, empty_trailer, tl);
    }
    if (m && sums) ZT_TRY(join_sums(c));  // (the trailers need the checksums from the second stream)
    ZT_TRY(run_launch(c, keep, std::move(sc), static_cast<const uint32_t *>(d_sums), s, kScatter));
    // the next group reuses kIn, kOut and kSums; the last group's work stays
    // queued for the caller's stream
    if (g + 2 < cut.size()) {
      ZT_HIP(hipStreamSynchronize(s));
      keep.clear();
    }
  }
  ZT_HIP(hipStreamSynchronize(s));  // (the tables in `keep` are pageable host memory)
  for (size_t i = 0; i < count; ++i)
    if (status[i]) return set_error(ZT_E_ARG, kCapMsg);
  return ZT_OK;
}

// ---- inflate ------------------------------------------------------------------
int inflate_groups(DeviceCtx *c, const uint64_t *src, const size_t *n, const size_t *index, size_t count,
                   const uint64_t *dst, const size_t *out_cap, size_t *out_len, size_t *end_ip, int *status,
                   uint32_t *crc_out, uint32_t *adler_out) {
  hipStream_t s = c->stream;
  const bool want_sums = crc_out || adler_out;
  const std::vector<size_t> all = iota_ids(count);
  const std::vector<size_t> cut = dev_group_cuts(n, all, 256, group_bytes(kDevInflateGroupBytes));
  std::list<Launch> keep;
  size_t first_i = count;  // the first failing item, its code and detail
  int first_code = ZT_OK, first_detail = 0;
  for (size_t g = 0; g + 1 < cut.size(); ++g) {
    const size_t i0 = cut[g], m = cut[g + 1] - i0;
    std::vector<size_t> ids(m);
    for (size_t k = 0; k < m; ++k) ids[k] = i0 + k;
    const PackLayout L = pack_layout(n, ids, 256, 1);  // as the host call packs them
    void *d_in;
    ZT_TRY(scratch(c, kIn, L.total + 64, &d_in));
    Launch ga;
    if (dev_gather_plan(src, n, ids, L, reinterpret_cast<uint64_t>(d_in), false, ga.cp)) return too_many_tiles();
    ZT_TRY(run_launch(c, keep, std::move(ga), nullptr, s, kGather));
    std::vector<uint8_t> over(m, 0);
    DevSink sink;
    sink.put = [&](const uint8_t *d_base, const std::vector<SinkPiece> &pieces, hipStream_t ps) -> int {
      if (!dst) return ZT_OK;  // sizes only
      Launch sc;
      for (const SinkPiece &p : pieces) {
        const size_t i = i0 + p.item;
        if (!dev_fits(p.len, out_cap, i)) {
          over[p.item] = 1;
          continue;
        }
        if (p.len && !dst[i]) return set_error(ZT_E_ARG, "null output");
        if (!sc.cp.add(reinterpret_cast<uint64_t>(d_base) + p.off, dst[i], p.len)) return too_many_tiles();
      }
      return run_launch(c, keep, std::move(sc), nullptr, ps, kScatter);
    };
    std::vector<uint32_t> hsums(2 * m);
    for (size_t k = 0; k < m; ++k) {
      hsums[2 * k] = 0;
      hsums[2 * k + 1] = 1;
    }
    std::vector<int> detail(m, 0), st(m, ZT_OK);
    std::vector<uint8_t *> gout(m, nullptr);
    BatchExtras ex;
    ex.sums = want_sums ? hsums.data() : nullptr;
    ex.detail = detail.data();
    ex.sink = &sink;
    const int rc = inflate_batch_dev_streams_ex(c, d_in, L.off, n + i0, index ? index + i0 : nullptr, m, gout.data(),
                                                out_len + i0, end_ip ? end_ip + i0 : nullptr, st.data(), nullptr, 0,
                                                &ex);
    // (a code no item carries: the call itself failed)
    if (rc && std::find(st.begin(), st.end(), rc) == st.end()) return rc;
    for (size_t k = 0; k < m; ++k) {
      const size_t i = i0 + k;
      status[i] = st[k] ? st[k] : over[k] ? ZT_E_ARG : ZT_OK;
      if (crc_out) crc_out[i] = hsums[2 * k];
      if (adler_out) adler_out[i] = hsums[2 * k + 1];
      if (status[i] && first_i == count) {
        first_i = i;
        first_code = status[i];
        first_detail = st[k] ? detail[k] : -1;
      }
    }
    ZT_HIP(hipStreamSynchronize(s));
    keep.clear();
  }
  if (first_i == count) return ZT_OK;
  if (first_detail == -1 && first_code == ZT_E_ARG) return set_error(ZT_E_ARG, kCapMsg);
  return inflate_error(first_code, first_detail);
}

int check_ptrs(const void *const *d_in, const size_t *n, size_t count, uint64_t *src) {
  for (size_t i = 0; i < count; ++i) {
    if (n[i] && !d_in[i]) return set_error(ZT_E_ARG, "null input");
    src[i] = reinterpret_cast<uint64_t>(d_in[i]);
  }
  return ZT_OK;
}

}  // namespace

}  // namespace zt

using namespace zt;

extern "C" {

// debug (exported, not part of include/zt_dev_batch.h; tools/dev_batch_time.py):
// the HIP-event time of the gather (out[0]) and scatter (out[1]) launches since
// the last call, in ms, then cleared; enable != 0 turns the timing on for the
// calls that follow (every launch is then waited for), 0 turns it off
int zt_debug_dev_batch_times(int enable, double out[2]) {
  if (out) {
    out[0] = g_times_ms[0];
    out[1] = g_times_ms[1];
  }
  g_times_ms[0] = g_times_ms[1] = 0;
  g_times_on = enable != 0;
  return ZT_OK;
}

size_t zt_deflate_dev_batch_bound(size_t n, int compression_type, int format) {
  if (compression_type < 0 || compression_type > 2 || format < kFmtRaw || format > kFmtGzip) return 0;
  return (size_t)dev_batch_bound(n, compression_type, (MemberKind)format);
}

int zt_deflate_dev_batch(const void *const *d_in, const size_t *n, size_t count, const zt_deflate_opts *opts,
                         int format, void *const *d_out, const size_t *out_cap, size_t *out_len, int *status,
                         void *stream) {
  if (count == 0) return ZT_OK;
  if (!d_in || !n || !d_out || !out_cap || !out_len || !status) return set_error(ZT_E_ARG, "null argument");
  if (format < kFmtRaw || format > kFmtGzip) return set_error(ZT_E_ARG, "unknown format");
  int ct, lv;
  ZT_TRY(resolve_opts(opts, &ct, &lv));
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  std::vector<uint64_t> src(count), dst(count);
  ZT_TRY(check_ptrs(d_in, n, count, src.data()));
  for (size_t i = 0; i < count; ++i) {
    dst[i] = reinterpret_cast<uint64_t>(d_out[i]);
    out_len[i] = 0;
    status[i] = ZT_OK;
  }
  StreamBridge br(c, stream);
  ZT_TRY(br.enter());
  // (zlib's FLEVEL: the compression type as given, as zt_zlib_compress_batch writes it)
  const int rc = deflate_groups(c, src.data(), n, count, ct, lv,
                                frame_of((MemberKind)format, opts ? opts->compression_type : 2), dst.data(), out_cap,
                                out_len, status);
  const std::string msg = rc ? zt_last_error_message() : "";
  if (const int lrc = br.leave()) return rc ? set_error(rc, msg) : lrc;
  return rc ? set_error(rc, msg) : ZT_OK;
}

int zt_inflate_dev_batch(const void *const *d_in, const size_t *n, const size_t *index, size_t count,
                         void *const *d_out, const size_t *out_cap, size_t *out_len, size_t *end_ip, int *status,
                         uint32_t *crc_out, uint32_t *adler_out, void *stream) {
  if (count == 0) return ZT_OK;
  if (!d_in || !n || !out_len || !status || (d_out && !out_cap)) return set_error(ZT_E_ARG, "null argument");
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  std::vector<uint64_t> src(count), dst(d_out ? count : 0);
  ZT_TRY(check_ptrs(d_in, n, count, src.data()));
  for (size_t i = 0; i < count; ++i) {
    if (d_out) dst[i] = reinterpret_cast<uint64_t>(d_out[i]);
    out_len[i] = 0;
    status[i] = ZT_OK;
  }
  StreamBridge br(c, stream);
  ZT_TRY(br.enter());
  const int rc = inflate_groups(c, src.data(), n, index, count, d_out ? dst.data() : nullptr, out_cap, out_len,
                                end_ip, status, crc_out, adler_out);
  const std::string msg = rc ? zt_last_error_message() : "";
  if (const int lrc = br.leave()) return rc ? set_error(rc, msg) : lrc;
  return rc ? set_error(rc, msg) : ZT_OK;
}

}  // extern "C"
