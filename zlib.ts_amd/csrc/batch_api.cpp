// batch_api.cpp -- many independent buffers per call (configs C4 and C2's
// producer side; include/zt.h): zt_gzip_compress_batch, zt_zlib_compress_batch
// and zt_deflate_raw_batch.
//
// Per device, one pipeline for the whole share: the buffers are packed into
// pinned staging at 32 KiB boundaries and uploaded with one copy; the batch
// deflate pipeline (deflate.hip's deflate_batch_dev_run: the match kernel, then
// deflate_post.hip's stages; one match workgroup per block so no history
// crosses buffers) runs on the main stream while the batched CRC-32 /
// Adler-32 kernels read the same device bytes on the second stream; one copy
// brings every stream back.  With zt_set_devices(mask) the buffers are split
// over the devices by longest-processing-time (largest first onto the least
// loaded device) and each device's share runs on its own host thread.
// Replaces a loop of new GZip(input).compress() (src/GZip.ts:96-194),
// new Deflate(input).compress() (src/Deflate.ts:60-99) and
// new RawDeflate(input).compress() (src/RawDeflate.ts:87-114).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "zt_internal.h"

namespace zt {

namespace {

constexpr uint64_t kBlk = 32768;

// ZT_BATCH_STAGES=1: host-only stage timers of one device's share (JSON line
// on stderr per share) -- packing into pinned staging and framing the members
// are the host work that has to keep up with k devices on a node
// (tools/c4_host_stages.py).  Measurement only.
bool stages_on() {
  static const bool on = getenv("ZT_BATCH_STAGES") != nullptr;
  return on;
}
struct StageTimes {
  double pack_ms = 0, frame_ms = 0, wall_ms = 0;
  uint64_t in_bytes = 0, out_bytes = 0;
  size_t items = 0, groups = 0;
  void report(int dev) const {
    if (!stages_on()) return;
    fprintf(stderr,
            "{\"zt_batch_stages\": 1, \"device\": %d, \"items\": %zu, \"groups\": %zu, \"in_bytes\": %llu, "
            "\"out_bytes\": %llu, \"pack_ms\": %.3f, \"frame_ms\": %.3f, \"wall_ms\": %.3f}\n",
            dev, items, groups, (unsigned long long)in_bytes, (unsigned long long)out_bytes, pack_ms, frame_ms,
            wall_ms);
  }
};

// fills out[i] (malloc'd: prefix | stream | trailer) for item i
// (dst: the item's place in a batch slab, or null for its own allocation)
int frame_item(const MemberFrame &fr, size_t n_in, const uint8_t *body, size_t blen, uint32_t crc, uint32_t adler,
               uint8_t **out, size_t *out_len, uint8_t *dst = nullptr) {
  const size_t total = fr.prefix.size() + blen + fr.trailer_len();
  uint8_t *h = dst ? dst : host_out(total);
  if (!h) return set_error(ZT_E_NOMEM, "host allocation failed");
  if (!fr.prefix.empty()) memcpy(h, fr.prefix.data(), fr.prefix.size());
  if (blen) memcpy(h + fr.prefix.size(), body, blen);
  put_trailer(h + fr.prefix.size() + blen, fr.kind, crc, adler, (uint32_t)n_in);
  *out = h;
  *out_len = total;
  return ZT_OK;
}

// items [k0, k0 + nb) framed into one slab (slab_out): their offsets, and
// the slab (null when it cannot be allocated)
uint8_t *frame_slab(const MemberFrame &fr, const uint64_t *oo, size_t nb, std::vector<size_t> &soff) {
  soff.resize(nb);
  size_t tot = 0;
  for (size_t j = 0; j < nb; ++j) {
    soff[j] = tot;
    tot += slab_stride(fr.prefix.size(), oo[j + 1] - oo[j], fr.trailer_len());
  }
  return slab_out(tot, nb);
}

// Large shares (>= kGroupMin padded bytes): the items are cut, in order, into
// groups of about 1/6 of the share (>= 128 MiB) and run as a three-stage
// pipeline, so PCIe and the host work overlap the GPU: group g + 1 is packed
// into pinned staging and uploaded (stream c->up, one host thread) while
// group g is checksummed (c->aux) and deflated (c->stream, the caller's
// thread) and group g - 1 comes back and is framed into the members (stream
// c->dn, one host thread).  Groups are independent batch pipelines (no item
// spans two), so every member is the one the single pipeline writes.
constexpr uint64_t kGroupMin = 256ull << 20;

int batch_grouped(DeviceCtx *c, const uint8_t *const *in, const size_t *n, const std::vector<size_t> &work,
                  const PackLayout &L, const std::vector<uint64_t> &len, int ct, int lv, const MemberFrame &fr,
                  uint8_t **out, size_t *out_len, StageTimes &tm, const DictHist *dh) {
  const size_t m = work.size();
  const std::vector<size_t> &off = L.off;
  const uint64_t padded = L.total;
  const bool sums = fr.kind != kFmtRaw;
  // groups [gk[g], gk[g + 1]) of items
  // tuning hook: ZT_BATCH_GROUPS = groups per share (default 6)
  static const int ng_env = getenv("ZT_BATCH_GROUPS") ? atoi(getenv("ZT_BATCH_GROUPS")) : 0;
  const uint64_t target = std::max<uint64_t>(padded / (ng_env > 0 ? ng_env : 6), 64ull << 20);
  const std::vector<size_t> gk = group_cuts(off, m, padded, target);
  const size_t ng = gk.size() - 1;
  auto gbeg = [&](size_t g) { return off[gk[g]]; };
  auto gend = [&](size_t g) { return gk[g + 1] < m ? off[gk[g + 1]] : padded; };
  uint64_t gmax = 0, obmax = 0;
  std::vector<uint64_t> ooff(ng + 1, 0);  // device output region of group g
  for (size_t g = 0; g < ng; ++g) {
    const uint64_t ob = batch_out_bound(gend(g) - gbeg(g), 256);
    gmax = std::max(gmax, gend(g) - gbeg(g));
    obmax = std::max(obmax, ob);
    ooff[g + 1] = ooff[g] + ob;
  }
  void *d_in, *d_out, *d_scr, *d_sums = nullptr, *p;
  ZT_TRY(scratch(c, kIn, padded + 64, &d_in));
  ZT_TRY(scratch(c, kOut, ooff[ng], &d_out));
  const size_t ss = deflate_batch_scratch_bytes(c, gmax);
  ZT_TRY(scratch(c, kDeflateOrDesc, ss, &d_scr));
  if (sums) ZT_TRY(scratch(c, kSums, 8 * m, &d_sums));
  uint8_t *stage_in[2], *stage_out;
  ZT_TRY(pinned(c, gmax, &p, kPinBatch));
  stage_in[0] = static_cast<uint8_t *>(p);
  ZT_TRY(pinned(c, gmax, &p, kPinGroupIn));
  stage_in[1] = static_cast<uint8_t *>(p);
  ZT_TRY(pinned(c, obmax, &p, kPinGroupOut));
  stage_out = static_cast<uint8_t *>(p);
  struct Staged {  // stage_in[k]'s last upload has left it
    hipEvent_t ev[2] = {};
    ~Staged() {
      for (auto e : ev)
        if (e) (void)hipEventDestroy(e);
    }
  } staged;
  for (auto &e : staged.ev) ZT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));

  std::vector<uint32_t> hsums(2 * m, 0);
  std::vector<uint64_t> oo(m + ng, 0);  // group g's stream offsets at oo[gk[g] + g ..]
  StagePipe pipe(c, ng);
  auto up_stage = [&](size_t g) -> int {
    uint8_t *st = stage_in[g & 1];
    if (g >= 2) ZT_HIP(hipEventSynchronize(staged.ev[g & 1]));  // its previous upload has left
    const double t0 = now_ms();
    pack_items(st, in, n, work, L, gk[g], gk[g + 1], true, gend(g) - gbeg(g));
    tm.pack_ms += now_ms() - t0;  // (this thread only)
    ZT_HIP(hipMemcpyAsync((uint8_t *)d_in + gbeg(g), st, gend(g) - gbeg(g), hipMemcpyHostToDevice, c->up));
    ZT_HIP(hipEventRecord(staged.ev[g & 1], c->up));
    return ZT_OK;
  };
  auto compute = [&](size_t g) -> int {
    const size_t k0 = gk[g], nb = gk[g + 1] - k0;
    const uint64_t b = gbeg(g);
    std::vector<uint64_t> ro(nb), rl(len.begin() + k0, len.begin() + k0 + nb);
    for (size_t j = 0; j < nb; ++j) ro[j] = off[k0 + j] - b;
    uint32_t *gsums = sums ? (uint32_t *)d_sums + 2 * k0 : nullptr;
    ZT_TRY(deflate_members_dev(c, (const uint8_t *)d_in + b, nb, ro.data(), rl.data(), ct, lv,
                               (uint8_t *)d_out + ooff[g], &oo[k0 + g], d_scr, ss, dh, gsums, pipe.landed(g)));
    if (sums) {
      ZT_HIP(hipMemcpyAsync(hsums.data() + 2 * k0, gsums, 8 * nb, hipMemcpyDeviceToHost, c->aux));
      ZT_HIP(hipStreamSynchronize(c->aux));
    }
    return ZT_OK;
  };
  auto dn_stage = [&](size_t g) -> int {
    const size_t k0 = gk[g], nb = gk[g + 1] - k0;
    const uint64_t *go = &oo[k0 + g];
    ZT_HIP(hipMemcpyAsync(stage_out, (uint8_t *)d_out + ooff[g], go[nb], hipMemcpyDeviceToHost, c->dn));
    ZT_HIP(hipStreamSynchronize(c->dn));
    std::vector<int> rcs(nb, ZT_OK);
    std::vector<size_t> soff;
    const double t0 = now_ms();
    uint8_t *slab = frame_slab(fr, go, nb, soff);
    if (!slab) return set_error(ZT_E_NOMEM, "host allocation failed");
    parallel_copy(nb, [&](size_t j) {
      const size_t k = k0 + j, i = work[k];
      rcs[j] = frame_item(fr, len[k], stage_out + go[j], go[j + 1] - go[j], hsums[2 * k], hsums[2 * k + 1], &out[i],
                          &out_len[i], slab + soff[j]);
    }, go[nb]);
    tm.frame_ms += now_ms() - t0;  // (this thread only)
    tm.out_bytes += go[nb];
    for (int rc : rcs)
      if (rc) return rc;
    return ZT_OK;
  };
  tm.groups = ng;
  return pipe.run(up_stage, compute, dn_stage);
}

// one device's share: items `ids` of the batch (for_each_device: c is locked)
int batch_on_device(DeviceCtx *c, const uint8_t *const *in, const size_t *n, const std::vector<size_t> &ids, int ct,
                    int lv, const MemberFrame &fr, uint8_t **out, size_t *out_len, const HostDict &hd) {
  const bool sums = fr.kind != kFmtRaw;
  // empty inputs: a final empty stored block, as the one-buffer calls write
  // (deflate.hip) -- no device work
  std::vector<size_t> work;
  for (size_t i : ids) {
    if (n[i] == 0) {
      uint8_t empty_stored[5];
      stored_write(nullptr, 0, empty_stored);
      ZT_TRY(frame_item(fr, 0, empty_stored, sizeof empty_stored, 0, 1, &out[i], &out_len[i]));
    } else {
      work.push_back(i);
    }
  }
  if (work.empty()) return ZT_OK;
  // preset dictionary: one copy per device of the history the match kernel
  // loads in front of every stream (dict_host.h: padding | usable tail)
  DictHist dict_dev{nullptr, 0, 0};
  const DictHist *dh = nullptr;
  std::vector<uint8_t> dict_img;
  if (hd.dict_len && ct != 0) {
    const DictLayout D = dict_layout(hd.dict_len);
    void *d_dict;
    ZT_TRY(scratch(c, kDict, D.hist, &d_dict));
    dict_img.resize(D.hist);
    dict_fill_history(D, hd.dict, dict_img.data());
    ZT_HIP(hipMemcpyAsync(d_dict, dict_img.data(), D.hist, hipMemcpyHostToDevice, c->stream));
    ZT_HIP(hipStreamSynchronize(c->stream));
    dict_dev = DictHist{static_cast<const uint8_t *>(d_dict), D.hist, D.floor};
    dh = &dict_dev;
  }
  const size_t m = work.size();
  const PackLayout L = pack_layout(n, work, kBlk, 1);  // every item from a 32 KiB boundary
  const std::vector<size_t> &off = L.off;
  const uint64_t padded = L.total;
  std::vector<uint64_t> len(m);
  uint64_t in_bytes = 0;
  for (size_t k = 0; k < m; ++k) in_bytes += len[k] = n[work[k]];
  StageTimes tm;
  tm.items = m;
  tm.in_bytes = in_bytes;
  const double t_start = now_ms();
  struct Report {
    StageTimes &tm;
    double t0;
    int dev;
    ~Report() {
      tm.wall_ms = now_ms() - t0;
      tm.report(dev);
    }
  } report{tm, t_start, c->device};
  if (ct != 0 && padded >= kGroupMin && m >= 2)
    return batch_grouped(c, in, n, work, L, len, ct, lv, fr, out, out_len, tm, dh);
  void *d_in;
  ZT_TRY(pack_upload(c, in, n, work, L, PackMode{true, false, in_bytes, &tm.pack_ms}, &d_in));
  tm.groups = 1;
  // checksums on the second stream, over the same device bytes
  std::vector<uint32_t> hsums(2 * m, 0);
  void *d_sums = nullptr, *d_out = nullptr, *d_scr = nullptr;
  size_t ss = 0;
  AuxWait aux_wait{c->aux};
  if (sums) ZT_TRY(scratch(c, kSums, 8 * m, &d_sums));
  if (ct != 0) {
    ZT_TRY(scratch(c, kOut, batch_out_bound(padded), &d_out));
    ss = deflate_batch_scratch_bytes(c, padded);
    ZT_TRY(scratch(c, kDeflateOrDesc, ss, &d_scr));
  }
  std::vector<uint64_t> oo(m + 1, 0);
  ZT_TRY(deflate_members_dev(c, (const uint8_t *)d_in, m, off.data(), len.data(), ct, lv, (uint8_t *)d_out, oo.data(),
                             d_scr, ss, dh, (uint32_t *)d_sums, nullptr));
  if (sums) ZT_HIP(hipMemcpyAsync(hsums.data(), d_sums, 8 * m, hipMemcpyDeviceToHost, c->aux));
  uint8_t *body_host = nullptr;
  std::vector<uint8_t> stored_host;
  if (ct == 0) {
    // stored blocks of <= 65535 bytes (src/RawDeflate.ts:93-100,122-153): framing only
    uint64_t tot = 0;
    for (size_t k = 0; k < m; ++k) {
      oo[k] = tot;
      tot += stored_len(len[k]);
    }
    oo[m] = tot;
    stored_host.resize(tot);
    for (size_t k = 0; k < m; ++k) stored_write(in[work[k]], len[k], stored_host.data() + oo[k]);
    body_host = stored_host.data();
  } else {
    // The members are framed on the device (prefix | stream | trailer, at
    // their slab offsets) and come back with one copy -- straight into the
    // slab when it is a registered pool buffer (a caller batching again after
    // freeing the last outputs): the host only lays the slab out.  Host
    // framing (the slab filled from a staged copy of the streams) was a
    // quarter of a device thread's host time on a node's worth of devices
    // (tools/c4_host_stages.py).
    const double t_frame = now_ms();
    const uint32_t plen = fr.prefix_len(), tl = fr.trailer_len();
    std::vector<FrameItem> fi(m);
    std::vector<size_t> soff(m);
    size_t tot = 0;
    for (size_t k = 0; k < m; ++k) {
      soff[k] = tot;
      fi[k] = FrameItem{oo[k], tot, (uint32_t)(oo[k + 1] - oo[k]), (uint32_t)len[k]};
      tot += slab_stride(plen, oo[k + 1] - oo[k], tl);
    }
    const size_t fr_bytes = (tot + 255) & ~size_t(255), it_bytes = (m * sizeof(FrameItem) + 255) & ~size_t(255);
    void *d_fr;
    ZT_TRY(scratch(c, kFramed, fr_bytes + it_bytes + plen + 256, &d_fr));
    uint8_t *d_framed = static_cast<uint8_t *>(d_fr);
    FrameItem *d_items = reinterpret_cast<FrameItem *>(d_framed + fr_bytes);
    uint8_t *d_prefix = d_framed + fr_bytes + it_bytes;
    ZT_HIP(hipMemcpyAsync(d_items, fi.data(), m * sizeof(FrameItem), hipMemcpyHostToDevice, c->stream));
    if (plen) ZT_HIP(hipMemcpyAsync(d_prefix, fr.prefix.data(), plen, hipMemcpyHostToDevice, c->stream));
    if (sums) ZT_TRY(join_sums(c));  // (the trailers need the checksums from the second stream)
    ZT_TRY(frame_members_dev(d_items, (uint32_t)m, d_prefix, plen, fr.kind, static_cast<const uint8_t *>(d_out),
                             static_cast<const uint32_t *>(d_sums), d_framed, c->stream));
    uint8_t *slab = slab_out(tot, m, true);
    if (!slab) return set_error(ZT_E_NOMEM, "host allocation failed");
    const bool direct = host_direct(slab, tot);
    tm.frame_ms += now_ms() - t_frame;
    if (direct) {  // (DMA time, not host work: like the upload, outside the stage timers)
      ZT_HIP(hipMemcpyAsync(slab, d_framed, tot, hipMemcpyDeviceToHost, c->stream));
      ZT_HIP(hipStreamSynchronize(c->stream));
    } else {
      const double t_dl = now_ms();
      ZT_TRY(download(c, slab, d_framed, tot, c->stream));
      tm.frame_ms += now_ms() - t_dl;  // (staged: host copies)
    }
    ZT_HIP(hipStreamSynchronize(c->aux));
    for (size_t k = 0; k < m; ++k) {
      out[work[k]] = slab + soff[k];
      out_len[work[k]] = plen + (oo[k + 1] - oo[k]) + tl;
    }
    tm.out_bytes += oo[m];
    return ZT_OK;
  }
  ZT_HIP(hipStreamSynchronize(c->aux));
  std::vector<int> rcs(m, ZT_OK);
  std::vector<size_t> soff;
  const double t_frame = now_ms();
  uint8_t *slab = frame_slab(fr, oo.data(), m, soff);
  if (!slab) return set_error(ZT_E_NOMEM, "host allocation failed");
  parallel_copy(m, [&](size_t k) {
    const size_t i = work[k];
    rcs[k] = frame_item(fr, len[k], body_host + oo[k], oo[k + 1] - oo[k], hsums[2 * k], hsums[2 * k + 1], &out[i],
                        &out_len[i], slab + soff[k]);
  }, oo[m]);
  tm.frame_ms += now_ms() - t_frame;
  tm.out_bytes += oo[m];
  for (int rc : rcs)
    if (rc) return rc;
  return ZT_OK;
}

// split over the batch devices (LPT); a failed share fails the call: every
// output is released and the first code and message are the caller's
int run_batch(const uint8_t *const *in, const size_t *n, size_t count, int ct, int lv, const MemberFrame &fr,
              uint8_t **out, size_t *out_len, int *status, const HostDict &hd = HostDict()) {
  for (size_t i = 0; i < count; ++i) {
    out[i] = nullptr;
    out_len[i] = 0;
    if (n[i] && !in[i]) return set_error(ZT_E_ARG, "null input");
  }
  const std::vector<int> devs = fanout_devices(count);
  const std::vector<std::vector<size_t>> share = lpt_shares(n, count, devs.size());
  const std::vector<ShareResult> res =
      for_each_device(devs, share, [&](size_t, DeviceCtx *c, const std::vector<size_t> &ids) {
        return batch_on_device(c, in, n, ids, ct, lv, fr, out, out_len, hd);
      });
  int first = ZT_OK;
  for (size_t d = 0; d < share.size(); ++d) {
    for (size_t i : share[d]) status[i] = res[d].code;
    if (res[d].code && first == ZT_OK) first = set_error(res[d].code, res[d].msg);
  }
  if (first) {
    for (size_t i = 0; i < count; ++i) {
      zt_free(out[i]);
      out[i] = nullptr;
      out_len[i] = 0;
    }
  }
  return first;
}

}  // namespace

// zt_dict.h's batch deflate calls (dict_api.cpp): raw streams, or zlib members
// whose header carries FDICT and the dictionary's Adler-32 (frame_zlib_dict)
int deflate_batch_host(const uint8_t *const *in, const size_t *n, size_t count, const zt_deflate_opts *opts,
                       const HostDict &hd, const MemberFrame &fr, uint8_t **out, size_t *out_len, int *status) {
  int ct, lv;
  ZT_TRY(resolve_opts(opts, &ct, &lv));
  return run_batch(in, n, count, ct, lv, fr, out, out_len, status, hd);
}

}  // namespace zt

using namespace zt;

extern "C" {

int zt_deflate_raw_batch(const uint8_t *const *in, const size_t *n, size_t count, const zt_deflate_opts *opts,
                         uint8_t **out, size_t *out_len, int *status) {
  if (count == 0) return ZT_OK;
  if (!in || !n || !out || !out_len || !status) return set_error(ZT_E_ARG, "null argument");
  int ct, lv;
  ZT_TRY(resolve_opts(opts, &ct, &lv));
  return run_batch(in, n, count, ct, lv, frame_raw(), out, out_len, status);
}

int zt_gzip_compress_batch(const uint8_t *const *in, const size_t *n, size_t count, const zt_gzip_opts *opts,
                           uint8_t **out, size_t *out_len, int *status) {
  if (count == 0) return ZT_OK;
  if (!in || !n || !out || !out_len || !status) return set_error(ZT_E_ARG, "null argument");
  int ct, lv;
  ZT_TRY(resolve_opts(opts ? &opts->deflate : nullptr, &ct, &lv));
  return run_batch(in, n, count, ct, lv, frame_gzip(opts), out, out_len, status);
}

int zt_crc32_batch(const uint8_t *const *in, const size_t *n, size_t count, uint32_t *crc_out) {
  if (count == 0) return ZT_OK;
  if (!in || !n || !crc_out) return set_error(ZT_E_ARG, "null argument");
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  for (size_t i = 0; i < count; ++i)
    if (n[i] && !in[i]) return set_error(ZT_E_ARG, "null input");
  const std::vector<size_t> ids = iota_ids(count);
  const PackLayout L = pack_layout(n, ids, 256, 0);
  void *d_in, *d_sums;
  ZT_TRY(pack_upload(c, in, n, ids, L, PackMode{false, false}, &d_in));
  ZT_TRY(scratch(c, kSums, 8 * count, &d_sums));
  ZT_TRY(checksums_batch_dev(c, (const uint8_t *)d_in, count, L.off.data(), n, (uint32_t *)d_sums, c->stream));
  std::vector<uint32_t> sums(2 * count);
  ZT_HIP(hipMemcpyAsync(sums.data(), d_sums, 8 * count, hipMemcpyDeviceToHost, c->stream));
  ZT_HIP(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < count; ++i) crc_out[i] = sums[2 * i];
  return ZT_OK;
}

int zt_zlib_compress_batch(const uint8_t *const *in, const size_t *n, size_t count, const zt_deflate_opts *opts,
                           uint8_t **out, size_t *out_len, int *status) {
  if (count == 0) return ZT_OK;
  if (!in || !n || !out || !out_len || !status) return set_error(ZT_E_ARG, "null argument");
  int ct, lv;
  ZT_TRY(resolve_opts(opts, &ct, &lv));
  return run_batch(in, n, count, ct, lv, frame_zlib(opts ? opts->compression_type : 2), out, out_len, status);
}

}  // extern "C"
