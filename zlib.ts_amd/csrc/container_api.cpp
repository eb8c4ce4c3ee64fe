// container_api.cpp -- GZip (RFC 1952) and zlib (RFC 1950) containers over the
// raw DEFLATE engine (include/zt.h).
//
// Headers and trailers are a few bytes of host logic; the hot path stays on
// the GPU: GZip compress uploads the input once and runs the deflate pipeline
// and the CRC-32 kernel on the same device-resident bytes (the reference
// deflates and then walks the input a second time for the CRC,
// src/GZip.ts:164-180); zlib compress does the same with Adler-32.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/zt_index.h"
#include "gunzip_chain.h"
#include "zt_internal.h"

namespace zt {

namespace {

// Raw DEFLATE of host bytes into `out` after `prefix` bytes of header, with the
// input's CRC-32 and/or Adler-32 from the same device copy of the input.
// *out (malloc'd) = prefix | stream | `trailer` bytes of room.  With idx
// non-null (the _indexed calls) the stream's deflate-time index comes back
// too, its positions counted in *out: stream_start = prefix_len.
int deflate_with_checksums(const uint8_t *in, size_t n, const zt_deflate_opts *opts, const uint8_t *prefix,
                           size_t prefix_len, size_t trailer, uint8_t **out, size_t *stream_len, uint32_t *crc,
                           uint32_t *adler, uint8_t **idx = nullptr, size_t *idx_len = nullptr) {
  int ct, lv;
  if (idx) {  // (before any device work)
    ZT_TRY(resolve_opts(opts, &ct, &lv));
    ZT_TRY(deflate_index_refuse(ct, n));
  }
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  ZT_TRY(resolve_opts(opts, &ct, &lv));
  DeflateIndexTable tab;
  DeflateIndexReq req{};
  if (idx) {
    ZT_TRY(deflate_index_begin(c, std::vector<size_t>{n}, prefix_len, &tab));
    req = deflate_index_piece(tab, 0, 0, 0);
  }
  const size_t ob = deflate_out_bound(ct, n);
  void *d_in, *d_out, *d_scr, *d_res;
  ZT_TRY(scratch(c, kIn, n + 64, &d_in));
  ZT_TRY(scratch(c, kOut, ob, &d_out));
  const size_t ss = deflate_scratch_bytes(c, n);
  ZT_TRY(scratch(c, kDeflateOrDesc, ss, &d_scr));
  ZT_TRY(scratch(c, kSmall, 16, &d_res));
  ZT_TRY(upload(c, d_in, in, n, c->stream));
  // the checksums run on the second stream beside the deflate pipeline (both
  // only read the input); every return below waits for that stream first
  uint32_t sums[2] = {0, 1};  // CRC-32 and Adler-32 of nothing
  AuxWait aux_wait{c->aux};
  if (n) {
    ZT_HIP(hipEventRecord(c->aux_ev, c->stream));
    ZT_HIP(hipStreamWaitEvent(c->aux, c->aux_ev, 0));
    ZT_TRY(checksums_dev(c, (const uint8_t *)d_in, n, crc != nullptr, adler != nullptr, 0, 1, (uint32_t *)d_res,
                         c->aux));
    ZT_HIP(hipMemcpyAsync(sums, d_res, sizeof sums, hipMemcpyDeviceToHost, c->aux));
  }
  size_t len = 0;
  ZT_TRY(deflate_dev_run(c, (const uint8_t *)d_in, n, 0, 1, ct, lv, (uint8_t *)d_out, &len, d_scr, ss, c->stream,
                         idx ? &req : nullptr));
  uint8_t *h = host_out(prefix_len + len + trailer + 1);
  if (!h) return set_error(ZT_E_NOMEM, "host allocation failed");
  if (prefix_len) memcpy(h, prefix, prefix_len);
  int drc = download(c, h + prefix_len, d_out, len, c->stream);
  if (!drc && idx) drc = deflate_index_finish(c, tab, len, n, idx, idx_len, c->stream);
  if (drc) {
    zt_free(h);
    return drc;
  }
  hipError_t e = hipStreamSynchronize(c->aux);
  if (e != hipSuccess) {
    zt_free(h);
    if (idx && *idx) {
      zt_free(*idx);
      *idx = nullptr;
    }
    return hip_fail(e, "hipStreamSynchronize");
  }
  if (crc) *crc = sums[0];
  if (adler) *adler = sums[1];
  *out = h;
  *stream_len = len;
  return ZT_OK;
}

// One member from one host buffer: zt_gzip_compress and zt_zlib_compress, and
// with idx non-null their _indexed forms.  *sum_out: the trailer's checksum.
int compress_member_host(const MemberFrame &fr, const uint8_t *in, size_t n, const zt_deflate_opts *opts,
                         uint8_t **out, size_t *out_len, uint32_t *sum_out, uint8_t **idx, size_t *idx_len) {
  uint8_t *buf;
  size_t slen;
  uint32_t crc = 0, adler = 1;
  const bool gz = fr.kind == kFmtGzip;
  ZT_TRY(deflate_with_checksums(in, n, opts, fr.prefix.data(), fr.prefix.size(), fr.trailer_len(), &buf, &slen,
                                gz ? &crc : nullptr, gz ? nullptr : &adler, idx, idx_len));
  put_trailer(buf + fr.prefix.size() + slen, fr.kind, crc, adler, (uint32_t)n);
  *out = buf;
  *out_len = fr.prefix.size() + slen + fr.trailer_len();
  if (sum_out) *sum_out = gz ? crc : adler;
  return ZT_OK;
}

}  // namespace
}  // namespace zt

using namespace zt;

extern "C" {

// zt_gzip_compress, and with idx non-null zt_gzip_compress_indexed
static int gzip_compress_host(const uint8_t *in, size_t n, const zt_gzip_opts *opts, uint8_t **out, size_t *out_len,
                              uint32_t *crc_out, uint8_t **idx, size_t *idx_len) {
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if (n && !in) return set_error(ZT_E_ARG, "null input");
  return compress_member_host(frame_gzip(opts), in, n, opts ? &opts->deflate : nullptr, out, out_len, crc_out, idx,
                              idx_len);
}

int zt_gzip_compress(const uint8_t *in, size_t n, const zt_gzip_opts *opts, uint8_t **out, size_t *out_len,
                     uint32_t *crc_out) {
  return gzip_compress_host(in, n, opts, out, out_len, crc_out, nullptr, nullptr);
}

int zt_gzip_compress_indexed(const uint8_t *in, size_t n, const zt_gzip_opts *opts, uint8_t **out, size_t *out_len,
                             uint32_t *crc_out, uint8_t **idx, size_t *idx_len) {
  if (!idx || !idx_len) return set_error(ZT_E_ARG, "null index output");
  if (out) *out = nullptr;
  *idx = nullptr;
  *idx_len = 0;
  return gzip_compress_host(in, n, opts, out, out_len, crc_out, idx, idx_len);
}

int zt_gunzip(const uint8_t *in, size_t n, uint8_t **out, size_t *out_len, zt_gzip_member **members,
              size_t *nmembers) {
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if (n && !in) return set_error(ZT_E_ARG, "null input");
  std::vector<zt_gzip_member> mem;
  std::vector<uint8_t> data;
  size_t ip = 0;
  // the input goes to the device once; every member decodes from there
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  void *d_in = nullptr;
  if (n) {
    ZT_TRY(scratch(c, kContainerIn, n + 64, &d_in));
    ZT_TRY(upload(c, d_in, in, n, c->stream));
  }
  // src/GUnzip.ts:57-65: members until the input is consumed (header and
  // trailer checks: gunzip_chain.h, shared with zt_gunzip_batch)
  while (ip < n) {
    zt_gzip_member m;
    GzError ge;
    size_t body = 0;
    if (gzip_parse_header(in, n, ip, &m, &body, &ge)) return set_error(ge.code, ge.msg);
    // body (src/GUnzip.ts:149-153): the engine's RawInflate from index `body`
    uint8_t *o = nullptr;
    size_t olen = 0, eip = 0;
    ZT_TRY(inflate_dev_member(c, (const uint8_t *)d_in, n, body, &o, &olen, &eip));
    uint32_t crc = 0;
    const int rc = zt_crc32_update(0, o, olen, &crc);
    if (rc) {
      zt_free(o);
      return rc;
    }
    size_t next = 0;
    if (gzip_check_trailer(in, n, eip, crc, olen, &m, &next, &ge)) {
      zt_free(o);
      return set_error(ge.code, ge.msg);
    }
    m.data_off = data.size();
    m.data_len = olen;
    data.insert(data.end(), o, o + olen);
    zt_free(o);
    mem.push_back(m);
    ip = next;
  }
  uint8_t *h = host_out(data.size());
  if (!h) return set_error(ZT_E_NOMEM, "host allocation failed");
  if (!data.empty()) memcpy(h, data.data(), data.size());
  *out = h;
  *out_len = data.size();
  if (members) {
    *members = (zt_gzip_member *)malloc((mem.size() ? mem.size() : 1) * sizeof(zt_gzip_member));
    if (!*members) {
      zt_free(h);
      return set_error(ZT_E_NOMEM, "host allocation failed");
    }
    if (!mem.empty()) memcpy(*members, mem.data(), mem.size() * sizeof(zt_gzip_member));
  }
  if (nmembers) *nmembers = mem.size();
  return ZT_OK;
}

// zt_zlib_compress, and with idx non-null zt_zlib_compress_indexed
static int zlib_compress_host(const uint8_t *in, size_t n, const zt_deflate_opts *opts, uint8_t **out,
                              size_t *out_len, uint32_t *adler_out, uint8_t **idx, size_t *idx_len) {
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if (n && !in) return set_error(ZT_E_ARG, "null input");
  const int ct = opts ? opts->compression_type : 2;
  if (ct < 0 || ct > 2) return set_error(ZT_E_INVALID_COMPRESSION_TYPE, "invalid compression type");
  return compress_member_host(frame_zlib(ct), in, n, opts, out, out_len, adler_out, idx, idx_len);
}

int zt_zlib_compress(const uint8_t *in, size_t n, const zt_deflate_opts *opts, uint8_t **out, size_t *out_len,
                     uint32_t *adler_out) {
  return zlib_compress_host(in, n, opts, out, out_len, adler_out, nullptr, nullptr);
}

int zt_zlib_compress_indexed(const uint8_t *in, size_t n, const zt_deflate_opts *opts, uint8_t **out, size_t *out_len,
                             uint32_t *adler_out, uint8_t **idx, size_t *idx_len) {
  if (!idx || !idx_len) return set_error(ZT_E_ARG, "null index output");
  if (out) *out = nullptr;
  *idx = nullptr;
  *idx_len = 0;
  return zlib_compress_host(in, n, opts, out, out_len, adler_out, idx, idx_len);
}

int zt_zlib_decompress(const uint8_t *in, size_t n, size_t index, int verify, uint8_t **out, size_t *out_len,
                       size_t *end_ip, uint32_t *adler_out) {
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if (n && !in) return set_error(ZT_E_ARG, "null input");
  // src/Inflate.ts:44-58
  ZlibHeader h;
  int code;
  std::string msg;
  if (zlib_header_status(zlib_parse_header(in, n, index, &h), h, &code, &msg)) return set_error(code, msg);
  if (h.fdict) return set_error(ZT_E_ZLIB_FDICT, "fdict flag is not supported");
  uint8_t *o = nullptr;
  size_t olen = 0, eip = 0;
  ZT_TRY(zt_inflate_raw(in, n, index + 2, nullptr, &o, &olen, &eip));
  uint32_t adler = 1;
  if (verify) {
    // src/Inflate.ts:80-90 (the Adler-32 of the output, on the GPU)
    const int rc = zt_adler32_update(1, o, olen, &adler);
    if (rc) {
      zt_free(o);
      return rc;
    }
    Reader t{in, n, eip};
    uint32_t want = 0;
    for (int k = 0; k < 4; ++k) want = (want << 8) | t.u8();
    if (adler != want) {
      zt_free(o);
      return set_error(ZT_E_ZLIB_ADLER, "invalid adler-32 checksum");
    }
  }
  *out = o;
  *out_len = olen;
  if (end_ip) *end_ip = eip;
  if (adler_out) *adler_out = adler;
  return ZT_OK;
}

}  // extern "C"
