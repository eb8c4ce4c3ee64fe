// dict_api.cpp -- preset dictionaries (include/zt_dict.h): raw DEFLATE with a
// dictionary in front of the stream's history, and RFC 1950 FDICT framing.
//
// Deflate: every dictionary call is a batch (batch_api.cpp) -- one stream is a
// batch of one -- whose streams' first match workgroup loads the dictionary's
// usable tail as history (deflate.hip: DictView, match_dict_kernel).  Inflate: one
// wavefront per stream (inflate.hip) with the dictionary's last 32 KiB as the
// history every job points at; each device holds one copy.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/zt_dict.h"
#include "zt_internal.h"

using namespace zt;

namespace {

// streams [i0, i1) of the batch on device `dev` (this thread's afterwards)
int inflate_share(int dev, const uint8_t *const *in, const size_t *n, const size_t *index, size_t i0, size_t i1,
                  const uint8_t *dict, size_t dict_len, uint8_t **out, size_t *out_len, size_t *end_ip, int *status,
                  std::string *err) {
  auto fail = [&](int rc) {
    *err = zt_last_error_message();
    return rc;
  };
  if (zt_set_device(dev)) return fail(ZT_E_NO_DEVICE);
  DeviceCtx *c;
  if (int rc = get_ctx(&c)) return fail(rc);
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  const uint32_t wlen = dict_window_len(dict_len);
  void *d_hist;
  if (int rc = scratch(c, kDict, wlen, &d_hist)) return fail(rc);
  if (hipMemcpyAsync(d_hist, dict + dict_window_off(dict_len), wlen, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return fail(set_error(ZT_E_HIP, "dictionary upload failed"));
  const int rc = inflate_host_batch_hist(in + i0, n + i0, index ? index + i0 : nullptr, i1 - i0,
                                         static_cast<const uint8_t *>(d_hist), wlen, out + i0, out_len + i0,
                                         end_ip ? end_ip + i0 : nullptr, status + i0);
  return rc ? fail(rc) : ZT_OK;
}

int inflate_batch_dict(const uint8_t *const *in, const size_t *n, const size_t *index, size_t count,
                       const uint8_t *dict, size_t dict_len, uint8_t **out, size_t *out_len, size_t *end_ip,
                       int *status) {
  for (size_t i = 0; i < count; ++i) {
    out[i] = nullptr;
    out_len[i] = 0;
    status[i] = ZT_OK;
    if (n[i] && !in[i]) return set_error(ZT_E_ARG, "null input");
  }
  const std::vector<int> devs = batch_devices();
  const size_t nd = std::min(devs.size(), count);
  const int caller_dev = current_device();
  std::vector<int> rc(nd, ZT_OK);
  std::vector<std::string> err(nd);
  // contiguous shares of about equal compressed bytes
  std::vector<size_t> cut(nd + 1, count);
  cut[0] = 0;
  if (nd > 1) {
    uint64_t total = 0, acc = 0;
    for (size_t i = 0; i < count; ++i) total += n[i] + 256;
    size_t d = 1;
    for (size_t i = 0; i < count && d < nd; ++i) {
      acc += n[i] + 256;
      if (acc * nd >= total * d) cut[d++] = i + 1;
    }
  }
  if (nd == 1) {
    rc[0] = inflate_share(devs[0], in, n, index, 0, count, dict, dict_len, out, out_len, end_ip, status, &err[0]);
  } else {
    std::vector<std::thread> th;
    for (size_t d = 0; d < nd; ++d)
      th.emplace_back([&, d] {
        if (cut[d] < cut[d + 1])
          rc[d] = inflate_share(devs[d], in, n, index, cut[d], cut[d + 1], dict, dict_len, out, out_len, end_ip,
                                status, &err[d]);
      });
    for (auto &t : th) t.join();
  }
  zt_set_device(caller_dev);
  for (size_t d = 0; d < nd; ++d)
    if (rc[d]) return set_error(rc[d], err[d]);
  return ZT_OK;
}

}  // namespace

extern "C" {

int zt_deflate_raw_batch_dict(const uint8_t *const *in, const size_t *n, size_t count, const zt_deflate_opts *opts,
                              const uint8_t *dict, size_t dict_len, uint8_t **out, size_t *out_len, int *status) {
  if (dict_len == 0) return zt_deflate_raw_batch(in, n, count, opts, out, out_len, status);
  if (count == 0) return ZT_OK;
  if (!in || !n || !out || !out_len || !status || !dict) return set_error(ZT_E_ARG, "null argument");
  return deflate_batch_host(in, n, count, opts, HostDict{dict, dict_len}, false, 0, out, out_len, status);
}

int zt_deflate_raw_dict(const uint8_t *in, size_t n, const zt_deflate_opts *opts, const uint8_t *dict,
                        size_t dict_len, uint8_t **out, size_t *out_len) {
  if (dict_len == 0) return zt_deflate_raw(in, n, opts, out, out_len);
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if ((n && !in) || !dict) return set_error(ZT_E_ARG, "null input");
  int st = 0;
  return deflate_batch_host(&in, &n, 1, opts, HostDict{dict, dict_len}, false, 0, out, out_len, &st);
}

int zt_zlib_compress_batch_dict(const uint8_t *const *in, const size_t *n, size_t count,
                                const zt_deflate_opts *opts, const uint8_t *dict, size_t dict_len, uint8_t **out,
                                size_t *out_len, int *status) {
  if (dict_len == 0) return zt_zlib_compress_batch(in, n, count, opts, out, out_len, status);
  if (count == 0) return ZT_OK;
  if (!in || !n || !out || !out_len || !status || !dict) return set_error(ZT_E_ARG, "null argument");
  uint32_t dictid = 1;
  ZT_TRY(zt_adler32_update(1, dict, dict_len, &dictid));  // (the checksum kernel, over the whole dictionary)
  return deflate_batch_host(in, n, count, opts, HostDict{dict, dict_len}, true, dictid, out, out_len, status);
}

int zt_zlib_compress_dict(const uint8_t *in, size_t n, const zt_deflate_opts *opts, const uint8_t *dict,
                          size_t dict_len, uint8_t **out, size_t *out_len, uint32_t *adler_out) {
  if (dict_len == 0) return zt_zlib_compress(in, n, opts, out, out_len, adler_out);
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if ((n && !in) || !dict) return set_error(ZT_E_ARG, "null input");
  const int ct = opts ? opts->compression_type : 2;
  if (ct < 0 || ct > 2) return set_error(ZT_E_INVALID_COMPRESSION_TYPE, "invalid compression type");
  int st = 0;
  ZT_TRY(zt_zlib_compress_batch_dict(&in, &n, 1, opts, dict, dict_len, out, out_len, &st));
  if (adler_out) {  // (the member's trailer)
    const uint8_t *t = *out + *out_len - 4;
    *adler_out = (uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | t[3];
  }
  return ZT_OK;
}

int zt_inflate_raw_batch_dict(const uint8_t *const *in, const size_t *n, size_t count, const zt_inflate_opts *opts,
                              const uint8_t *dict, size_t dict_len, uint8_t **out, size_t *out_len, size_t *end_ip,
                              int *status) {
  if (dict_len == 0) return zt_inflate_raw_batch(in, n, count, opts, out, out_len, end_ip, status);
  if (count == 0) return ZT_OK;
  if (!in || !n || !out || !out_len || !status || !dict) return set_error(ZT_E_ARG, "null argument");
  return inflate_batch_dict(in, n, nullptr, count, dict, dict_len, out, out_len, end_ip, status);
}

int zt_inflate_raw_dict(const uint8_t *in, size_t n, size_t index, const zt_inflate_opts *opts, const uint8_t *dict,
                        size_t dict_len, uint8_t **out, size_t *out_len, size_t *end_ip) {
  if (dict_len == 0) return zt_inflate_raw(in, n, index, opts, out, out_len, end_ip);
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if ((n && !in) || !dict) return set_error(ZT_E_ARG, "null input");
  int st = 0;
  size_t ip = 0;
  // (one stream: the current device, whatever zt_set_devices says)
  std::string err;
  const int rc = inflate_share(current_device(), &in, &n, &index, 0, 1, dict, dict_len, out, out_len, &ip, &st, &err);
  if (rc) return set_error(rc, err);
  if (end_ip) *end_ip = ip;
  return ZT_OK;
}

int zt_zlib_decompress_dict(const uint8_t *in, size_t n, size_t index, int verify, const uint8_t *dict,
                            size_t dict_len, uint8_t **out, size_t *out_len, size_t *end_ip, uint32_t *adler_out) {
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if ((n && !in) || (dict_len && !dict)) return set_error(ZT_E_ARG, "null input");
  ZlibHeader h;
  const ZlibHdr hs = zlib_parse_header(in, n, index, &h);
  // no FDICT (or a header zt_zlib_decompress rejects with its own message)
  if (!h.fdict) return zt_zlib_decompress(in, n, index, verify, out, out_len, end_ip, adler_out);
  if (dict_len == 0) return set_error(ZT_E_ZLIB_FDICT, "fdict flag is not supported");
  if (hs == ZH_BROKEN) return set_error(ZT_E_INPUT_BROKEN, "input buffer is broken");
  uint32_t given = 1;
  ZT_TRY(zt_adler32_update(1, dict, dict_len, &given));
  if (given != h.dictid) {
    char msg[96];
    snprintf(msg, sizeof msg, "invalid dictionary id: 0x%x / 0x%x", h.dictid, given);
    return set_error(ZT_E_ZLIB_DICTID, msg);
  }
  uint8_t *o = nullptr;
  size_t olen = 0, eip = 0;
  ZT_TRY(zt_inflate_raw_dict(in, n, h.body, nullptr, dict, dict_len, &o, &olen, &eip));
  uint32_t adler = 1;
  if (verify) {
    const int rc = zt_adler32_update(1, o, olen, &adler);
    if (rc) {
      zt_free(o);
      return rc;
    }
    uint32_t want = 0;
    for (int k = 0; k < 4; ++k) want = (want << 8) | (eip + k < n ? in[eip + k] : 0u);
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
