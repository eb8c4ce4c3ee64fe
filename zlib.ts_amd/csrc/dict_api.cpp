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
#include <vector>

#include "../../include/zt_dict.h"
#include "zt_internal.h"

using namespace zt;

namespace {

// streams [i0, i1) of the batch on the locked context c (for_each_device)
int inflate_share(DeviceCtx *c, const uint8_t *const *in, const size_t *n, const size_t *index, size_t i0, size_t i1,
                  const uint8_t *dict, size_t dict_len, uint8_t **out, size_t *out_len, size_t *end_ip, int *status) {
  const uint32_t wlen = dict_window_len(dict_len);
  void *d_hist;
  ZT_TRY(scratch(c, kDict, wlen, &d_hist));
  if (hipMemcpyAsync(d_hist, dict + dict_window_off(dict_len), wlen, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return set_error(ZT_E_HIP, "dictionary upload failed");
  return inflate_host_batch_hist(in + i0, n + i0, index ? index + i0 : nullptr, i1 - i0,
                                 static_cast<const uint8_t *>(d_hist), wlen, out + i0, out_len + i0,
                                 end_ip ? end_ip + i0 : nullptr, status + i0);
}

// the batch over `devs`: contiguous shares of about equal compressed bytes
// (inflate_host_batch_hist takes a range); the first failed share's code and message
int inflate_batch_dict(const std::vector<int> &devs, const uint8_t *const *in, const size_t *n, const size_t *index,
                       size_t count, const uint8_t *dict, size_t dict_len, uint8_t **out, size_t *out_len,
                       size_t *end_ip, int *status) {
  for (size_t i = 0; i < count; ++i) {
    out[i] = nullptr;
    out_len[i] = 0;
    status[i] = ZT_OK;
    if (n[i] && !in[i]) return set_error(ZT_E_ARG, "null input");
  }
  const std::vector<size_t> cut = contiguous_cuts(n, count, devs.size());
  std::vector<std::vector<size_t>> shares(devs.size());
  for (size_t d = 0; d < devs.size(); ++d)
    for (size_t i = cut[d]; i < cut[d + 1]; ++i) shares[d].push_back(i);
  const std::vector<ShareResult> res =
      for_each_device(devs, shares, [&](size_t d, DeviceCtx *c, const std::vector<size_t> &) {
        return inflate_share(c, in, n, index, cut[d], cut[d + 1], dict, dict_len, out, out_len, end_ip, status);
      });
  for (const ShareResult &r : res)
    if (r.code) return set_error(r.code, r.msg);
  return ZT_OK;
}

}  // namespace

extern "C" {

int zt_deflate_raw_batch_dict(const uint8_t *const *in, const size_t *n, size_t count, const zt_deflate_opts *opts,
                              const uint8_t *dict, size_t dict_len, uint8_t **out, size_t *out_len, int *status) {
  if (dict_len == 0) return zt_deflate_raw_batch(in, n, count, opts, out, out_len, status);
  if (count == 0) return ZT_OK;
  if (!in || !n || !out || !out_len || !status || !dict) return set_error(ZT_E_ARG, "null argument");
  return deflate_batch_host(in, n, count, opts, HostDict{dict, dict_len}, frame_raw(), out, out_len, status);
}

int zt_deflate_raw_dict(const uint8_t *in, size_t n, const zt_deflate_opts *opts, const uint8_t *dict,
                        size_t dict_len, uint8_t **out, size_t *out_len) {
  if (dict_len == 0) return zt_deflate_raw(in, n, opts, out, out_len);
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if ((n && !in) || !dict) return set_error(ZT_E_ARG, "null input");
  int st = 0;
  return deflate_batch_host(&in, &n, 1, opts, HostDict{dict, dict_len}, frame_raw(), out, out_len, &st);
}

int zt_zlib_compress_batch_dict(const uint8_t *const *in, const size_t *n, size_t count,
                                const zt_deflate_opts *opts, const uint8_t *dict, size_t dict_len, uint8_t **out,
                                size_t *out_len, int *status) {
  if (dict_len == 0) return zt_zlib_compress_batch(in, n, count, opts, out, out_len, status);
  if (count == 0) return ZT_OK;
  if (!in || !n || !out || !out_len || !status || !dict) return set_error(ZT_E_ARG, "null argument");
  uint32_t dictid = 1;
  ZT_TRY(zt_adler32_update(1, dict, dict_len, &dictid));  // (the checksum kernel, over the whole dictionary)
  return deflate_batch_host(in, n, count, opts, HostDict{dict, dict_len},
                            frame_zlib_dict(opts ? opts->compression_type : 2, dictid), out, out_len, status);
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
  return inflate_batch_dict(fanout_devices(count), in, n, nullptr, count, dict, dict_len, out, out_len, end_ip,
                            status);
}

int zt_inflate_raw_dict(const uint8_t *in, size_t n, size_t index, const zt_inflate_opts *opts, const uint8_t *dict,
                        size_t dict_len, uint8_t **out, size_t *out_len, size_t *end_ip) {
  if (dict_len == 0) return zt_inflate_raw(in, n, index, opts, out, out_len, end_ip);
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if ((n && !in) || !dict) return set_error(ZT_E_ARG, "null input");
  int st = 0;
  size_t ip = 0;
  // (one stream: the current device, whatever zt_set_devices says)
  ZT_TRY(inflate_batch_dict({current_device()}, &in, &n, &index, 1, dict, dict_len, out, out_len, &ip, &st));
  if (end_ip) *end_ip = ip;
  return ZT_OK;
}

int zt_zlib_decompress_dict(const uint8_t *in, size_t n, size_t index, int verify, const uint8_t *dict,
                            size_t dict_len, uint8_t **out, size_t *out_len, size_t *end_ip, uint32_t *adler_out) {
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if ((n && !in) || (dict_len && !dict)) return set_error(ZT_E_ARG, "null input");
  ZlibHeader h;
  const ZlibHdr hs = zlib_parse_header(in, n, index, &h);
  int code;
  std::string hmsg;
  if (zlib_header_status(hs, h, &code, &hmsg)) return set_error(code, hmsg);
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
