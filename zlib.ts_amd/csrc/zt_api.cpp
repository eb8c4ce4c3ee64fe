// zt_api.cpp -- the C-ABI entry points (include/zt.h) that belong to no other
// file: the version and the checksums.  Contexts and errors: ctx.cpp; host
// output memory: host_mem.cpp; transfers: xfer.cpp.
//
// Every entry point computes on the GPU.  There is deliberately no CPU
// fallback: without a HIP device the calls fail with ZT_E_NO_DEVICE.
#include <mutex>

#include "zt_internal.h"

using namespace zt;

extern "C" {

const char *zt_version(void) { return "zlib.ts_amd 0.1 (gfx950)"; }

int zt_dev_checksums(const void *d_in, size_t n, uint32_t crc_in, uint32_t adler_in, uint32_t *crc_out,
                     uint32_t *adler_out, void *stream) {
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  if (n == 0) {
    if (crc_out) *crc_out = crc_in;
    if (adler_out) *adler_out = adler_in;
    return ZT_OK;
  }
  void *res;
  ZT_TRY(scratch(c, kSmall, 16, &res));
  ZT_TRY(checksums_dev(c, (const uint8_t *)d_in, n, crc_out != nullptr, adler_out != nullptr, crc_in, adler_in,
                       (uint32_t *)res, s));
  uint32_t h[2];
  ZT_HIP(hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, s));
  ZT_HIP(hipStreamSynchronize(s));
  if (crc_out) *crc_out = h[0];
  if (adler_out) *adler_out = h[1];
  return ZT_OK;
}

static int checksums_host(const uint8_t *data, size_t len, uint32_t crc_in, uint32_t adler_in, uint32_t *crc_out,
                          uint32_t *adler_out) {
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  if (len == 0) {  // the reference returns its inputs untouched (no % 65521)
    if (crc_out) *crc_out = crc_in;
    if (adler_out) *adler_out = adler_in;
    return ZT_OK;
  }
  if (!data) return set_error(ZT_E_ARG, "null data");
  void *d;
  ZT_TRY(scratch(c, kIn, len, &d));
  ZT_TRY(upload(c, d, data, len, c->stream));
  return zt_dev_checksums(d, len, crc_in, adler_in, crc_out, adler_out, c->stream);
}

int zt_crc32_update(uint32_t crc, const uint8_t *data, size_t len, uint32_t *out) {
  if (!out) return set_error(ZT_E_ARG, "null out");
  return checksums_host(data, len, crc, 0, out, nullptr);
}

int zt_adler32_update(uint32_t adler, const uint8_t *data, size_t len, uint32_t *out) {
  if (!out) return set_error(ZT_E_ARG, "null out");
  return checksums_host(data, len, 0, adler, nullptr, out);
}

int zt_checksums(const uint8_t *data, size_t len, uint32_t crc_in, uint32_t adler_in, uint32_t *crc_out,
                 uint32_t *adler_out) {
  return checksums_host(data, len, crc_in, adler_in, crc_out, adler_out);
}

}  // extern "C"
