// strategy_api.cpp -- the strategy entry points (include/zt_strategy.h): each
// is the plain call of the same name inside a StrategyScope, so that the
// level resolve_opts hands out on this thread carries the strategy down to
// deflate_params (zt_internal.h).  zt_deflate_plan_set_strategy lives with the
// plan, in deflate_api.cpp.
#include "../../include/zt_strategy.h"
#include "zt_internal.h"

using namespace zt;

extern "C" {

int zt_deflate_raw_strategy(const uint8_t *in, size_t n, const zt_deflate_opts *opts, int strategy, uint8_t **out,
                            size_t *out_len) {
  ZT_TRY(strategy_check(strategy));
  const StrategyScope scope(strategy);
  return zt_deflate_raw(in, n, opts, out, out_len);
}

int zt_deflate_raw_batch_strategy(const uint8_t *const *in, const size_t *n, size_t count,
                                  const zt_deflate_opts *opts, int strategy, uint8_t **out, size_t *out_len,
                                  int *status) {
  ZT_TRY(strategy_check(strategy));
  const StrategyScope scope(strategy);
  return zt_deflate_raw_batch(in, n, count, opts, out, out_len, status);
}

int zt_zlib_compress_strategy(const uint8_t *in, size_t n, const zt_deflate_opts *opts, int strategy, uint8_t **out,
                              size_t *out_len, uint32_t *adler_out) {
  ZT_TRY(strategy_check(strategy));
  const StrategyScope scope(strategy);
  return zt_zlib_compress(in, n, opts, out, out_len, adler_out);
}

int zt_gzip_compress_strategy(const uint8_t *in, size_t n, const zt_gzip_opts *opts, int strategy, uint8_t **out,
                              size_t *out_len, uint32_t *crc_out) {
  ZT_TRY(strategy_check(strategy));
  const StrategyScope scope(strategy);
  return zt_gzip_compress(in, n, opts, out, out_len, crc_out);
}

int zt_zlib_compress_batch_strategy(const uint8_t *const *in, const size_t *n, size_t count,
                                    const zt_deflate_opts *opts, int strategy, uint8_t **out, size_t *out_len,
                                    int *status) {
  ZT_TRY(strategy_check(strategy));
  const StrategyScope scope(strategy);
  return zt_zlib_compress_batch(in, n, count, opts, out, out_len, status);
}

int zt_gzip_compress_batch_strategy(const uint8_t *const *in, const size_t *n, size_t count, const zt_gzip_opts *opts,
                                    int strategy, uint8_t **out, size_t *out_len, int *status) {
  ZT_TRY(strategy_check(strategy));
  const StrategyScope scope(strategy);
  return zt_gzip_compress_batch(in, n, count, opts, out, out_len, status);
}

}  // extern "C"
