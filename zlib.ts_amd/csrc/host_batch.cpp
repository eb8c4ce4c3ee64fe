// host_batch.cpp -- what every batch entry point shares on the host: the
// fan-out over the batch devices and the packer (zt_internal.h; the
// arithmetic lives in batch_plan.h).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/zt_strategy.h"
#include "zt_internal.h"

namespace zt {

static thread_local int t_strategy = ZT_STRATEGY_DEFAULT;

StrategyScope::StrategyScope(int strategy) : prev_(t_strategy) { t_strategy = strategy; }
StrategyScope::~StrategyScope() { t_strategy = prev_; }

int strategy_check(int strategy) {
  if (strategy == ZT_STRATEGY_DEFAULT || strategy == ZT_STRATEGY_HUFFMAN_ONLY || strategy == ZT_STRATEGY_RLE)
    return ZT_OK;
  return set_error(ZT_E_ARG, "invalid strategy: " + std::to_string(strategy));
}

int resolve_opts(const zt_deflate_opts *o, int *ctype, int *level) {
  const int rc = resolve_deflate_opts(o, ctype, level);
  if (rc) return set_error(rc, "invalid compression type");
  *level = level_with_strategy(*level, t_strategy);
  return ZT_OK;
}

std::vector<int> fanout_devices(size_t count) {
  std::vector<int> devs = batch_devices();
  devs.resize(std::max<size_t>(1, std::min(devs.size(), count)));
  return devs;
}

std::vector<ShareResult> for_each_device(const std::vector<int> &devs, const std::vector<std::vector<size_t>> &shares,
                                         const std::function<int(size_t, DeviceCtx *, const std::vector<size_t> &)> &fn) {
  // the host's copy threads split between the device threads (8 per device
  // thread put 64 on one GPU's 16-thread CPU share with 8 devices; 32 in all
  // packed fastest: slowest device's host stages 10.9 GiB/s with 16, 13.3
  // with 32); ZT_BATCH_COPY_THREADS overrides the total
  static const size_t total = getenv("ZT_BATCH_COPY_THREADS") ? (size_t)atoi(getenv("ZT_BATCH_COPY_THREADS")) : 32;
  const size_t nd = shares.size();
  const int caller_dev = current_device();
  std::vector<ShareResult> res = fan_out(shares, [&](size_t d) -> int {
    if (nd > 1) set_copy_threads(std::max<size_t>(2, total / nd));
    ZT_TRY(zt_set_device(devs[d]));
    DeviceCtx *c;
    ZT_TRY(get_ctx(&c));
    std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
    return fn(d, c, shares[d]);
  }, zt_last_error_message);
  zt_set_device(caller_dev);
  return res;
}

void pack_items(uint8_t *stage, const uint8_t *const *in, const size_t *n, const std::vector<size_t> &ids,
                const PackLayout &L, size_t a, size_t b, bool zero_pad, size_t copy_bytes) {
  parallel_copy(b - a, [&](size_t j) {
    const size_t k = a + j, len = n[ids[k]];
    uint8_t *dst = stage + (L.off[k] - L.off[a]);
    copy_to_staging(dst, in[ids[k]], len);
    if (zero_pad) memset(dst + len, 0, (k + 1 < L.off.size() ? L.off[k + 1] : L.total) - L.off[k] - len);
  }, copy_bytes);
}

int pack_upload(DeviceCtx *c, const uint8_t *const *in, const size_t *n, const std::vector<size_t> &ids,
                const PackLayout &L, const PackMode &mode, void **d_in) {
  ZT_TRY(scratch(c, kIn, L.total + 64, d_in));
  void *h;
  ZT_TRY(pinned(c, L.total, &h));
  uint8_t *stage = static_cast<uint8_t *>(h), *dev = static_cast<uint8_t *>(*d_in);
  const size_t m = ids.size(), budget = mode.copy_bytes ? mode.copy_bytes : L.total;
  const double t0 = mode.pack_ms ? now_ms() : 0;
  if (mode.chunked) {
    // (every chunk with the whole batch's copy threads)
    const std::vector<size_t> runs = chunk_runs(L.off, L.total, 32u << 20);
    for (size_t r = 0; r + 1 < runs.size(); ++r) {
      const size_t a = runs[r], b = runs[r + 1], lo = L.off[a], hi = b < m ? L.off[b] : L.total;
      pack_items(stage + lo, in, n, ids, L, a, b, mode.zero_pad, budget);
      ZT_HIP(hipMemcpyAsync(dev + lo, stage + lo, hi - lo, hipMemcpyHostToDevice, c->stream));
    }
  } else {
    pack_items(stage, in, n, ids, L, 0, m, mode.zero_pad, budget);
  }
  if (mode.pack_ms) *mode.pack_ms += now_ms() - t0;
  if (!mode.chunked && L.total) ZT_HIP(hipMemcpyAsync(dev, stage, L.total, hipMemcpyHostToDevice, c->stream));
  return ZT_OK;
}

}  // namespace zt
