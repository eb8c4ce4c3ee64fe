// ctx.cpp -- errors, timing, the per-device contexts and their grow-only
// device scratch and pinned staging.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "zt_internal.h"

namespace zt {

static thread_local std::string g_err;
static thread_local int g_dev = 0;

int set_error(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

int hip_fail(hipError_t e, const char *what) {
  char buf[512];
  snprintf(buf, sizeof buf, "HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return set_error(ZT_E_NO_DEVICE, buf);
  if (e == hipErrorOutOfMemory) return set_error(ZT_E_NOMEM, buf);
  return set_error(ZT_E_HIP, buf);
}

int timing_begin(DeviceCtx *c, hipStream_t s, int k) {
  if (!c->timing) return ZT_OK;
  ZT_HIP(hipEventRecord(c->ev[2 * k], s));
  return ZT_OK;
}

int timing_end(DeviceCtx *c, hipStream_t s, int k) {
  if (!c->timing) return ZT_OK;
  ZT_HIP(hipEventRecord(c->ev[2 * k + 1], s));
  return ZT_OK;
}

int timing_collect(DeviceCtx *c, double *acc_ms, uint64_t *count, int k) {
  if (!c->timing) return ZT_OK;
  float ms = 0;
  ZT_HIP(hipEventElapsedTime(&ms, c->ev[2 * k], c->ev[2 * k + 1]));
  *acc_ms += ms;
  ++*count;
  return ZT_OK;
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void host_stamp(const char *tag, const char *label) { fprintf(stderr, "[%s] %-28s %9.3f ms\n", tag, label, now_ms()); }

// (no other file's static initialiser calls into the library, so these do
// not depend on the link order)
static std::mutex g_mu;
static std::vector<DeviceCtx *> g_ctx;
static std::mutex g_devs_mu;
static std::vector<int> g_devs;  // zt_set_devices; empty: the calling thread's device

// Test-only rehearsal of a multi-GPU node on fewer GPUs: ZT_ALIAS_DEVICES=k
// (read once) makes the library present k logical devices, logical d running
// on HIP device d % (HIP device count) with its own context (streams,
// scratch, pinned staging, host threads) -- what zt_set_devices(mask) spreads
// a batch over.  Unset: logical = HIP devices.
static int hip_count() {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count;
}
static int alias_count() {
  static const int k = [] {
    const char *e = getenv("ZT_ALIAS_DEVICES");
    const int v = e ? atoi(e) : 0;
    return v > 0 && v <= 64 ? v : 0;
  }();
  return k;
}

int get_ctx(DeviceCtx **out) {
  const int hc = hip_count();
  if (hc <= 0) return set_error(ZT_E_NO_DEVICE, "no HIP device visible (libzt computes on the GPU only)");
  const int count = alias_count() ? alias_count() : hc;
  if (g_dev < 0 || g_dev >= count) return set_error(ZT_E_NO_DEVICE, "invalid device index");
  const int phys = g_dev % hc;
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_ctx.size() < (size_t)count) g_ctx.resize(count, nullptr);
  ZT_HIP(hipSetDevice(phys));
  if (!g_ctx[g_dev]) {
    DeviceCtx *c = new DeviceCtx();
    c->device = g_dev;
    c->phys = phys;
    ZT_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    ZT_HIP(hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
    ZT_HIP(hipEventCreateWithFlags(&c->aux_ev, hipEventDisableTiming));
    hipDeviceProp_t prop;
    ZT_HIP(hipGetDeviceProperties(&prop, phys));
    c->num_cu = prop.multiProcessorCount;
    uint32_t bt[256], nib[ZT_CRC_NIB_N], x2n[32];
    crc_host_tables(bt, nib, x2n);
    ZT_HIP(hipMalloc(&c->d_crc_nib, sizeof nib));
    ZT_HIP(hipMalloc(&c->d_crc_x2n, sizeof x2n));
    ZT_HIP(hipMemcpy(c->d_crc_nib, nib, sizeof nib, hipMemcpyHostToDevice));
    ZT_HIP(hipMemcpy(c->d_crc_x2n, x2n, sizeof x2n, hipMemcpyHostToDevice));
    uint32_t shift[ZT_CRC_SHIFT_N] = {};
    crc_shift_tables(x2n, shift);
    ZT_HIP(hipMalloc(&c->d_crc_shift, sizeof shift));
    ZT_HIP(hipMemcpy(c->d_crc_shift, shift, sizeof shift, hipMemcpyHostToDevice));
    ZT_HIP(hipMalloc(&c->d_ck_acc, sizeof(CkAcc)));
    ZT_HIP(hipMemset(c->d_ck_acc, 0, sizeof(CkAcc)));
    for (auto &e : c->ev) ZT_HIP(hipEventCreate(&e));
    g_ctx[g_dev] = c;
  }
  *out = g_ctx[g_dev];
  return ZT_OK;
}

int scratch(DeviceCtx *c, int slot, size_t bytes, void **ptr) {
  if (bytes == 0) bytes = 16;
  if (c->buf_size[slot] < bytes) {
    if (c->d_buf[slot]) {
      ZT_HIP(hipDeviceSynchronize());  // any stream may still use it
      ZT_HIP(hipFree(c->d_buf[slot]));
      c->d_buf[slot] = nullptr;
      c->buf_size[slot] = 0;
    }
    size_t sz = bytes + bytes / 4;
    if (const hipError_t e = hipMalloc(&c->d_buf[slot], sz)) {
      c->d_buf[slot] = nullptr;
      (void)hipGetLastError();  // (a caller that falls back must not see it at its next launch check)
      return hip_fail(e, "hipMalloc (scratch)");
    }
    c->buf_size[slot] = sz;
  }
  *ptr = c->d_buf[slot];
  return ZT_OK;
}

// the grow-only pinned allocator behind pinned() and mailbox()
static int pinned_grow(DeviceCtx *c, int slot, size_t bytes, unsigned flags, const char *what, void **ptr) {
  if (c->pinned_size[slot] < bytes) {
    if (c->h_pinned[slot]) {
      ZT_HIP(hipDeviceSynchronize());
      ZT_HIP(hipHostFree(c->h_pinned[slot]));
      c->h_pinned[slot] = nullptr;
      c->pinned_size[slot] = 0;
    }
    const size_t sz = bytes + bytes / 4;
    if (const hipError_t e = hipHostMalloc(&c->h_pinned[slot], sz, flags)) {
      c->h_pinned[slot] = nullptr;
      (void)hipGetLastError();
      return hip_fail(e, what);
    }
    c->pinned_size[slot] = sz;
  }
  *ptr = c->h_pinned[slot];
  return ZT_OK;
}

int pinned(DeviceCtx *c, size_t bytes, void **ptr, int slot) {
  // (the inflate metadata is written and read by q_copy kernels: coherent)
  return pinned_grow(c, slot, bytes ? bytes : 16, slot == kPinInflateMeta ? hipHostMallocCoherent : hipHostMallocDefault,
                     "hipHostMalloc (staging)", ptr);
}

int mailbox(DeviceCtx *c, size_t n, void **p) {
  // coherent: the kernels' stores are visible to the host once the stream is synchronized
  return pinned_grow(c, kPinMailbox, n < 4096 ? 4096 : n, hipHostMallocCoherent, "hipHostMalloc (mailbox)", p);
}

int readback(DeviceCtx *c, void *h_dst, const void *d_src, size_t n, hipStream_t s) {
  if (!n) return ZT_OK;
  void *mb;
  ZT_TRY(mailbox(c, n, &mb));
  ZT_TRY(x_copy(mb, d_src, n, s));
  ZT_HIP(hipStreamSynchronize(s));
  memcpy(h_dst, mb, n);
  return ZT_OK;
}

int current_device() { return g_dev; }

std::vector<int> batch_devices() {
  std::lock_guard<std::mutex> lk(g_devs_mu);
  if (g_devs.empty()) return {g_dev};
  return g_devs;
}

}  // namespace zt

using namespace zt;

extern "C" {

int zt_set_devices(uint64_t mask) {
  const int count = zt_device_count();
  std::vector<int> v;
  for (int d = 0; d < 64; ++d)
    if ((mask >> d) & 1) {
      if (d >= count) return set_error(ZT_E_NO_DEVICE, "invalid device index");
      v.push_back(d);
    }
  std::lock_guard<std::mutex> lk(g_devs_mu);
  g_devs = v;
  return ZT_OK;
}

int zt_device_count(void) {
  const int hc = hip_count();
  return hc > 0 && alias_count() ? alias_count() : hc;
}

int zt_set_device(int device) {
  int count = zt_device_count();
  if (device < 0 || device >= count) return set_error(ZT_E_NO_DEVICE, "invalid device index");
  g_dev = device;
  return ZT_OK;
}

const char *zt_last_error_message(void) { return g_err.c_str(); }

int zt_timing_enable(int on) {
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  c->timing = on != 0;
  c->times = zt_kernel_times{};
  return ZT_OK;
}

int zt_timing_read(zt_kernel_times *out) {
  if (!out) return set_error(ZT_E_ARG, "null output");
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  *out = c->times;
  return ZT_OK;
}

int zt_scratch_bytes(size_t *device_bytes, size_t *pinned_bytes) {
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  size_t d = 0, h = 0;
  for (size_t v : c->buf_size) d += v;
  for (size_t v : c->pinned_size) h += v;
  if (device_bytes) *device_bytes = d;
  if (pinned_bytes) *pinned_bytes = h;
  return ZT_OK;
}

int zt_release_scratch(void) {
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  ZT_HIP(hipDeviceSynchronize());
  for (int k = 0; k < DeviceCtx::kSlots; ++k) {
    if (c->d_buf[k]) ZT_HIP(hipFree(c->d_buf[k]));
    c->d_buf[k] = nullptr;
    c->buf_size[k] = 0;
  }
  for (int k = 0; k < kPinnedSlots; ++k) {
    if (c->h_pinned[k]) ZT_HIP(hipHostFree(c->h_pinned[k]));
    c->h_pinned[k] = nullptr;
    c->pinned_size[k] = 0;
  }
  host_pool_drop();  // the host output pool's free buffers
  return ZT_OK;
}

}  // extern "C"
