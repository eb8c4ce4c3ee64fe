// xfer.cpp -- host <-> device transfers: the host copy helpers, the staged
// upload and download, the three-stage pipeline skeleton (StagePipe) and
// pipeline_h2d_d2h over it.
#include <immintrin.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "zt_internal.h"

namespace zt {

int x_copy(void *dst, const void *src, size_t n, hipStream_t s) {
  static const bool qc = getenv("ZT_QCOPY") != nullptr;
  if (qc) return q_copy(dst, src, n, s);
  if (n) ZT_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDefault, s));
  return ZT_OK;
}

// Copy into staging that only the DMA engine reads back: non-temporal
// (streaming) stores skip the read-for-ownership of every destination line
// and leave the caches to the source -- one read and one write of memory
// traffic per byte instead of two reads and a write, which is what several
// device threads packing at once share (config C4 on 8 GPUs).  AVX2 where
// the host has it, memcpy otherwise; an sfence at the end orders the stores
// before the caller issues the DMA.
__attribute__((target("avx2"))) static void copy_nt_avx2(uint8_t *dst, const uint8_t *src, size_t n) {
  size_t i = 0;
  const size_t head = (32 - ((uintptr_t)dst & 31)) & 31;
  if (head) {
    const size_t h = head < n ? head : n;
    memcpy(dst, src, h);
    i = h;
  }
  for (; i + 128 <= n; i += 128) {
    const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i));
    const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 32));
    const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 64));
    const __m256i d = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 96));
    _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i), a);
    _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 32), b);
    _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 64), c);
    _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 96), d);
  }
  if (i < n) memcpy(dst + i, src + i, n - i);
  _mm_sfence();
}

void copy_to_staging(void *dst, const void *src, size_t n) {
  static const bool avx2 = __builtin_cpu_supports("avx2") && getenv("ZT_NO_NT_COPY") == nullptr;
  if (avx2 && n >= 4096)
    copy_nt_avx2(static_cast<uint8_t *>(dst), static_cast<const uint8_t *>(src), n);
  else if (n)
    memcpy(dst, src, n);
}

// copy threads of parallel_copy on this thread (the batch's device threads
// split the host's copy threads between them: set_copy_threads)
static thread_local size_t tl_copy_threads = 8;
void set_copy_threads(size_t k) { tl_copy_threads = k < 1 ? 1 : k; }

void parallel_copy(size_t count, const std::function<void(size_t)> &fn, size_t total_bytes) {
  // host memcpy fan-out for the batch paths: one thread per ~8 MiB, at most
  // tl_copy_threads (8 unless a multi-device batch shares them out)
  size_t nt = total_bytes >> 23;
  if (nt > tl_copy_threads) nt = tl_copy_threads;
  if (nt > count) nt = count;
  if (nt < 2) {
    for (size_t i = 0; i < count; ++i) fn(i);
    return;
  }
  std::vector<std::thread> th;
  for (size_t t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      for (size_t i = t; i < count; i += nt) fn(i);
    });
  for (auto &x : th) x.join();
}

// Large host buffers move through two pinned 32 MiB chunks: the host copy of
// chunk k + 1 (a few threads) overlaps the DMA of chunk k -- pageable
// hipMemcpy stages through the runtime's own small buffers at a fraction of
// the PCIe rate.  Buffers below 8 MiB are copied directly.
static constexpr size_t kXferChunk = 32u << 20;

// (fresh output pages fault in during the copy: 8 threads keep a 32 MiB
// chunk's faults and copy under its DMA time; tools/micro/host_fault_probe)
static void host_copy(void *dst, const void *src, size_t n) {
  const size_t nt = n >= (16u << 20) ? 8 : n >= (8u << 20) ? 4 : 1;
  if (nt == 1) {
    copy_to_staging(dst, src, n);
    return;
  }
  std::vector<std::thread> th;
  const size_t per = (n + nt - 1) / nt;
  for (size_t t = 0; t < nt; ++t) {
    const size_t a = t * per, b = std::min(n, a + per);
    if (a < b) th.emplace_back([=] { copy_to_staging((uint8_t *)dst + a, (const uint8_t *)src + a, b - a); });
  }
  for (auto &t : th) t.join();
}

// pinned chunks kPinChunk0 + [0, count) and their events
static int xfer_setup(DeviceCtx *c, uint8_t **buf, int count) {
  for (int k = 0; k < count; ++k) {
    void *p;
    ZT_TRY(pinned(c, kXferChunk, &p, kPinChunk0 + k));
    buf[k] = static_cast<uint8_t *>(p);
    if (!c->xfer_ev[k]) ZT_HIP(hipEventCreateWithFlags(&c->xfer_ev[k], hipEventDisableTiming));
  }
  return ZT_OK;
}

// The staged copies.  buf / ev: two pinned chunks and the events behind their
// last DMA; *k: chunks these two have carried so far (chunk k uses buf[k & 1]).
// Up: a chunk is filled once its DMA of two chunks ago has left it.
static int staged_up(hipStream_t s, uint8_t *const *buf, hipEvent_t *ev, void *d_dst, const void *h_src, size_t n,
                     size_t *k) {
  for (size_t off = 0; off < n; off += kXferChunk, ++*k) {
    const size_t len = std::min(kXferChunk, n - off), b = *k & 1;
    if (*k >= 2) ZT_HIP(hipEventSynchronize(ev[b]));
    host_copy(buf[b], (const uint8_t *)h_src + off, len);
    ZT_HIP(hipMemcpyAsync((uint8_t *)d_dst + off, buf[b], len, hipMemcpyHostToDevice, s));
    ZT_HIP(hipEventRecord(ev[b], s));
  }
  return ZT_OK;
}
// Down: issue chunk j + 1, wait for chunk j, copy chunk j out.
static int staged_down(hipStream_t s, uint8_t *const *buf, hipEvent_t *ev, void *h_dst, const void *d_src, size_t n,
                       size_t *k) {
  const size_t nch = (n + kXferChunk - 1) / kXferChunk;
  auto issue = [&](size_t j) -> int {
    const size_t off = j * kXferChunk, len = std::min(kXferChunk, n - off), b = (*k + j) & 1;
    ZT_HIP(hipMemcpyAsync(buf[b], (const uint8_t *)d_src + off, len, hipMemcpyDeviceToHost, s));
    ZT_HIP(hipEventRecord(ev[b], s));
    return ZT_OK;
  };
  if (nch) ZT_TRY(issue(0));
  for (size_t j = 0; j < nch; ++j) {
    if (j + 1 < nch) ZT_TRY(issue(j + 1));
    const size_t off = j * kXferChunk, len = std::min(kXferChunk, n - off), b = (*k + j) & 1;
    ZT_HIP(hipEventSynchronize(ev[b]));
    host_copy((uint8_t *)h_dst + off, buf[b], len);
  }
  *k += nch;
  return ZT_OK;
}

int upload(DeviceCtx *c, void *d_dst, const void *h_src, size_t n, hipStream_t s) {
  if (n < (8u << 20) || host_direct(h_src, n)) {
    if (n) ZT_HIP(hipMemcpyAsync(d_dst, h_src, n, hipMemcpyHostToDevice, s));
    return ZT_OK;
  }
  uint8_t *buf[2];
  ZT_TRY(xfer_setup(c, buf, 2));
  size_t k = 0;
  ZT_TRY(staged_up(s, buf, c->xfer_ev, d_dst, h_src, n, &k));
  // the staging chunks are reused by the next call: let the last copies land
  ZT_HIP(hipEventSynchronize(c->xfer_ev[0]));
  ZT_HIP(hipEventSynchronize(c->xfer_ev[1]));
  return ZT_OK;
}

int download(DeviceCtx *c, void *h_dst, const void *d_src, size_t n, hipStream_t s) {
  if (n < (8u << 20) || host_direct(h_dst, n)) {
    if (n) ZT_HIP(hipMemcpyAsync(h_dst, d_src, n, hipMemcpyDeviceToHost, s));
    ZT_HIP(hipStreamSynchronize(s));
    return ZT_OK;
  }
  uint8_t *buf[2];
  ZT_TRY(xfer_setup(c, buf, 2));
  size_t k = 0;
  return staged_down(s, buf, c->xfer_ev, h_dst, d_src, n, &k);
}

// ---- StagePipe (zt_internal.h) --------------------------------------------------
StagePipe::~StagePipe() {
  for (hipEvent_t e : landed_)
    if (e) (void)hipEventDestroy(e);
}

void StagePipe::fail(int rc) {
  std::lock_guard<std::mutex> lk(mu_);
  if (!err_) {
    err_ = rc;
    err_msg_ = zt_last_error_message();
  }
  cv_.notify_all();
}

bool StagePipe::stopped() {
  std::lock_guard<std::mutex> lk(mu_);
  return err_ != 0;
}

bool StagePipe::wait(const size_t &counter, size_t i) {
  std::unique_lock<std::mutex> lk(mu_);
  cv_.wait(lk, [&] { return counter > i || err_; });
  return err_ == 0;
}

void StagePipe::done(size_t &counter, size_t i) {
  std::lock_guard<std::mutex> lk(mu_);
  counter = i + 1;
  cv_.notify_all();
}

int StagePipe::run(const Stage &up, const Stage &compute, const Stage &dn) {
  DeviceCtx *c = c_;
  if (!c->up) ZT_HIP(hipStreamCreateWithFlags(&c->up, hipStreamNonBlocking));
  if (!c->dn) ZT_HIP(hipStreamCreateWithFlags(&c->dn, hipStreamNonBlocking));
  landed_.assign(np_, nullptr);
  for (auto &e : landed_) ZT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  const int dev = c->phys;
  // the copy stages, each on its own thread (a stopped pipeline ends them)
  auto up_thread = [&]() -> int {
    ZT_HIP(hipSetDevice(dev));
    for (size_t i = 0; i < np_ && !stopped(); ++i) {
      ZT_TRY(up(i));
      ZT_HIP(hipEventRecord(landed_[i], c->up));
      done(uploaded_, i);
    }
    return ZT_OK;
  };
  auto dn_thread = [&]() -> int {
    ZT_HIP(hipSetDevice(dev));
    for (size_t i = 0; i < np_ && wait(computed_, i); ++i) {
      ZT_TRY(dn(i));
      done(downloaded_, i);
    }
    return ZT_OK;
  };
  std::thread tu([&] {
    if (int rc = up_thread()) fail(rc);
  });
  std::thread td([&] {
    if (int rc = dn_thread()) fail(rc);
  });
  // stage 2 on the caller's thread: compute(i) after piece i has landed
  for (size_t i = 0; i < np_ && wait(uploaded_, i); ++i) {
    int rc = hipStreamWaitEvent(c->stream, landed_[i], 0) == hipSuccess ? ZT_OK
                                                                        : set_error(ZT_E_HIP, "hipStreamWaitEvent");
    if (!rc) rc = compute(i);
    if (rc) {
      fail(rc);
      break;
    }
    done(computed_, i);
  }
  tu.join();
  td.join();
  if (trace) trace("joined");
  // nothing may still be copying into the output or out of the input when
  // the caller gets it back (error paths: zt_free / reuse right after)
  const hipError_t e1 = hipStreamSynchronize(c->up), e2 = hipStreamSynchronize(c->dn),
                   e3 = hipStreamSynchronize(c->aux), e4 = hipStreamSynchronize(c->stream);
  if (trace) trace("drained");
  if (err_) {
    (void)hipGetLastError();
    return set_error(err_, err_msg_);
  }
  if (e1 != hipSuccess) return hip_fail(e1, "pipeline upload stream");
  if (e2 != hipSuccess) return hip_fail(e2, "pipeline download stream");
  if (e3 != hipSuccess) return hip_fail(e3, "pipeline checksum stream");
  if (e4 != hipSuccess) return hip_fail(e4, "pipeline compute stream");
  return ZT_OK;
}

// pipeline_h2d_d2h (zt_internal.h) over StagePipe.
// ZT_PIPE_TIMING=1: per-piece stage timestamps on stderr (measurement only)
static bool pt_on() {
  static const bool on = getenv("ZT_PIPE_TIMING") != nullptr;
  return on;
}
#define PT(...) \
  if (pt_on()) fprintf(stderr, "[pipe %9.3f] " __VA_ARGS__)

int pipeline_h2d_d2h(DeviceCtx *c, size_t np, const std::function<PipePiece(size_t)> &input,
                     const std::function<int(size_t, const void **d_res, size_t *n_res)> &compute, PipeOut &out) {
  const double t_start = now_ms();
  uint8_t *stage[4];
  ZT_TRY(xfer_setup(c, stage, 4));
  // `drained[i]`: behind piece i's copy back (recorded from drain_from on)
  std::vector<hipEvent_t> drained(np, nullptr);
  struct EvFree {
    std::vector<hipEvent_t> &v;
    ~EvFree() {
      for (auto e : v)
        if (e) (void)hipEventDestroy(e);
    }
  } ev_free{drained};
  for (auto &e : drained) ZT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  std::vector<const void *> res(np, nullptr);
  std::vector<size_t> res_n(np, 0);
  StagePipe pipe(c, np);
  pipe.trace = [&](const char *what) { PT("%s\n", now_ms() - t_start, what); };
  // stage 1: host -> pinned chunk (host threads) -> device (DMA on c->up)
  size_t ku = 0;  // chunks issued
  auto up_stage = [&](size_t i) -> int {
    const PipePiece pc = input(i);
    const bool direct = host_direct(pc.h_src, pc.n);  // (a registered pool buffer: DMA from it)
    if (direct) {
      if (pc.n) ZT_HIP(hipMemcpyAsync(pc.d_dst, pc.h_src, pc.n, hipMemcpyHostToDevice, c->up));
    } else {
      ZT_TRY(staged_up(c->up, stage, c->xfer_ev, pc.d_dst, pc.h_src, pc.n, &ku));
    }
    PT("up %zu issued (%zu B, %s)\n", now_ms() - t_start, i, pc.n, direct ? "direct" : "staged");
    return ZT_OK;
  };
  // stage 3: device -> host: straight into a registered pool buffer (DMA on
  // c->dn), else device -> pinned chunk (DMA on c->dn) -> host (host threads)
  uint8_t *base = out.base;
  size_t cap = out.cap, total = 0, kd = 0;
  auto dn_stage = [&](size_t i) -> int {
    const size_t n = res_n[i];
    if (!base) {  // (the output's size estimate may look at piece 0's result)
      cap = std::max(out.cap_fn ? out.cap_fn() : (size_t)0, n);
      base = host_out(cap, true);
      if (!base) return set_error(ZT_E_NOMEM, "host allocation failed");
    }
    PT("dn %zu start (%zu B)\n", now_ms() - t_start, i, n);
    if (total + n > cap) {  // a larger buffer: the bytes so far move over
      PT("dn %zu grows the output %zu -> ...\n", now_ms() - t_start, i, cap);
      const size_t ncap = std::max(2 * cap, total + n + (total + n) / 4);
      uint8_t *nb = host_out(ncap, true);
      if (!nb) return set_error(ZT_E_NOMEM, "host allocation failed");
      ZT_HIP(hipStreamSynchronize(c->dn));
      host_copy(nb, base, total);
      host_discard(base);
      base = nb;
      cap = ncap;
    }
    if (host_direct(base + total, n)) {
      if (n) ZT_HIP(hipMemcpyAsync(base + total, res[i], n, hipMemcpyDeviceToHost, c->dn));
      PT("dn %zu direct\n", now_ms() - t_start, i);
    } else {
      PT("dn %zu staged\n", now_ms() - t_start, i);
      ZT_TRY(staged_down(c->dn, stage + 2, c->xfer_ev + 2, base + total, res[i], n, &kd));
    }
    total += n;
    if (i >= out.drain_from) ZT_HIP(hipEventRecord(drained[i], c->dn));
    return ZT_OK;
  };
  out.drain = [&](size_t j) -> int {
    if (j < out.drain_from) return set_error(ZT_E_INTERNAL, "pipeline: drain of a piece before drain_from");
    if (!pipe.wait_downloaded(j)) return set_error(ZT_E_INTERNAL, "pipeline stopped");
    ZT_HIP(hipStreamWaitEvent(c->stream, drained[j], 0));
    return ZT_OK;
  };
  const int rc = pipe.run(up_stage, [&](size_t i) -> int {
    PT("compute %zu start\n", now_ms() - t_start, i);
    const int r = compute(i, &res[i], &res_n[i]);
    PT("compute %zu done (%zu B)\n", now_ms() - t_start, i, res_n[i]);
    return r;
  }, dn_stage);
  out.drain = nullptr;
  out.base = base;
  out.cap = cap;
  out.total = total;
  return rc;
}

}  // namespace zt
