// host_mem.cpp -- host output memory: the bounded pool of large outputs, the
// batch calls' slabs, zt_free.
#include <sys/mman.h>

#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>

#include "zt_internal.h"

namespace zt {

// The single-buffer calls' large host outputs (zt_deflate_raw /
// zt_inflate_raw, >= 8 MiB) come from a bounded pool (a caching host
// allocator): zt_free returns such a buffer to the pool -- registered with
// HIP (hipHostRegister) on its first return, a one-time cost of that
// zt_free (~25 ms per GiB, pages past the written output faulted in) -- and
// the next output of a similar size reuses it, so downloads into it and
// uploads from it (a stream handed back to zt_inflate_raw) go by DMA with no
// pinned staging, host memcpy or page faults.  The free buffers the pool
// keeps are bounded by ZT_HOST_POOL_MB (default 4096; 0: no pool, every
// output freshly allocated); zt_release_scratch drops them.  The batch
// calls' slabs (slab_out: the GZip batch's framed members, the batch
// inflate's outputs) come from the pool too -- a slab returns once its last
// item is freed -- so a batch caller in a loop downloads by DMA straight
// into them (C2: 22.7 -> 15.7 ms per 4096 x 64 KiB).
static uint8_t *host_alloc(size_t n) {
  // 2 MiB-aligned and backed by transparent huge pages where the kernel
  // allows it -- 512x fewer first-touch faults while the download fills them
  void *p = nullptr;
  if (posix_memalign(&p, 2u << 20, n)) return nullptr;
  (void)madvise(p, n, MADV_HUGEPAGE);
  return (uint8_t *)p;
}

struct PoolBuf {
  uint8_t *p;
  size_t cap;
  size_t len;      // bytes the current use returns (host_out_used; default: the request)
  size_t hi;       // the most any use returned: the pages ever touched
  size_t reg_len;  // registered prefix (hipHostRegister of [p, p + reg_len)), 0: none
  bool used;
  bool reg_bad;    // registration failed once: not tried again
};
static std::mutex g_pool_mu;
static std::vector<PoolBuf> g_pool;

static size_t pool_limit() {
  static const size_t v = [] {
    const char *e = getenv("ZT_HOST_POOL_MB");
    return e ? (size_t)strtoull(e, nullptr, 10) << 20 : (size_t)4096 << 20;
  }();
  return v;
}

// resident bytes of a free pool buffer: the pages its uses touched
static size_t pool_resident(const PoolBuf &e) { return std::max(e.hi, e.reg_len); }

// free pool buffers beyond the bound, largest first (g_pool_mu held)
static void pool_trim(size_t limit) {
  for (;;) {
    size_t free_bytes = 0, big = SIZE_MAX;
    for (size_t i = 0; i < g_pool.size(); ++i)
      if (!g_pool[i].used) {
        free_bytes += pool_resident(g_pool[i]);
        if (big == SIZE_MAX || pool_resident(g_pool[i]) > pool_resident(g_pool[big])) big = i;
      }
    if (big == SIZE_MAX || (limit && free_bytes <= limit)) return;  // (limit 0: all of them)
    if (g_pool[big].reg_len) (void)hipHostUnregister(g_pool[big].p);
    free(g_pool[big].p);
    g_pool.erase(g_pool.begin() + (long)big);
  }
}

void host_pool_drop() {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  pool_trim(0);
}

uint8_t *host_out(size_t n, bool pool) {
  if (n < (8u << 20)) return (uint8_t *)malloc(n ? n : 1);
  if (!pool || !pool_limit()) return host_alloc(n);
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    size_t best = SIZE_MAX;
    for (size_t i = 0; i < g_pool.size(); ++i) {
      const PoolBuf &e = g_pool[i];
      if (!e.used && e.cap >= n && e.cap / 2 <= n && (best == SIZE_MAX || e.cap < g_pool[best].cap)) best = i;
    }
    if (best != SIZE_MAX) {
      g_pool[best].used = true;
      g_pool[best].len = n;
      return g_pool[best].p;
    }
  }
  uint8_t *p = host_alloc(n);
  if (!p) return nullptr;
  std::lock_guard<std::mutex> lk(g_pool_mu);
  g_pool.push_back(PoolBuf{p, n, n, 0, 0, true, false});
  return p;
}

void host_out_used(void *p, size_t n) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (PoolBuf &e : g_pool)
    if (e.p == p && e.used) e.len = std::min(n, e.cap);
}

// A pool buffer back to the pool (false: p is not one).  The pages its uses
// returned are registered with HIP on the way in -- not its whole capacity
// (a pipelined inflate's buffer is sized for several times its input), and
// outside g_pool_mu (~25 ms per GiB): the buffer stays `used` meanwhile, so
// no other thread takes or trims it, and other threads' host_out / zt_free
// go on.
static bool pool_release(void *p) {
  std::unique_lock<std::mutex> lk(g_pool_mu);
  PoolBuf *e = nullptr;
  for (PoolBuf &x : g_pool)
    if (x.p == p && x.used) e = &x;
  if (!e) return false;
  e->hi = std::max(e->hi, e->len);
  const size_t want = std::min(e->cap, (e->hi + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1));
  if (!e->reg_bad && want > e->reg_len) {
    uint8_t *bp = e->p;
    const size_t old = e->reg_len;
    lk.unlock();
    if (old) (void)hipHostUnregister(bp);
    const bool ok = hipHostRegister(bp, want, hipHostRegisterPortable) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    lk.lock();
    for (PoolBuf &x : g_pool)
      if (x.p == bp) {
        x.reg_len = ok ? want : 0;
        x.reg_bad = !ok;
        x.used = false;
      }
  } else {
    e->used = false;
  }
  pool_trim(pool_limit());
  return true;
}

void host_release(void *p) {
  if (!pool_release(p)) free(p);
}

void host_discard(void *p) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); ++i)
      if (g_pool[i].p == p && g_pool[i].used) {
        if (g_pool[i].reg_len) (void)hipHostUnregister(p);
        g_pool.erase(g_pool.begin() + (long)i);
        break;
      }
  }
  free(p);
}

bool host_direct(const void *p, size_t n) {
  const uint8_t *q = static_cast<const uint8_t *>(p);
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (const PoolBuf &e : g_pool)
    if (e.used && e.reg_len && q >= e.p && q + n <= e.p + e.reg_len) return true;
  return false;
}

// Batch outputs share one host allocation (a slab, on huge pages when large):
// one allocation and one stream of first-touch faults instead of one per
// item (4096 x 64 KiB outputs: 21 ms of faults in the copy-out).  Each item
// pointer is still released by zt_free; the slab goes with its last item.
struct Slab {
  size_t size;
  size_t refs;
};
static std::mutex g_slab_mu;
static std::map<uintptr_t, Slab> g_slabs;

uint8_t *slab_out(size_t total, size_t items, bool pool) {
  if (total == 0) total = 1;
  uint8_t *b = host_out(total, pool);
  if (!b) return nullptr;
  std::lock_guard<std::mutex> lk(g_slab_mu);
  g_slabs[(uintptr_t)b] = Slab{total, items};
  return b;
}

bool slab_release(void *p) {
  std::lock_guard<std::mutex> lk(g_slab_mu);
  if (g_slabs.empty()) return false;
  auto it = g_slabs.upper_bound((uintptr_t)p);
  if (it == g_slabs.begin()) return false;
  --it;
  if ((uintptr_t)p >= it->first + it->second.size) return false;
  if (--it->second.refs == 0) {
    host_release(reinterpret_cast<void *>(it->first));
    g_slabs.erase(it);
  }
  return true;
}

}  // namespace zt

extern "C" void zt_free(void *p) {
  if (!p) return;
  if (zt::slab_release(p)) return;
  zt::host_release(p);
}
