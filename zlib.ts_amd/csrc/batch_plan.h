// batch_plan.h -- the arithmetic of the host batch layer, no HIP: how a batch
// is split over devices, laid out in staging, cut into upload chunks and
// pipeline groups, the output bounds of a deflate call, the option resolver,
// and the thread fan-out that collects each share's code and message.  Pure
// functions, checked on the CPU by tools/batch_plan_check.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/zt.h"
#include "inflate_chain.h"  // align_up
#include "member_frame.h"   // stored_len

namespace zt {

static_assert(std::is_same<size_t, uint64_t>::value, "item offsets go to the launchers as uint64_t");

inline std::vector<size_t> iota_ids(size_t count) {
  std::vector<size_t> v(count);
  for (size_t i = 0; i < count; ++i) v[i] = i;
  return v;
}

// ---- splits over devices ------------------------------------------------------
// Longest processing time: largest item first onto the least loaded of nd
// devices (cost n[i] + 4096 per item, ties in index order), each share
// ascending.  nd == 1: the identity.
inline std::vector<std::vector<size_t>> lpt_shares(const size_t *n, size_t count, size_t nd) {
  std::vector<std::vector<size_t>> share(nd);
  if (nd == 1) {
    share[0] = iota_ids(count);
    return share;
  }
  std::vector<size_t> order = iota_ids(count);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return n[a] > n[b]; });
  std::vector<uint64_t> load(nd, 0);
  for (size_t i : order) {
    const size_t d = (size_t)(std::min_element(load.begin(), load.end()) - load.begin());
    share[d].push_back(i);
    load[d] += n[i] + 4096;  // + per-item cost
  }
  for (auto &v : share) std::sort(v.begin(), v.end());
  return share;
}

// Contiguous shares of about equal bytes (cost n[i] + 256): device d takes
// items [cut[d], cut[d + 1]); a share may be empty.
inline std::vector<size_t> contiguous_cuts(const size_t *n, size_t count, size_t nd) {
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
  return cut;
}

// ---- staging layout -----------------------------------------------------------
// Items `ids` one after the other, item k at off[k], each taking
// max(n, min_len) bytes rounded up to `align`.  (256, 1) on the inflate
// side, 32768 (the deflate pipeline's block) on the deflate side.
struct PackLayout {
  std::vector<size_t> off;
  size_t total = 0;
};
inline PackLayout pack_layout(const size_t *n, const std::vector<size_t> &ids, size_t align, size_t min_len) {
  PackLayout L;
  L.off.resize(ids.size());
  for (size_t k = 0; k < ids.size(); ++k) {
    L.off[k] = L.total;
    L.total += align_up(std::max(n[ids[k]], min_len), align);
  }
  return L;
}

// Runs [r[j], r[j + 1]) of items for a chunked upload: a run ends with the
// first item that brings it to `chunk` bytes (so a run holds at least one
// item and less than `chunk` bytes before its last).
inline std::vector<size_t> chunk_runs(const std::vector<size_t> &off, size_t total, size_t chunk) {
  (void)total;
  const size_t m = off.size();
  std::vector<size_t> r{0};
  for (size_t a = 0; a < m;) {
    size_t b = a + 1;
    while (b < m && off[b] - off[a] < chunk) ++b;
    r.push_back(b);
    a = b;
  }
  return r;
}

// Groups [g[j], g[j + 1]) of a grouped batch: a group ends once it holds
// `target` bytes, the last one takes what is left (never empty).
inline std::vector<size_t> group_cuts(const std::vector<size_t> &off, size_t m, uint64_t padded, uint64_t target) {
  (void)padded;
  std::vector<size_t> gk{0};
  for (size_t k = 0; k < m; ++k)
    if (k + 1 < m && off[k + 1] - off[gk.back()] >= target) gk.push_back(k + 1);
  gk.push_back(m);
  return gk;
}

// ---- sizes --------------------------------------------------------------------
// Output bound of one deflate call; pipeline_bound = deflate_bound_bytes(n)
inline size_t deflate_out_bound(int ctype, size_t n, size_t pipeline_bound) {
  if (ctype == 0) return stored_len(n) + 16;
  return pipeline_bound + (ctype == 1 ? n / 8 + 64 : 0);
}
// Output bound of a batch pipeline over `padded` bytes of 32 KiB-aligned
// items, rounded up to `round` (a power of two; 256 for a group's region)
inline uint64_t batch_out_bound(uint64_t padded, uint64_t round = 1) {
  return (padded + padded / 8 + 1024 * (padded / 32768 + 1) + 4096 + (round - 1)) & ~(round - 1);
}
// An item's room in a slab of framed members: >= 1 byte more than the member, 64-aligned
inline size_t slab_stride(size_t prefix, size_t body, size_t trailer) {
  return (prefix + body + trailer + 64) & ~size_t(63);
}

// ---- options ------------------------------------------------------------------
// compression type and level of a call (null opts: dynamic codes, level 6);
// ZT_E_INVALID_COMPRESSION_TYPE for a type outside 0..2 (the caller sets the message)
inline int resolve_deflate_opts(const zt_deflate_opts *o, int *ctype, int *level) {
  int ct = o ? o->compression_type : 2;
  int lv = o ? o->level : -1;
  if (ct < 0 || ct > 2) return ZT_E_INVALID_COMPRESSION_TYPE;
  if (lv < 0 || lv > 9) lv = 6;
  if (lv == 0) ct = 0;
  // the reference's `lazy` option asks for deferred matching: use the lazy parse
  if (o && o->lazy > 0 && lv < 4) lv = 4;
  *ctype = ct;
  *level = lv;
  return ZT_OK;
}

// ---- fan-out ------------------------------------------------------------------
struct ShareResult {
  int code = ZT_OK;
  std::string msg;
};
// run(d) for every non-empty share d: on the caller's thread when there is
// one share, else each on a thread of its own.  A share's message is read
// once, on its thread, after run returns a code: last_message() is that
// thread's error text.
template <class Run, class Msg>
std::vector<ShareResult> fan_out(const std::vector<std::vector<size_t>> &shares, const Run &run,
                                 const Msg &last_message) {
  std::vector<ShareResult> res(shares.size());
  auto one = [&](size_t d) {
    res[d].code = run(d);
    if (res[d].code) res[d].msg = last_message();
  };
  if (shares.size() == 1) {
    one(0);
    return res;
  }
  std::vector<std::thread> th;
  for (size_t d = 0; d < shares.size(); ++d)
    if (!shares[d].empty()) th.emplace_back(one, d);
  for (auto &t : th) t.join();
  return res;
}

}  // namespace zt
