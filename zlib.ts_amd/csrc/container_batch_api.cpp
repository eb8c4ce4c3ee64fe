// container_batch_api.cpp -- the read side of the batched containers
// (include/zt_container_batch.h): zt_gunzip_batch, zt_zlib_decompress_batch
// and zt_zlib_decompress_batch_dict.
//
// Per device share, one pipeline: the items are packed at 256-byte offsets
// and uploaded once (chunked, as inflate_host_batch does).  GZip: find_members
// (container.hip) lists every position where 1F 8B 08 starts; every candidate
// whose header parses is decoded in one call of the batch decoder, its input
// bounded by the item's next candidate + a slack (64 KiB, less where the
// candidates lie dense: gunzip_chain.h) so that scratch stays proportional
// to the packed input; the CRC-32 of every output is taken from
// its device copy behind the decode; the host then walks each item's chain
// from offset 0 (gunzip_chain.h), which drops the candidates that lie inside
// data, comments or FEXTRA.  A start the chain needs that was not decoded (a
// truncated list: it goes into the next pass with the candidates a host scan
// finds behind it) and a member that did not settle inside its bound (decoded
// again with 8 times the input, at the latest to the item's end) make a
// further pass; every pass advances every unfinished chain.  Only a member
// of the chain that fails at the item's end is decoded once more by one wave
// for the reference's exact status: speculative streams never are.  zlib: one
// stream per item from index[i], no scan; items with FDICT decode with the
// dictionary on the one-wave path, the others on the normal path, and the
// Adler-32 comes from the device copy when `verify` is set.
// Replaces a loop of new GUnzip(input).decompress() (src/GUnzip.ts:53-175)
// and of new Inflate(input, {index, verify}).decompress() (src/Inflate.ts:34-93).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/zt_container_batch.h"
#include "gunzip_chain.h"
#include "zt_internal.h"

namespace zt {

namespace {

thread_local std::vector<std::string> t_msgs;
thread_local zt_gunzip_batch_stats t_stats = {0, 0, 0, 0, 0};

// (a decode call that fails as a whole -- device memory, HIP -- leaves kNotRun)
constexpr int kNotRun = -0x7FFF;

// library outputs not handed to the caller are released on every return
struct Outputs {
  std::vector<uint8_t *> p;
  ~Outputs() {
    for (uint8_t *q : p) zt_free(q);
  }
  uint8_t *take(size_t slot) {
    uint8_t *q = p[slot];
    p[slot] = nullptr;
    return q;
  }
  void drop(size_t slot) { zt_free(take(slot)); }
};

// this thread's message for a decoder status
std::string inflate_message(int status, int detail) {
  inflate_error(status, detail);
  return zt_last_error_message();
}

// items `ids` packed at 256-byte offsets into scratch slot kIn, uploaded in
// chunks as they are packed
int pack_in(DeviceCtx *c, const uint8_t *const *in, const size_t *n, const std::vector<size_t> &ids,
            std::vector<size_t> &in_off, size_t *total, void **d_in) {
  PackLayout L = pack_layout(n, ids, 256, 1);
  ZT_TRY(pack_upload(c, in, n, ids, L, PackMode{false, true}, d_in));
  in_off.swap(L.off);
  *total = L.total;
  return ZT_OK;
}

// ---- gzip -------------------------------------------------------------------------
struct GunzipArgs {
  const uint8_t *const *in;
  const size_t *n;
  uint8_t **out;
  size_t *out_len;
  zt_gzip_member **members;
  size_t *nmembers;
  int *status;
  std::string *msgs;
};

int gunzip_share_locked(DeviceCtx *c, const GunzipArgs &A, const std::vector<size_t> &ids,
                        zt_gunzip_batch_stats *st) {
  const size_t m = ids.size();
  std::vector<size_t> in_off;
  size_t total = 0;
  void *d_in;
  ZT_TRY(pack_in(c, A.in, A.n, ids, in_off, &total, &d_in));
  // candidates: the list's capacity is proportional to the packed input (one
  // per item and per 256 bytes; gz_slack keeps the decode scratch in proportion)
  const uint32_t cap = (uint32_t)std::min<size_t>(m + total / 256, 0x7FFFFFFFu);
  uint64_t *d_ioff = nullptr, *d_ilen = nullptr;
  MemberCand *d_list = nullptr;
  uint32_t *d_found = nullptr;
  ZT_TRY(scratch_carved(c, kContainerIn, [&](void *base) {
    Carve cv(base);
    d_ioff = cv.take<uint64_t>(m);
    d_ilen = cv.take<uint64_t>(m);
    d_list = cv.take<MemberCand>(cap);
    d_found = cv.take<uint32_t>(1);
    return cv.bytes();
  }));
  std::vector<uint64_t> ioff(m), ilen(m);
  for (size_t k = 0; k < m; ++k) {
    ioff[k] = in_off[k];
    ilen[k] = A.n[ids[k]];
  }
  ZT_HIP(hipMemcpyAsync(d_ioff, ioff.data(), m * 8, hipMemcpyHostToDevice, c->stream));
  ZT_HIP(hipMemcpyAsync(d_ilen, ilen.data(), m * 8, hipMemcpyHostToDevice, c->stream));
  ZT_TRY(find_members_dev(static_cast<const uint8_t *>(d_in), total, d_ioff, d_ilen, (uint32_t)m, d_list, cap, d_found,
                          c->stream));
  uint32_t found = 0;
  ZT_TRY(readback(c, &found, d_found, sizeof found, c->stream));
  std::vector<MemberCand> list(std::min(found, cap));
  if (!list.empty()) ZT_TRY(readback(c, list.data(), d_list, list.size() * sizeof(MemberCand), c->stream));
  // per item, sorted; offset 0 is a start whatever it holds
  std::vector<std::vector<size_t>> cands(m);
  for (size_t k = 0; k < m; ++k)
    if (ilen[k]) {
      cands[k].push_back(0);
      st->candidates++;
    }
  st->candidates += found;
  for (const MemberCand &q : list) {
    if (q.item >= m || q.off == 0 || q.off + 3 > ilen[q.item]) return set_error(ZT_E_INTERNAL, "find_members: bad entry");
    cands[q.item].push_back((size_t)q.off);
  }
  for (auto &v : cands) std::sort(v.begin(), v.end());

  // a member to decode: with the bound of its candidates (bound 0), or again
  // with this wider one; exact: with the decoder's own status when it fails
  // (one more decode by one wave, which only the chain's own members are worth)
  struct Req {
    size_t k, start, bound;
    bool exact;
  };
  std::vector<Req> reqs;
  for (size_t k = 0; k < m; ++k)
    for (size_t s : cands[k]) reqs.push_back(Req{k, s, 0, false});
  std::vector<std::vector<GzDecoded>> table(m);
  std::vector<GzWalk> walk(m);
  Outputs outs;
  for (uint64_t pass = 0;; ++pass) {
    // the pass's streams: requests whose header parses (the walk reports the
    // header errors of the starts its chain reaches)
    std::vector<Req> run;
    std::vector<size_t> s_off, s_n, s_idx;
    std::vector<uint8_t> s_spec;
    for (const Req &q : reqs) {
      const size_t i = ids[q.k];
      zt_gzip_member hm;
      GzError ge;
      size_t body = 0;
      if (gzip_parse_header(A.in[i], A.n[i], q.start, &hm, &body, &ge, false)) continue;
      run.push_back(q);
      s_off.push_back(in_off[q.k]);
      s_n.push_back(q.bound ? q.bound
                            : std::max(body, gz_bound(cands[q.k], q.start, A.n[i],
                                                      gz_slack(A.n[i], cands[q.k].size()))));
      s_spec.push_back(q.exact ? 0 : 1);
      s_idx.push_back(body);
    }
    if (!run.empty()) {
      const size_t r = run.size();
      std::vector<uint8_t *> o(r, nullptr);
      std::vector<size_t> ol(r, 0), eip(r, 0);
      std::vector<int> sst(r, kNotRun), det(r, 0);
      std::vector<uint32_t> sums(2 * r, 0);
      BatchExtras ex;
      ex.sums = sums.data();
      ex.detail = det.data();
      ex.speculative = s_spec.data();
      const int rc = inflate_batch_dev_streams_ex(c, d_in, s_off, s_n.data(), s_idx.data(), r, o.data(), ol.data(),
                                                  eip.data(), sst.data(), nullptr, 0, &ex);
      bool ran = true;
      for (size_t j = 0; j < r; ++j) {
        outs.p.push_back(o[j]);
        if (sst[j] == kNotRun) ran = false;
      }
      if (!ran) return rc ? rc : set_error(ZT_E_INTERNAL, "gunzip batch: members not decoded");
      st->decode_passes++;
      if (pass) st->redecoded += r;
      for (size_t j = 0; j < r; ++j) {
        GzDecoded d;
        d.start = run[j].start;
        d.bound = s_n[j];
        d.status = sst[j];
        d.detail = det[j];
        d.end_ip = eip[j];
        d.out_len = ol[j];
        d.crc = sums[2 * j];
        d.slot = outs.p.size() - r + j;
        d.exact = run[j].exact;
        std::vector<GzDecoded> &t = table[run[j].k];
        auto it = std::lower_bound(t.begin(), t.end(), d.start,
                                   [](const GzDecoded &a, size_t v) { return a.start < v; });
        if (it != t.end() && it->start == d.start) {  // decoded again: the earlier output goes
          outs.drop(it->slot);
          *it = d;
        } else {
          t.insert(it, d);
        }
      }
    }
    reqs.clear();
    for (size_t k = 0; k < m; ++k) {
      GzWalk &w = walk[k];
      if (w.state == GZ_DONE || w.state == GZ_FAILED) continue;
      const bool had = w.state == GZ_NEED;
      const size_t was_start = w.need_start, was_bound = w.need_bound;
      const bool was_full = w.need_full, was_exact = w.need_exact;
      const size_t n_k = A.n[ids[k]];
      if (gz_walk(A.in[ids[k]], n_k, table[k], &w) == GZ_NEED) {
        if (had && was_start == w.need_start && was_full == w.need_full && was_bound == w.need_bound &&
            was_exact == w.need_exact)
          return set_error(ZT_E_INTERNAL, "gunzip batch: a chain did not advance");
        // (a member that did not settle: 8 times the input it had, at the
        // item's end with the decoder's own status)
        const size_t wider = w.need_full ? gz_wider(w.need_start, w.need_bound, n_k) : 0;
        reqs.push_back(Req{k, w.need_start, wider, w.need_full && wider >= n_k});
        if (!w.need_full) {
          // a start that was not in the list (truncated: more candidates than
          // its capacity): the host scans on from it for the next candidates,
          // twice as many every pass, so a long chain takes few passes
          std::vector<size_t> more;
          gz_scan(A.in[ids[k]], A.n[ids[k]], w.need_start, (size_t)32 << std::min<uint64_t>(pass, 12), &more);
          std::vector<size_t> &cv = cands[k];
          const auto self = std::lower_bound(cv.begin(), cv.end(), w.need_start);
          if (self == cv.end() || *self != w.need_start) cv.insert(self, w.need_start);
          for (size_t s : more) {
            const auto at = std::lower_bound(cv.begin(), cv.end(), s);
            if (at != cv.end() && *at == s) continue;  // (decoded in the first pass)
            cv.insert(at, s);
            reqs.push_back(Req{k, s, 0, false});
          }
        }
      }
    }
    if (reqs.empty()) break;
  }
  // outputs: a single member keeps the decoder's buffer; several are joined,
  // by one parallel copy for the whole share, into one pooled slab (one
  // buffer of a steady size per call: many pooled buffers of varying sizes
  // push the decoder's own slab out of the bounded pool)
  std::vector<uint8_t *> joined(m, nullptr);
  struct Piece {
    uint8_t *dst;
    const uint8_t *src;
    size_t len;
  };
  std::vector<Piece> pieces;
  size_t piece_bytes = 0, join_total = 0, join_items = 0;
  std::vector<size_t> join_off(m, 0);
  for (size_t k = 0; k < m; ++k) {
    const GzWalk &w = walk[k];
    if (w.state == GZ_FAILED || w.members.size() < 2) continue;
    join_off[k] = join_total;
    join_total += slab_stride(0, w.total, 0);  // (>= 1 byte each: every pointer distinct)
    ++join_items;
  }
  uint8_t *jslab = join_items ? slab_out(join_total, join_items, true) : nullptr;
  if (join_items && !jslab) return set_error(ZT_E_NOMEM, "host allocation failed");
  for (size_t k = 0; k < m; ++k) {
    const GzWalk &w = walk[k];
    if (w.state == GZ_FAILED || w.members.size() == 1) continue;
    if (w.members.empty()) {
      joined[k] = host_out(0);
      if (!joined[k]) {
        for (uint8_t *q : joined) zt_free(q);
        return set_error(ZT_E_NOMEM, "host allocation failed");
      }
      continue;
    }
    joined[k] = jslab + join_off[k];
    for (size_t q = 0; q < w.members.size(); ++q)
      if (w.members[q].data_len) {
        pieces.push_back(Piece{joined[k] + w.members[q].data_off, outs.p[w.slots[q]], w.members[q].data_len});
        piece_bytes += w.members[q].data_len;
      }
  }
  parallel_copy(pieces.size(), [&](size_t j) { memcpy(pieces[j].dst, pieces[j].src, pieces[j].len); }, piece_bytes);
  for (size_t k = 0; k < m; ++k) {
    const size_t i = ids[k];
    GzWalk &w = walk[k];
    if (w.state == GZ_FAILED) {
      A.status[i] = w.err.code;
      A.msgs[i] = w.err.msg[0] ? std::string(w.err.msg) : inflate_message(w.err.code, w.detail);
      continue;
    }
    const size_t nm = w.members.size();
    uint8_t *h = nm == 1 ? outs.take(w.slots[0]) : joined[k];
    joined[k] = nullptr;
    if (A.members) {
      zt_gzip_member *mm = (zt_gzip_member *)malloc((nm ? nm : 1) * sizeof(zt_gzip_member));
      if (!mm) {
        zt_free(h);
        for (uint8_t *q : joined) zt_free(q);
        return set_error(ZT_E_NOMEM, "host allocation failed");
      }
      if (nm) memcpy(mm, w.members.data(), nm * sizeof(zt_gzip_member));
      A.members[i] = mm;
    }
    if (A.nmembers) A.nmembers[i] = nm;
    A.out[i] = h;
    A.out_len[i] = w.total;
    A.status[i] = ZT_OK;
    st->members += nm;
  }
  return ZT_OK;
}

// ---- zlib -------------------------------------------------------------------------
struct ZlibArgs {
  const uint8_t *const *in;
  const size_t *n;
  const size_t *index;
  int verify;
  const uint8_t *dict;
  size_t dict_len;
  uint32_t dictid;  // Adler-32 of the dictionary
  uint8_t **out;
  size_t *out_len;
  size_t *end_ip;
  uint32_t *adler_out;
  int *status;
  std::string *msgs;
};

int zlib_share_locked(DeviceCtx *c, const ZlibArgs &A, const std::vector<size_t> &ids) {
  const size_t m = ids.size();
  // headers: the checks of zt_zlib_decompress / zt_zlib_decompress_dict, in their order
  std::vector<size_t> part[2];  // local items without / with FDICT
  std::vector<size_t> body(m, 0);
  for (size_t k = 0; k < m; ++k) {
    const size_t i = ids[k];
    auto fail = [&](int code, const std::string &msg) {
      A.status[i] = code;
      A.msgs[i] = msg;
    };
    ZlibHeader h;
    const ZlibHdr hs = zlib_parse_header(A.in[i], A.n[i], A.index ? A.index[i] : 0, &h);
    int code;
    std::string hmsg;
    if (zlib_header_status(hs, h, &code, &hmsg)) {
      fail(code, hmsg);
    } else if (h.fdict && A.dict_len == 0) {
      fail(ZT_E_ZLIB_FDICT, "fdict flag is not supported");
    } else if (hs == ZH_BROKEN) {
      fail(ZT_E_INPUT_BROKEN, "input buffer is broken");
    } else if (h.fdict && h.dictid != A.dictid) {
      char msg[96];
      snprintf(msg, sizeof msg, "invalid dictionary id: 0x%x / 0x%x", h.dictid, A.dictid);
      fail(ZT_E_ZLIB_DICTID, msg);
    } else {
      body[k] = h.body;
      part[h.fdict ? 1 : 0].push_back(k);
    }
  }
  if (part[0].empty() && part[1].empty()) return ZT_OK;
  std::vector<size_t> in_off;
  size_t total = 0;
  void *d_in;
  ZT_TRY(pack_in(c, A.in, A.n, ids, in_off, &total, &d_in));
  const uint8_t *d_hist = nullptr;
  uint32_t wlen = 0;
  if (!part[1].empty()) {  // this device's copy of the dictionary's window
    wlen = dict_window_len(A.dict_len);
    void *p;
    ZT_TRY(scratch(c, kDict, wlen, &p));
    ZT_HIP(hipMemcpyAsync(p, A.dict + dict_window_off(A.dict_len), wlen, hipMemcpyHostToDevice, c->stream));
    ZT_HIP(hipStreamSynchronize(c->stream));
    d_hist = static_cast<const uint8_t *>(p);
  }
  for (int fd = 0; fd < 2; ++fd) {
    const std::vector<size_t> &ks = part[fd];
    const size_t r = ks.size();
    if (!r) continue;
    std::vector<size_t> s_off(r), s_n(r), s_idx(r), ol(r, 0), eip(r, 0);
    std::vector<uint8_t *> o(r, nullptr);
    std::vector<int> sst(r, kNotRun), det(r, 0);
    std::vector<uint32_t> sums(A.verify ? 2 * r : 0, 0);
    for (size_t j = 0; j < r; ++j) {
      s_off[j] = in_off[ks[j]];
      s_n[j] = A.n[ids[ks[j]]];
      s_idx[j] = body[ks[j]];
    }
    BatchExtras ex;
    ex.sums = A.verify ? sums.data() : nullptr;
    ex.detail = det.data();
    const int rc = inflate_batch_dev_streams_ex(c, d_in, s_off, s_n.data(), s_idx.data(), r, o.data(), ol.data(),
                                                eip.data(), sst.data(), fd ? d_hist : nullptr, fd ? wlen : 0, &ex);
    Outputs outs;
    outs.p = o;
    for (size_t j = 0; j < r; ++j)
      if (sst[j] == kNotRun) return rc ? rc : set_error(ZT_E_INTERNAL, "zlib batch: streams not decoded");
    for (size_t j = 0; j < r; ++j) {
      const size_t i = ids[ks[j]];
      if (sst[j]) {
        A.status[i] = sst[j];
        A.msgs[i] = inflate_message(sst[j], det[j]);
        continue;
      }
      uint32_t adler = 1;
      if (A.verify) {  // src/Inflate.ts:80-90
        adler = sums[2 * j + 1];
        Reader t{A.in[i], A.n[i], eip[j]};
        uint32_t want = 0;
        for (int q = 0; q < 4; ++q) want = (want << 8) | t.u8();
        if (adler != want) {
          A.status[i] = ZT_E_ZLIB_ADLER;
          A.msgs[i] = "invalid adler-32 checksum";
          continue;
        }
      }
      A.out[i] = outs.take(j);
      A.out_len[i] = ol[j];
      if (A.end_ip) A.end_ip[i] = eip[j];
      if (A.adler_out) A.adler_out[i] = adler;
      A.status[i] = ZT_OK;
    }
  }
  return ZT_OK;
}

// ---- devices ----------------------------------------------------------------------
// Items split over the batch devices by longest processing time; share(dev
// index, device context, ids) runs under for_each_device.  A share that fails
// as a whole gives its code and message to each of its items.
template <class Share>
void run_shares(const size_t *n, size_t count, int *status, std::string *msgs, const Share &share) {
  const std::vector<int> devs = fanout_devices(count);
  const std::vector<std::vector<size_t>> ids = lpt_shares(n, count, devs.size());
  const std::vector<ShareResult> res = for_each_device(devs, ids, share);
  for (size_t d = 0; d < ids.size(); ++d)
    if (res[d].code)
      for (size_t i : ids[d]) {
        status[i] = res[d].code;
        msgs[i] = res[d].msg;
      }
}

// first failing item's code with its message set; this thread's messages
int finish(size_t count, const int *status, std::vector<std::string> &msgs) {
  int first = ZT_OK;
  for (size_t i = 0; i < count && first == ZT_OK; ++i)
    if (status[i]) first = set_error(status[i], msgs[i]);
  t_msgs.swap(msgs);
  return first;
}

int zlib_batch(const uint8_t *const *in, const size_t *n, const size_t *index, size_t count, int verify,
               const uint8_t *dict, size_t dict_len, uint8_t **out, size_t *out_len, size_t *end_ip,
               uint32_t *adler_out, int *status) {
  t_msgs.clear();
  if (count == 0) return ZT_OK;
  if (!in || !n || !out || !out_len || !status || (dict_len && !dict)) return set_error(ZT_E_ARG, "null argument");
  for (size_t i = 0; i < count; ++i)
    if (n[i] && !in[i]) return set_error(ZT_E_ARG, "null input");
  for (size_t i = 0; i < count; ++i) {
    out[i] = nullptr;
    out_len[i] = 0;
    status[i] = ZT_OK;
    if (end_ip) end_ip[i] = 0;
    if (adler_out) adler_out[i] = 1;
  }
  uint32_t dictid = 1;
  if (dict_len) ZT_TRY(zt_adler32_update(1, dict, dict_len, &dictid));  // (the checksum kernel, over the whole dictionary)
  std::vector<std::string> msgs(count);
  const ZlibArgs A{in, n, index, verify, dict, dict_len, dictid, out, out_len, end_ip, adler_out, status, msgs.data()};
  run_shares(n, count, status, msgs.data(), [&](size_t, DeviceCtx *c, const std::vector<size_t> &ids) {
    const int rc = zlib_share_locked(c, A, ids);
    if (rc)  // (the share failed as a whole: nothing of it is handed out)
      for (size_t i : ids) {
        zt_free(out[i]);
        out[i] = nullptr;
        out_len[i] = 0;
      }
    return rc;
  });
  return finish(count, status, msgs);
}

}  // namespace

}  // namespace zt

using namespace zt;

extern "C" {

int zt_gunzip_batch(const uint8_t *const *in, const size_t *n, size_t count, uint8_t **out, size_t *out_len,
                    zt_gzip_member **members, size_t *nmembers, int *status) {
  t_msgs.clear();
  t_stats = zt_gunzip_batch_stats{count, 0, 0, 0, 0};
  if (count == 0) return ZT_OK;
  if (!in || !n || !out || !out_len || !status) return set_error(ZT_E_ARG, "null argument");
  for (size_t i = 0; i < count; ++i)
    if (n[i] && !in[i]) return set_error(ZT_E_ARG, "null input");
  for (size_t i = 0; i < count; ++i) {
    out[i] = nullptr;
    out_len[i] = 0;
    status[i] = ZT_OK;
    if (members) members[i] = nullptr;
    if (nmembers) nmembers[i] = 0;
  }
  std::vector<std::string> msgs(count);
  const GunzipArgs A{in, n, out, out_len, members, nmembers, status, msgs.data()};
  std::vector<zt_gunzip_batch_stats> st(batch_devices().size() + 1, zt_gunzip_batch_stats{0, 0, 0, 0, 0});
  run_shares(n, count, status, msgs.data(), [&](size_t d, DeviceCtx *c, const std::vector<size_t> &ids) {
    const int rc = gunzip_share_locked(c, A, ids, &st[d]);
    if (rc)  // (the share failed as a whole: nothing of it is handed out)
      for (size_t i : ids) {
        zt_free(out[i]);
        out[i] = nullptr;
        out_len[i] = 0;
        if (members) {
          zt_free(members[i]);
          members[i] = nullptr;
        }
        if (nmembers) nmembers[i] = 0;
      }
    return rc;
  });
  for (const zt_gunzip_batch_stats &s : st) {
    t_stats.candidates += s.candidates;
    t_stats.members += s.members;
    t_stats.decode_passes += s.decode_passes;
    t_stats.redecoded += s.redecoded;
  }
  return finish(count, status, msgs);
}

int zt_zlib_decompress_batch(const uint8_t *const *in, const size_t *n, const size_t *index, size_t count,
                             int verify, uint8_t **out, size_t *out_len, size_t *end_ip, uint32_t *adler_out,
                             int *status) {
  return zlib_batch(in, n, index, count, verify, nullptr, 0, out, out_len, end_ip, adler_out, status);
}

int zt_zlib_decompress_batch_dict(const uint8_t *const *in, const size_t *n, const size_t *index, size_t count,
                                  int verify, const uint8_t *dict, size_t dict_len, uint8_t **out, size_t *out_len,
                                  size_t *end_ip, uint32_t *adler_out, int *status) {
  return zlib_batch(in, n, index, count, verify, dict, dict_len, out, out_len, end_ip, adler_out, status);
}

const char *zt_container_batch_message(size_t i) { return i < t_msgs.size() ? t_msgs[i].c_str() : ""; }

int zt_gunzip_batch_last_stats(zt_gunzip_batch_stats *out) {
  if (!out) return set_error(ZT_E_ARG, "null output");
  *out = t_stats;
  return ZT_OK;
}

}  // extern "C"
