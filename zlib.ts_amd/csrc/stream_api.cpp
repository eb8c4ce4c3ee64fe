// stream_api.cpp -- the inflate sessions' host side (include/zt_stream.h; the
// kernel: inflate_stream.hip; the arithmetic: stream_host.h).
//
// A session's decode state lives in its device record; the host keeps what the
// device cannot know: the unconsumed tail of the bytes it was fed (the result
// record says how many bits the decoded tokens took, so the device needs no
// carry buffer), the totals and the running checksums.  A feed call packs
// `pending | new bytes` of every session that can decode something into the
// pinned staging (pack_layout, 256-byte offsets), uploads once, launches one
// wavefront per session and reads the result records back; sessions that
// stopped on a full output slot are launched again, on the rest of the input
// already uploaded, into a larger slot.  A round's outputs are gathered dense
// on the device (dev_copy_dev), their checksums are taken from that copy
// (checksums_batch_dev) and combined with the running values on the host, and
// one download brings them into a slab: the call's own when one round did it
// all, else the pieces of the rounds move into one.
//
// The same loop serves the container sessions (stream_session.h): a session
// with a frame is walked over its header and trailer bytes on the host
// (cs_step, container_stream_host.h) before its first launch and after every
// launch that ended a body; one that starts a new member has its record turned
// over (session_turn.hip, one launch per round) and is launched again on the
// rest of its slot.
#include <cstring>
#include <map>
#include <mutex>

#include "../../include/zt_stream.h"
#include "stream_host.h"
#include "stream_session.h"
#include "zt_internal.h"

namespace zt {

int session_jobs_dev(const SessJob *d_jobs, SessResult *d_res, int count, hipStream_t s);  // inflate_stream.hip
int session_turns_dev(const SessTurn *d_turns, int count, hipStream_t s);                  // session_turn.hip

namespace {

// ---- device records: slabs of kSlabRecs, a free list per device ------------------
constexpr size_t kSlabRecs = 64;
std::mutex g_rec_mu;
std::map<int, std::vector<SessRec *>> g_rec_free;  // by logical device

int rec_take(int device, SessRec **out) {
  std::lock_guard<std::mutex> lk(g_rec_mu);
  std::vector<SessRec *> &fl = g_rec_free[device];
  if (fl.empty()) {
    void *p;
    ZT_HIP(hipMalloc(&p, kSlabRecs * sizeof(SessRec)));
    for (size_t k = kSlabRecs; k-- > 0;) fl.push_back(static_cast<SessRec *>(p) + k);
  }
  *out = fl.back();
  fl.pop_back();
  return ZT_OK;
}
void rec_give(int device, SessRec *r) {
  std::lock_guard<std::mutex> lk(g_rec_mu);
  g_rec_free[device].push_back(r);
}

const uint32_t *crc_x2n() {
  static uint32_t x2n[32];
  static std::once_flag once;
  std::call_once(once, [] {
    uint32_t bt[256], nib[ZT_CRC_NIB_N];
    crc_host_tables(bt, nib, x2n);
  });
  return x2n;
}
// CRC-32 of A | B from CRC-32(A), CRC-32(B) and len(B)
uint32_t crc_combine(uint32_t a, uint32_t b, uint64_t len_b) { return multmodp(x2nmodp(crc_x2n(), len_b, 3), a) ^ b; }

int sticky(zt_inflate_session *s, int status, int detail) {
  s->status = inflate_error(status, detail);
  s->msg = zt_last_error_message();
  s->pending.clear();
  s->pending.shrink_to_fit();
  return s->status;
}

// a container session's framing error: the frame's own code and text
int sticky_frame(zt_inflate_session *s) {
  s->status = s->frame->code;
  s->msg = s->frame->msg;
  s->pending.clear();
  s->pending.shrink_to_fit();
  return s->status;
}

// one job of a feed call: item `item`, its slot in the packed input
struct Item {
  size_t item;
  size_t m;        // pending + new bytes
  size_t used = 0; // bytes of the slot the earlier launches of this call consumed
  unsigned relaunch = 0;
  bool window = false;  // a container session's preset window goes up before its next launch
  uint64_t out_len = 0;
  uint32_t crc = 0, adler = 1;
  // its output so far: `len` bytes at `off` of round buffer `buf`, in order
  struct Piece {
    size_t buf, off, len;
  };
  std::vector<Piece> pieces;
};
// one launch round's outputs on the host, dense (64-byte offsets): a slab of `items` pointers
struct RoundBuf {
  uint8_t *p;
  size_t items;
};
void rounds_release(std::vector<RoundBuf> &rounds) {
  for (RoundBuf &r : rounds)
    for (size_t q = 0; q < r.items; ++q) slab_release(r.p);
  rounds.clear();
}

}  // namespace

int sessions_feed_rounds(DeviceCtx *c, zt_inflate_session *const *ss, const uint8_t *const *in, const size_t *n,
                         const int *last, size_t count, uint8_t **out, size_t *out_len, int *status) {
  hipStream_t s = c->stream;
  std::vector<Item> items;
  for (size_t i = 0; i < count; ++i) {
    zt_inflate_session *z = ss[i];
    out[i] = nullptr;
    out_len[i] = 0;
    status[i] = ZT_OK;
    if (z->status) {
      status[i] = z->status;
      continue;
    }
    z->total_in += n[i];
    if (z->finished) {  // trailing bytes: counted only
      if (z->frame) z->frame->unused += n[i];
      continue;
    }
    const int fin = last ? last[i] : 0;
    const size_t m = z->pending.size() + n[i];
    // (a container session outside a body: its frame decides, below)
    if ((!z->frame || z->frame->state == CS_BODY) && !sess_has_work(m, z->bit_off, fin)) {
      if (n[i]) z->pending.insert(z->pending.end(), in[i], in[i] + n[i]);
      continue;
    }
    Item it;
    it.item = i;
    it.m = m;
    items.push_back(std::move(it));
  }
  if (items.empty()) return ZT_OK;

  // ---- pack pending | new and upload once
  std::vector<size_t> ms(items.size()), ids = iota_ids(items.size());
  for (size_t k = 0; k < items.size(); ++k) ms[k] = items[k].m;
  const PackLayout L = pack_layout(ms.data(), ids, 256, 1);
  void *stage_v, *d_in_v;
  ZT_TRY(pinned(c, L.total, &stage_v, kPinBatch));
  ZT_TRY(scratch(c, kIn, L.total, &d_in_v));
  uint8_t *stage = static_cast<uint8_t *>(stage_v);
  const uint8_t *d_in = static_cast<const uint8_t *>(d_in_v);
  for (size_t k = 0; k < items.size(); ++k) {
    const zt_inflate_session *z = ss[items[k].item];
    uint8_t *dst = stage + L.off[k];
    if (!z->pending.empty()) memcpy(dst, z->pending.data(), z->pending.size());
    if (n[items[k].item]) memcpy(dst + z->pending.size(), in[items[k].item], n[items[k].item]);
  }

  // ---- container sessions: the frame bytes in front of a body.  advance(k):
  // item k, outside a body, walks on over its slot; true when a body with
  // something to decode follows.  The records to turn over collect in `turns`.
  std::vector<SessTurn> turns;
  auto advance = [&](size_t k) -> bool {
    Item &it = items[k];
    zt_inflate_session *z = ss[it.item];
    CsFrame *f = z->frame;
    const int fin = last ? last[it.item] : 0;
    if (f->state != CS_BODY) {
      const CsStep st = cs_step(f, stage + L.off[k] + it.used, it.m - it.used, fin, z->total_in - it.m + it.used);
      it.used += st.consumed;
      if (st.action == CS_ACT_ERROR) {
        status[it.item] = sticky_frame(z);
        return false;
      }
      if (st.action == CS_ACT_DONE) {
        z->finished = 1;
        f->unused += it.m - it.used;
        it.used = it.m;
        return false;
      }
      if (st.action == CS_ACT_WAIT) return false;
      if (st.turn) {
        it.window = st.window;
        turns.push_back(SessTurn{z->d_rec, st.op});
      }
    }
    return sess_has_work(it.m - it.used, z->bit_off, fin);
  };
  // the records of `turns`: preset windows first, then one turn-over launch
  auto turn_over = [&]() -> int {
    if (turns.empty()) return ZT_OK;
    void *d_turns;
    ZT_TRY(scratch(c, kSmall, turns.size() * sizeof(SessTurn), &d_turns));
    for (Item &it : items) {
      if (!it.window) continue;
      it.window = false;
      const zt_inflate_session *z = ss[it.item];
      ZT_HIP(hipMemcpyAsync(z->d_rec->ring, z->window, z->wlen, hipMemcpyHostToDevice, s));
    }
    ZT_HIP(hipMemcpyAsync(d_turns, turns.data(), turns.size() * sizeof(SessTurn), hipMemcpyHostToDevice, s));
    ZT_TRY(session_turns_dev(static_cast<const SessTurn *>(d_turns), (int)turns.size(), s));
    ZT_HIP(hipStreamSynchronize(s));  // (`turns` is pageable host memory)
    turns.clear();
    return ZT_OK;
  };
  std::vector<size_t> active;
  for (size_t k = 0; k < items.size(); ++k)
    if (!ss[items[k].item]->frame || advance(k)) active.push_back(k);
  if (!active.empty()) ZT_HIP(hipMemcpyAsync(d_in_v, stage, L.total, hipMemcpyHostToDevice, s));

  // ---- rounds: launch, read the results back, launch again what stopped on a full slot
  std::vector<RoundBuf> rounds;
  struct Guard {  // an early return keeps no round buffer
    std::vector<RoundBuf> &r;
    ~Guard() { rounds_release(r); }
  } guard{rounds};
  std::vector<SessJob> jobs;
  std::vector<SessResult> res;
  while (!active.empty()) {
    std::vector<size_t> am(active.size());
    std::vector<unsigned> ar(active.size());
    for (size_t a = 0; a < active.size(); ++a) {
      am[a] = items[active[a]].m - items[active[a]].used;
      ar[a] = items[active[a]].relaunch;
    }
    const SessOutPlan P = sess_out_plan(am, ar);
    const size_t na = active.size();
    SessJob *d_jobs = nullptr;
    SessResult *d_res = nullptr;
    DevCopyJob *d_copy = nullptr;
    ZT_TRY(scratch_carved(c, kSession, [&](void *base) {
      Carve cv(base);
      d_jobs = cv.take<SessJob>(na);
      d_res = cv.take<SessResult>(na);
      d_copy = cv.take<DevCopyJob>(na);
      return cv.bytes();
    }));
    ZT_TRY(turn_over());  // the members that start in this round
    // the slots, and behind them room for their dense copy (an output is
    // shorter than its slot by the slot's 256 bytes of slack)
    void *d_out_v, *d_sums_v;
    ZT_TRY(scratch(c, kOut, 2 * P.total, &d_out_v));
    ZT_TRY(scratch(c, kSums, na * 8, &d_sums_v));
    uint8_t *d_out = static_cast<uint8_t *>(d_out_v);
    uint8_t *d_dense = d_out + P.total;
    jobs.assign(na, SessJob{});
    for (size_t a = 0; a < na; ++a) {
      const Item &it = items[active[a]];
      const zt_inflate_session *z = ss[it.item];
      jobs[a].rec = z->d_rec;
      jobs[a].in = d_in + L.off[active[a]] + it.used;
      jobs[a].n = it.m - it.used;
      jobs[a].out = d_out + P.off[a];
      jobs[a].cap = P.cap[a] - 256;  // (the slot's last 256 bytes: slack behind the 258 of room)
      jobs[a].last = last ? last[it.item] : 0;
    }
    ZT_HIP(hipMemcpyAsync(d_jobs, jobs.data(), na * sizeof(SessJob), hipMemcpyHostToDevice, s));
    ZT_TRY(session_jobs_dev(d_jobs, d_res, (int)na, s));
    res.resize(na);
    ZT_TRY(readback(c, res.data(), d_res, na * sizeof(SessResult), s));

    // this round's outputs: gathered dense on the device, their checksums taken
    // from that copy, one download
    std::vector<uint64_t> ck_off, ck_len;
    std::vector<size_t> ck_who;
    DevCopyPlan gather;
    size_t dense = 0;
    for (size_t a = 0; a < na; ++a) {
      if (res[a].out_len > jobs[a].cap) return set_error(ZT_E_INTERNAL, "session: output slot overrun");
      if (res[a].status == ZT_OK && res[a].out_len) {
        gather.add((uint64_t)(uintptr_t)jobs[a].out, (uint64_t)(uintptr_t)(d_dense + dense), res[a].out_len);
        ck_off.push_back(dense);
        ck_len.push_back(res[a].out_len);
        ck_who.push_back(a);
        dense += align_up((size_t)res[a].out_len, 64);
      }
    }
    if (!ck_who.empty()) {
      std::vector<uint32_t> sums(ck_who.size() * 2);
      ZT_HIP(hipMemcpyAsync(d_copy, gather.jobs.data(), gather.jobs.size() * sizeof(DevCopyJob),
                            hipMemcpyHostToDevice, s));
      ZT_TRY(dev_copy_dev(d_copy, (uint32_t)gather.jobs.size(), gather.tiles, s));
      ZT_TRY(checksums_batch_dev(c, d_dense, ck_who.size(), ck_off.data(), ck_len.data(),
                                 static_cast<uint32_t *>(d_sums_v), s));
      uint8_t *h = slab_out(dense, ck_who.size(), true);
      if (!h) return set_error(ZT_E_NOMEM, "host allocation failed");
      rounds.push_back(RoundBuf{h, ck_who.size()});
      ZT_TRY(download(c, h, d_dense, dense, s));
      ZT_TRY(readback(c, sums.data(), d_sums_v, sums.size() * 4, s));
      for (size_t q = 0; q < ck_who.size(); ++q) {
        Item &it = items[active[ck_who[q]]];
        it.crc = crc_combine(it.crc, sums[2 * q], ck_len[q]);
        it.adler = adler_combine(it.adler, sums[2 * q + 1], ck_len[q]);
        it.out_len += ck_len[q];
        if (CsFrame *f = ss[it.item]->frame) {  // the member's own running checksums
          f->crc = crc_combine(f->crc, sums[2 * q], ck_len[q]);
          f->adler = adler_combine(f->adler, sums[2 * q + 1], ck_len[q]);
          f->member_out += ck_len[q];
        }
        it.pieces.push_back(Item::Piece{rounds.size() - 1, (size_t)ck_off[q], (size_t)ck_len[q]});
      }
    }

    // container sessions whose final feed ran out of input: their records' states, one wait for all
    // (cs_truncation, container_stream_host.h, walks on from them; session_kernel keeps SessRec's meaning)
    struct RecState {
      uint8_t lens[320];
      uint64_t op;
      uint32_t phase, bfinal, btype, stored_left, hlit, hdist;
    };
    static_assert(offsetof(SessRec, hdist) + 4 - offsetof(SessRec, lens) == sizeof(RecState), "the record's state");
    std::vector<size_t> rec_state_of(na, 0);
    size_t broken = 0;
    for (size_t a = 0; a < na; ++a)
      if (res[a].stop == SS_ERROR && res[a].status == ZT_E_INPUT_BROKEN && ss[items[active[a]].item]->frame)
        rec_state_of[a] = broken++;
    std::vector<RecState> rec_states(broken);
    if (broken) {
      for (size_t a = 0; a < na; ++a) {
        const zt_inflate_session *z = ss[items[active[a]].item];
        if (res[a].stop == SS_ERROR && res[a].status == ZT_E_INPUT_BROKEN && z->frame)
          ZT_HIP(hipMemcpyAsync(&rec_states[rec_state_of[a]], z->d_rec->lens, sizeof(RecState), hipMemcpyDeviceToHost,
                                s));
      }
      ZT_HIP(hipStreamSynchronize(s));
    }
    std::vector<int32_t> stops(na);
    for (size_t a = 0; a < na; ++a) {
      Item &it = items[active[a]];
      zt_inflate_session *z = ss[it.item];
      const SessResult &r = res[a];
      z->launches++;
      z->decoded_bits += r.read_bits;
      stops[a] = r.stop;
      if (r.stop == SS_ERROR) {
        int code = r.status;
        if (z->frame && code == ZT_E_INPUT_BROKEN) {
          // a container session reports the one-shot call's status: where did the input end?
          // (the record is what it was before this launch; z->bit_off too)
          const RecState &st = rec_states[rec_state_of[a]];
          const CsTruncation t = cs_truncation(stage + L.off[active[a]] + it.used, it.m - it.used, z->bit_off,
                                               st.phase, st.bfinal, st.btype, st.stored_left, st.hlit, st.hdist,
                                               st.lens);
          if (t == CS_TRUNC_STORED_LEN) code = ZT_E_STORED_LEN;
          if (t == CS_TRUNC_STORED_NLEN) code = ZT_E_STORED_NLEN;
        }
        status[it.item] = sticky(z, code, r.detail);
        continue;
      }
      // the slot's front the decoded tokens consumed
      const SessTail t = sess_tail(it.m - it.used, r.end_bits);
      z->end_bits += r.end_bits - z->bit_off;
      z->bit_off = t.bit_off;
      it.used += t.drop;
      if (r.stop == SS_FINISHED && !z->frame) z->finished = 1;
      if (r.stop == SS_OUT_FULL) it.relaunch++;
    }
    // the next round: what stopped on a full slot, and the container sessions
    // whose body ended with the next member's body inside the slot
    std::vector<char> again(na, 0);
    for (const size_t a : sess_relaunch(stops)) again[a] = 1;
    for (size_t a = 0; a < na; ++a) {
      Item &it = items[active[a]];
      zt_inflate_session *z = ss[it.item];
      if (stops[a] != SS_FINISHED || !z->frame) continue;
      if (z->bit_off) {  // the trailer starts at the next whole byte
        it.used++;
        z->bit_off = 0;
      }
      it.relaunch = 0;
      z->frame->state = CS_TRAILER;
      again[a] = advance(active[a]);
    }
    std::vector<size_t> next;
    for (size_t a = 0; a < na; ++a)
      if (again[a]) next.push_back(active[a]);
    active.swap(next);
  }
  ZT_TRY(turn_over());  // (a member whose header ended the fed bytes)

  // ---- the sessions' books and the outputs.  One round with every item's
  // output kept: its buffer is the call's slab.  Else the pieces move into one.
  bool direct = rounds.size() == 1;
  size_t slab_total = 0, slab_items = 0;
  // (a failing feed returns nothing; a container session's returns what its earlier launches decoded)
  auto keeps = [&](const Item &it) { return it.out_len && (!ss[it.item]->status || ss[it.item]->frame); };
  for (const Item &it : items) {
    if (it.out_len && !keeps(it)) direct = false;
    if (keeps(it)) {
      slab_total += align_up((size_t)it.out_len, 64);
      slab_items++;
    }
  }
  uint8_t *slab = nullptr;
  if (direct) {
    slab = rounds[0].p;
    rounds.clear();  // its pointers are the caller's now
  } else if (slab_items) {
    slab = slab_out(slab_total, slab_items, true);
    if (!slab) return set_error(ZT_E_NOMEM, "host allocation failed");
  }
  size_t at = 0;
  for (const Item &it : items) {
    zt_inflate_session *z = ss[it.item];
    if (!z->status) {
      const uint8_t *slot = stage + L.off[&it - items.data()];
      if (z->finished)
        z->pending.clear();
      else
        z->pending.assign(slot + it.used, slot + it.m);
    }
    if (!keeps(it)) continue;
    size_t w = 0;
    uint8_t *dst;
    if (direct) {
      dst = slab + it.pieces[0].off;
      w = it.pieces[0].len;
    } else {
      dst = slab + at;
      for (const Item::Piece &pc : it.pieces) {
        memcpy(dst + w, rounds[pc.buf].p + pc.off, pc.len);
        w += pc.len;
      }
      at += align_up(w, 64);
    }
    out[it.item] = dst;
    out_len[it.item] = w;
    z->crc = crc_combine(z->crc, it.crc, w);
    z->adler = adler_combine(z->adler, it.adler, w);
    z->total_out += w;
  }
  return ZT_OK;
}

// a record whose state is "at the start of a stream with this preset window"
int session_record_take(DeviceCtx *c, const uint8_t *window, size_t wlen, SessRec **out) {
  SessRec *rec;
  ZT_TRY(rec_take(c->device, &rec));
  // the record's state: everything behind the ring zero but the cursor
  static_assert(offsetof(SessRec, lens) == kSessRing, "state follows the ring");
  std::vector<uint8_t> st(sizeof(SessRec) - kSessRing, 0);
  const uint64_t op = wlen;
  memcpy(st.data() + (offsetof(SessRec, op) - kSessRing), &op, sizeof op);
  hipError_t e = hipMemcpyAsync(rec->lens, st.data(), st.size(), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && wlen) e = hipMemcpyAsync(rec->ring, window, wlen, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    rec_give(c->device, rec);
    return hip_fail(e, "session record upload");
  }
  *out = rec;
  return ZT_OK;
}
void session_record_give(int device, SessRec *rec) { rec_give(device, rec); }

}  // namespace zt

using namespace zt;

extern "C" {

int zt_inflate_session_create(const uint8_t *window, size_t wlen, zt_inflate_session **s) {
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  if (!s || (wlen && !window)) return set_error(ZT_E_ARG, "null argument");
  *s = nullptr;
  if (wlen > kSessRing) {  // only the last 32 KiB can be referenced
    window += wlen - kSessRing;
    wlen = kSessRing;
  }
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  SessRec *rec;
  ZT_TRY(session_record_take(c, window, wlen, &rec));
  zt_inflate_session *z = new zt_inflate_session();
  z->device = c->device;
  z->d_rec = rec;
  z->wlen = (uint32_t)wlen;
  *s = z;
  return ZT_OK;
}

void zt_inflate_session_destroy(zt_inflate_session *s) {
  if (!s) return;
  if (s->d_rec) rec_give(s->device, s->d_rec);
  delete s;
}

int zt_inflate_sessions_feed(zt_inflate_session *const *s, const uint8_t *const *in, const size_t *n, const int *last,
                             size_t count, uint8_t **out, size_t *out_len, int *status) {
  if (count == 0) return ZT_OK;
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  if (!s || !in || !n || !out || !out_len || !status) return set_error(ZT_E_ARG, "null argument");
  for (size_t i = 0; i < count; ++i) {
    if (!s[i] || (n[i] && !in[i])) return set_error(ZT_E_ARG, "null session or input");
    if (s[i]->device != c->device) return set_error(ZT_E_ARG, "session belongs to another device");
  }
  if (sess_has_duplicates(reinterpret_cast<const void *const *>(s), count))
    return set_error(ZT_E_ARG, "a session is named twice in one call");
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  const int rc = sessions_feed_rounds(c, s, in, n, last, count, out, out_len, status);
  if (rc) {  // the call itself failed: no item keeps an output
    for (size_t i = 0; i < count; ++i) {
      zt_free(out[i]);
      out[i] = nullptr;
      out_len[i] = 0;
    }
    return rc;
  }
  for (size_t i = 0; i < count; ++i)
    if (status[i]) return set_error(status[i], s[i]->msg);
  return ZT_OK;
}

int zt_inflate_session_feed(zt_inflate_session *s, const uint8_t *in, size_t n, int last, uint8_t **out,
                            size_t *out_len) {
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  if (!s || !out || !out_len) return set_error(ZT_E_ARG, "null argument");
  int st = ZT_OK;
  *out = nullptr;
  *out_len = 0;
  return zt_inflate_sessions_feed(&s, &in, &n, &last, 1, out, out_len, &st);
}

int zt_inflate_session_get_info(const zt_inflate_session *s, zt_inflate_session_info *info) {
  if (!s || !info) return set_error(ZT_E_ARG, "null argument");
  info->total_in = s->total_in;
  info->end_bits = s->end_bits;
  info->total_out = s->total_out;
  info->decoded_bits = s->decoded_bits;
  info->crc32 = s->crc;
  info->adler32 = s->adler;
  info->pending = (uint32_t)s->pending.size();
  info->finished = s->finished;
  info->status = s->status;
  info->launches = s->launches;
  return ZT_OK;
}

const char *zt_inflate_session_message(const zt_inflate_session *s) { return s ? s->msg.c_str() : ""; }

}  // extern "C"
