// container_stream_api.cpp -- the container sessions' C interface
// (include/zt_stream_container.h).  A container session is an inflate session
// (stream_session.h) with a frame: the framing logic is
// container_stream_host.h, the feed is the inflate sessions' round loop
// (sessions_feed_rounds, stream_api.cpp), the only device code of its own is
// the record turn-over (session_turn.hip).
#include <cstring>
#include <vector>

#include "../../include/zt_stream_container.h"
#include "stream_session.h"

static_assert(ZT_SESSION_AUTO == zt::CS_AUTO && ZT_SESSION_GZIP == zt::CS_GZIP && ZT_SESSION_ZLIB == zt::CS_ZLIB,
              "the header's formats are the frame's");

struct zt_container_session {
  zt_inflate_session raw;
  zt::CsFrame frame;
  std::vector<uint8_t> window;  // the last 32 KiB of the dictionary
};

using namespace zt;

extern "C" {

int zt_container_session_create(int format, const uint8_t *dict, size_t dict_len, int verify,
                                zt_container_session **s) {
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  if (!s || (dict_len && !dict)) return set_error(ZT_E_ARG, "null argument");
  *s = nullptr;
  if (format != ZT_SESSION_AUTO && format != ZT_SESSION_GZIP && format != ZT_SESSION_ZLIB)
    return set_error(ZT_E_ARG, "unknown session format");
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  SessRec *rec;
  ZT_TRY(session_record_take(c, nullptr, 0, &rec));
  zt_container_session *z = new zt_container_session();
  z->raw.device = c->device;
  z->raw.d_rec = rec;
  z->raw.frame = &z->frame;
  z->frame.init(format, verify);
  if (dict_len) {
    z->frame.has_dict = true;
    z->frame.dict_id = adler32_small(dict, dict_len);
    z->frame.dict_len = dict_window_len(dict_len);
    z->window.assign(dict + dict_window_off(dict_len), dict + dict_len);
    z->raw.window = z->window.data();
    z->raw.wlen = z->frame.dict_len;
  }
  *s = z;
  return ZT_OK;
}

void zt_container_session_destroy(zt_container_session *s) {
  if (!s) return;
  if (s->raw.d_rec) session_record_give(s->raw.device, s->raw.d_rec);
  delete s;
}

int zt_container_sessions_feed(zt_container_session *const *s, const uint8_t *const *in, const size_t *n,
                               const int *last, size_t count, uint8_t **out, size_t *out_len, int *status) {
  if (count == 0) return ZT_OK;
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  if (!s || !in || !n || !out || !out_len || !status) return set_error(ZT_E_ARG, "null argument");
  for (size_t i = 0; i < count; ++i) {
    if (!s[i] || (n[i] && !in[i])) return set_error(ZT_E_ARG, "null session or input");
    if (s[i]->raw.device != c->device) return set_error(ZT_E_ARG, "session belongs to another device");
  }
  if (sess_has_duplicates(reinterpret_cast<const void *const *>(s), count))
    return set_error(ZT_E_ARG, "a session is named twice in one call");
  std::vector<zt_inflate_session *> raws(count);
  for (size_t i = 0; i < count; ++i) raws[i] = &s[i]->raw;
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  const int rc = sessions_feed_rounds(c, raws.data(), in, n, last, count, out, out_len, status);
  if (rc) {
    // the call itself failed (a device or allocation error): no item keeps an output, and the
    // sessions it fed are failed for good -- their frames may have walked on over bytes whose
    // bodies were never decoded, and a queued turn-over may not have run
    const std::string msg = zt_last_error_message();
    for (size_t i = 0; i < count; ++i) {
      zt_free(out[i]);
      out[i] = nullptr;
      out_len[i] = 0;
      zt_inflate_session &r = s[i]->raw;
      if (r.status == ZT_OK) {
        r.status = rc;
        r.msg = msg;
        r.pending.clear();
        r.pending.shrink_to_fit();
      }
      status[i] = r.status;
    }
    return set_error(rc, msg);
  }
  for (size_t i = 0; i < count; ++i)
    if (status[i]) return set_error(status[i], s[i]->raw.msg);
  return ZT_OK;
}

int zt_container_session_feed(zt_container_session *s, const uint8_t *in, size_t n, int last, uint8_t **out,
                              size_t *out_len) {
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  if (!s || !out || !out_len) return set_error(ZT_E_ARG, "null argument");
  int st = ZT_OK;
  *out = nullptr;
  *out_len = 0;
  return zt_container_sessions_feed(&s, &in, &n, &last, 1, out, out_len, &st);
}

int zt_container_session_get_info(const zt_container_session *s, zt_container_session_info *info) {
  if (!s || !info) return set_error(ZT_E_ARG, "null argument");
  const zt_inflate_session &r = s->raw;
  const CsFrame &f = s->frame;
  memset(info, 0, sizeof *info);
  info->total_in = r.total_in;
  info->total_out = r.total_out;
  info->members_done = f.members_done;
  info->unused = f.unused;
  info->decoded_bits = r.decoded_bits;
  info->end_bits = cs_end_bits(r.total_in, f.unused, r.pending.size(), r.bit_off);
  info->crc32 = f.crc;
  info->adler32 = f.adler;
  info->at_member_end = r.status == ZT_OK && f.at_member_end() && r.pending.empty();
  info->finished = r.finished;
  info->status = r.status;
  info->launches = r.launches;
  info->format = f.format;
  info->pending = (uint32_t)r.pending.size();
  return ZT_OK;
}

int zt_container_session_member(const zt_container_session *s, size_t i, zt_container_member *m) {
  if (!s || !m) return set_error(ZT_E_ARG, "null argument");
  if (i >= s->frame.members_done) return set_error(ZT_E_ARG, "no such member");
  const CsMember &k = s->frame.members[i];
  memset(m, 0, sizeof *m);
  m->flg = k.m.flg;
  m->mtime = k.m.mtime;
  m->xfl = k.m.xfl;
  m->os = k.m.os;
  m->xlen = k.m.xlen;
  m->has_crc16 = k.m.has_crc16;
  m->crc16 = k.m.crc16;
  m->crc32 = k.m.crc32;
  m->isize = k.m.isize;
  m->name = reinterpret_cast<const uint8_t *>(k.name.data());
  m->name_len = k.name.size();
  m->comment = reinterpret_cast<const uint8_t *>(k.comment.data());
  m->comment_len = k.comment.size();
  m->data_off = k.data_off;
  m->data_len = k.data_len;
  m->in_off = k.in_off;
  return ZT_OK;
}

const char *zt_container_session_message(const zt_container_session *s) { return s ? s->raw.msg.c_str() : ""; }

}  // extern "C"
