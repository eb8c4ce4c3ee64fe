// stream_session.h -- what the two kinds of session share on the host: the
// inflate session's record (stream_api.cpp) and the one round loop that feeds
// raw sessions (include/zt_stream.h) and container sessions
// (include/zt_stream_container.h, container_stream_api.cpp) alike.
#pragma once
#include <string>
#include <vector>

#include "container_stream_host.h"
#include "zt_internal.h"

struct zt_inflate_session {
  int device = -1;
  zt::SessRec *d_rec = nullptr;
  std::vector<uint8_t> pending;  // fed bytes not yet consumed (the first one possibly in part: bit_off)
  uint32_t bit_off = 0;
  uint64_t total_in = 0, end_bits = 0, total_out = 0, decoded_bits = 0;
  uint32_t crc = 0, adler = 1, launches = 0;
  uint32_t wlen = 0;
  int finished = 0, status = ZT_OK;
  std::string msg;
  // a container session: its framing (null: a raw session) and its preset window
  zt::CsFrame *frame = nullptr;
  const uint8_t *window = nullptr;
};

namespace zt {

// One feed call over `count` distinct sessions of c's device (c->mu held).
// A session with a frame has its headers and trailers walked on the host
// (cs_step) and its record turned over at every new member; a failing item of
// that kind keeps the output of its earlier launches.
int sessions_feed_rounds(DeviceCtx *c, zt_inflate_session *const *ss, const uint8_t *const *in, const size_t *n,
                         const int *last, size_t count, uint8_t **out, size_t *out_len, int *status);
int session_record_take(DeviceCtx *c, const uint8_t *window, size_t wlen, SessRec **rec);  // (c->mu held)
void session_record_give(int device, SessRec *rec);

}  // namespace zt
