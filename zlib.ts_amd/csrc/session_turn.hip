// session_turn.hip -- the record turn-over of the container sessions
// (include/zt_stream_container.h): every session of a feed call that starts a
// new member has its device record (SessRec, stream_host.h) set to "at the
// first block header of a stream whose history is the preset window, or
// nothing" -- one launch per round of the call, driven by a table.  The ring
// is not cleared: session_kernel's `dist > op` test refuses every distance
// that reaches before the member's start (tests/test_gpu_container_session.py,
// test_history_is_per_member).
#include "container_stream_host.h"
#include "zt_internal.h"

namespace zt {

namespace {

__global__ __launch_bounds__(64) void session_turn_kernel(const SessTurn *__restrict__ turns, int count) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  SessRec *rec = turns[i].rec;
  rec->op = turns[i].op;
  rec->phase = SP_HEADER;
  rec->bfinal = 0;
  rec->btype = 0;
  rec->stored_left = 0;
  rec->hlit = 0;
  rec->hdist = 0;
  rec->bit_off = 0;
  rec->status = 0;
  rec->detail = 0;
}

}  // namespace

int session_turns_dev(const SessTurn *d_turns, int count, hipStream_t s) {
  if (count <= 0) return ZT_OK;
  session_turn_kernel<<<(count + 63) / 64, 64, 0, s>>>(d_turns, count);
  ZT_HIP(hipGetLastError());
  return ZT_OK;
}

}  // namespace zt
