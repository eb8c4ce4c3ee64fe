// inflate_stream.hip -- the inflate sessions' kernel (include/zt_stream.h).
//
// One wavefront per session that has work, the grid indexing a job table as
// inflate_batch_kernel does.  A session's state is its device record
// (SessRec, stream_host.h): the 32 KiB history ring, the phase (at a block
// header, in a Huffman body, in a stored body, finished), the block's BFINAL /
// BTYPE, the stored bytes left, the current dynamic block's code lengths and
// the bit offset into the first pending byte.  A launch
//   1. loads the ring into LDS,
//   2. rebuilds the block's two decode tables from the recorded code lengths
//      (build_table: no header byte is needed again),
//   3. decodes from the job's input slot into its output slot, token by token,
//   4. writes back the state and the part of the ring that changed.
// It stops for exactly four reasons (SessStop): the next token or header is
// not complete, the output slot has fewer than 258 bytes of room, the final
// block ended, or the stream is corrupt.  Every stop leaves the state at a
// token boundary or at the start of the block header that did not complete (a
// partial dynamic header is read again from its start: below 1 KiB).
//
// A second reader of the record: cs_truncation (container_stream_host.h)
// walks a final feed's tokens on the host from the record's phase, bfinal,
// btype, stored_left, hlit, hdist and lens, as step 1 and step 2 below read
// them, after a container session's launch ran out of input.  A change to
// what those fields mean, or to SessRec's layout behind the ring
// (stream_api.cpp reads lens .. hdist in one copy), has to be made there too.
//
// Phantom bits: the Reader of inflate_common.h reads the bits past the end of
// the input as zeros, and a token can "decode" from them.  So nothing is
// written to the ring before the whole token -- code, extra bits, distance
// code, extra bits -- has passed the readers' end-of-input tests (decode_sym
// and Reader::bits test every piece against the end exactly).  A match copy
// overwrites the oldest 258 bytes of history, which a later distance-32768
// match reads: taking back the write cursor after the copy would be too late.
// A feed that is not the last starts no token in its last 8 bytes; a token is
// at most 48 bits, so every bit such a feed decodes is a real one.
#include "inflate_common.h"
#include "stream_host.h"

namespace zt {

namespace {

static_assert(kSessRing == RING, "the record's ring is the decoder's");

struct SessShared {
  uint8_t ring[RING];
  uint32_t inbuf[IN_RING_WORDS + 4];
  HuffTab lit;
  HuffTab dist;
  uint8_t lens[320];
};

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// ring bytes [lo, hi) (output positions) to the slot: out[p - base]; whole
// aligned dwords of the slot by one store each
__device__ __attribute__((noinline)) void sess_flush(const uint8_t *ring, uint8_t *out, uint64_t base, uint64_t lo,
                                                     uint64_t hi, int lane) {
  if (lo >= hi) return;
  const uint64_t qlo = lo - base, qhi = hi - base;
  for (uint64_t q = (qlo & ~uint64_t(3)) + (uint64_t)lane * 4; q < qhi; q += 256) {
    const uint64_t p = base + q;
    if (q >= qlo && q + 4 <= qhi) {
      const uint32_t w = (uint32_t)ring[p & RING_MASK] | ((uint32_t)ring[(p + 1) & RING_MASK] << 8) |
                         ((uint32_t)ring[(p + 2) & RING_MASK] << 16) | ((uint32_t)ring[(p + 3) & RING_MASK] << 24);
      *(uint32_t *)(out + q) = w;
    } else {
      for (int j = 0; j < 4; ++j)
        if (q + j >= qlo && q + j < qhi) out[q + j] = ring[(p + j) & RING_MASK];
    }
  }
}

__device__ __forceinline__ uint32_t sess_mod(uint32_t i, uint32_t d, float inv) {
  uint32_t q = (uint32_t)((float)i * inv);
  int32_t r = (int32_t)i - (int32_t)(q * d);
  if (r < 0) r += (int32_t)d;
  if (r >= (int32_t)d) r -= (int32_t)d;
  return (uint32_t)r;
}

// the reader's two end-of-input statuses (Reader::bits, decode_sym)
__device__ __forceinline__ bool ran_out(int st) { return st == ZT_E_INPUT_BROKEN || st == ZT_E_INVALID_CODE_LENGTH; }

__global__ __launch_bounds__(64) void session_kernel(const SessJob *__restrict__ jobs,
                                                     SessResult *__restrict__ results, int count) {
  __shared__ SessShared sh;
  const int j = blockIdx.x;
  if (j >= count) return;
  const int lane = threadIdx.x & 63;
  const SessJob job = jobs[j];
  SessRec *rec = job.rec;
  const bool last = job.last != 0;

  // ---- 1. the record
  const uint64_t op0 = rec->op;
  uint32_t phase = rec->phase, bfinal = rec->bfinal, btype = rec->btype, stored_left = rec->stored_left;
  uint32_t hlit = rec->hlit, hdist = rec->hdist;
  const uint32_t bit_off = rec->bit_off;
  {
    const uint32_t valid = op0 >= RING ? RING : (uint32_t)((op0 + 15) & ~uint64_t(15));
    const u32x4_t *src = (const u32x4_t *)rec->ring;
    u32x4_t *dst = (u32x4_t *)sh.ring;
    for (uint32_t i = lane; i < valid / 16; i += 64) dst[i] = src[i];
  }
  for (int s = lane; s < 320; s += 64) sh.lens[s] = rec->lens[s];
  wave_sync();

  Reader rd;
  rd.init(job.in, job.n, 0, sh.inbuf, lane);
  const uint64_t hi_bits = rd.hi * 8;
  // no token starts at or behind `limit` (sess_limit_bits, relative to the aligned base)
  const uint64_t limit = last ? hi_bits : (job.n > kSessLag ? (rd.hi - kSessLag) * 8 : rd.lo * 8);
  const uint64_t start_bits = rd.lo * 8 + bit_off;
  HuffTab *lt = &sh.lit, *dt = &sh.dist;
  int status = ZT_OK, detail = 0, stop = -1;
  uint32_t v;
  if (bit_off && !rd.template bits<false>((int)bit_off, v)) {
    status = ZT_E_INTERNAL;  // the host keeps the byte the offset points into
    stop = SS_ERROR;
  }

  // ---- 2. the tables of the block the session is in
  if (stop < 0 && phase == SP_HUFF) {
    int bst;
    if (btype == 1) {
      bst = read_tables<false>(rd, sh.lens, lt, dt, 1, lane, detail);
    } else {
      bst = build_table(sh.lens, (int)hlit, lt, lane, false, TREE_LITLEN);
      if (!bst) bst = build_table(sh.lens + hlit, (int)hdist, dt, lane, true, TREE_DIST);
    }
    if (bst) {
      status = ZT_E_INTERNAL;  // they were built from these lengths before
      stop = SS_ERROR;
    }
  }

  // ---- 3. decode
  uint64_t op = op0, flushed = op0;
  uint64_t done_bits = start_bits;  // the reader's position behind the last thing decoded
  const uint64_t cap = job.cap;
  g_u8 *gin = rd.abase;
  while (stop < 0) {
    if (phase == SP_DONE) {
      stop = SS_FINISHED;
      break;
    }
    if (phase == SP_HEADER) {
      if (!last && rd.pos_bits() >= limit) {
        stop = SS_NEED_INPUT;
        break;
      }
      if (!rd.template bits<false>(3, v)) {
        status = ZT_E_INPUT_BROKEN;
        stop = SS_ERROR;
        break;
      }
      bfinal = v & 1;
      btype = v >> 1;
      if (btype == 0) {
        // stored (src/RawInflate.ts:251-318): LEN at the next byte boundary, NLEN not compared
        const uint64_t p = (rd.pos_bits() + 7) >> 3;
        if (p + 4 > rd.hi) {
          if (last) {
            status = ZT_E_INPUT_BROKEN;
            stop = SS_ERROR;
          } else {
            stop = SS_NEED_INPUT;
          }
          break;
        }
        stored_left = (uint32_t)gin[p] | ((uint32_t)gin[p + 1] << 8);
        rd.seek_byte(p + 4 - rd.lo);
        done_bits = (p + 4) * 8;
        phase = stored_left ? SP_STORED : (bfinal ? SP_DONE : SP_HEADER);
        continue;
      }
      if (btype == 2) {  // read_tables keeps HLIT / HDIST to itself: peek them
        rd.refill();
        hlit = ((uint32_t)rd.bb & 31) + 257;
        hdist = (((uint32_t)rd.bb >> 5) & 31) + 1;
      }
      const int st = read_tables<false>(rd, sh.lens, lt, dt, btype, lane, detail);
      if (st) {
        if (ran_out(st) && !last) {
          stop = SS_NEED_INPUT;  // the header's bytes stay pending
        } else {
          status = ran_out(st) ? ZT_E_INPUT_BROKEN : st;
          stop = SS_ERROR;
        }
        break;
      }
      done_bits = rd.pos_bits();
      phase = SP_HUFF;
      continue;
    }
    if (phase == SP_STORED) {
      const uint64_t p = rd.pos_bits() >> 3;  // (a byte boundary: seek_byte left no bits buffered)
      const uint64_t in_end = limit >> 3;
      const uint64_t avail = in_end > p ? in_end - p : 0;
      const uint64_t room = cap - (op - op0);
      if (room == 0) {
        stop = SS_OUT_FULL;
        break;
      }
      if (avail == 0) {
        if (last) {
          status = ZT_E_INPUT_BROKEN;
          stop = SS_ERROR;
        } else {
          stop = SS_NEED_INPUT;
        }
        break;
      }
      uint32_t piece = stored_left;
      if (piece > avail) piece = (uint32_t)avail;
      if (piece > room) piece = (uint32_t)room;
      const uint32_t gran_room = GRAN - (uint32_t)(op - flushed);
      if (piece > gran_room) piece = gran_room;
      for (uint32_t k = lane; k < piece; k += 64) sh.ring[(op + k) & RING_MASK] = gin[p + k];
      wave_sync();
      op += piece;
      stored_left -= piece;
      if (op - flushed >= GRAN) {
        sess_flush(sh.ring, job.out, op0, flushed, flushed + GRAN, lane);
        flushed += GRAN;
      }
      rd.seek_byte(p + piece - rd.lo);
      done_bits = (p + piece) * 8;
      if (stored_left == 0) phase = bfinal ? SP_DONE : SP_HEADER;
      continue;
    }
    // ---- SP_HUFF: one token per turn (src/RawInflate.ts:466-516)
    for (;;) {
      op = uni64(op);
      if (cap - (op - op0) < 258) {
        stop = SS_OUT_FULL;
        break;
      }
      if (!last && rd.pos_bits() >= limit) {
        stop = SS_NEED_INPUT;
        break;
      }
      int clen = 0, st = ZT_OK;
      const int sym = decode_sym<false>(rd, lt, clen);
      if (sym >= 0 && sym < 256) {
        if (lane == 0) sh.ring[op & RING_MASK] = (uint8_t)sym;
        op++;
        done_bits = rd.pos_bits();
        if (op - flushed >= GRAN) {
          wave_sync();
          sess_flush(sh.ring, job.out, op0, flushed, flushed + GRAN, lane);
          flushed += GRAN;
        }
        continue;
      }
      if (sym == 256) {
        done_bits = rd.pos_bits();
        phase = bfinal ? SP_DONE : SP_HEADER;
        break;
      }
      uint32_t length = 0, dist = 0;
      if (sym < 0) {
        st = sym;
        detail = clen;
      } else {
        const uint32_t ls = uni((uint32_t)(sym - 257));  // (<= 28: decode_sym rejects 286 / 287)
        length = len_base(ls);
        const uint32_t lx = len_extra(ls);
        if (lx) {
          if (rd.template bits<false>((int)lx, v))
            length += v;
          else
            st = ZT_E_INPUT_BROKEN;
        }
        if (!st) {
          const int ds = decode_sym<false>(rd, dt, clen);
          if (ds < 0) {
            st = ds;
            detail = clen;
          } else if (ds >= 30) {
            st = ZT_E_INVALID_SYMBOL;
          } else {
            const uint32_t dsu = uni((uint32_t)ds);
            dist = dist_base(dsu);
            const uint32_t dx = dist_extra(dsu);
            if (dx) {
              if (rd.template bits<false>((int)dx, v))
                dist += v;
              else
                st = ZT_E_INPUT_BROKEN;
            }
            if (!st && dist > op) st = ZT_E_INVALID_DISTANCE;  // (op counts the preset window)
          }
        }
      }
      if (st) {
        // the token is not complete (the last feed: the stream is), or it is corrupt
        if (ran_out(st) && !last) {
          stop = SS_NEED_INPUT;
        } else {
          status = ran_out(st) ? ZT_E_INPUT_BROKEN : st;
          stop = SS_ERROR;
        }
        break;
      }
      // the whole token lies inside the input: only now the ring is written.
      // Byte k of the match is history[src + k mod dist], all of it before the
      // cursor: every read is issued before any write
      wave_sync();
      {
        const uint64_t src = op - dist;
        const uint32_t ng = (length + 63) >> 6;
        uint32_t b[5];
        if (dist >= length) {
#pragma unroll
          for (int g = 0; g < 5; ++g)
            if (g < (int)ng) b[g] = sh.ring[(src + g * 64 + lane) & RING_MASK];
        } else {
          const float inv = __builtin_amdgcn_rcpf((float)dist);
#pragma unroll
          for (int g = 0; g < 5; ++g)
            if (g < (int)ng) b[g] = sh.ring[(src + sess_mod(g * 64 + lane, dist, inv)) & RING_MASK];
        }
        wave_sync();
#pragma unroll
        for (int g = 0; g < 5; ++g)
          if (g < (int)ng && (uint32_t)(g * 64 + lane) < length) sh.ring[(op + g * 64 + lane) & RING_MASK] = (uint8_t)b[g];
      }
      wave_sync();
      op += length;
      done_bits = rd.pos_bits();
      if (op - flushed >= GRAN) {
        sess_flush(sh.ring, job.out, op0, flushed, flushed + GRAN, lane);
        flushed += GRAN;
      }
    }
  }
  wave_sync();

  // ---- 4. the output's rest, the record, the result
  const bool failed = stop == SS_ERROR;
  if (!failed) {
    sess_flush(sh.ring, job.out, op0, flushed, op, lane);
    if (op != op0) {
      // ring bytes [max(op0, op - RING), op), as whole 16-byte pieces (the bytes
      // around them are the record's own)
      uint64_t a = op - op0 >= RING ? op - RING : op0;
      a &= ~uint64_t(15);
      uint64_t b = (op + 15) & ~uint64_t(15);
      if (b - a > RING) a = b - RING;
      u32x4_t *dst = (u32x4_t *)rec->ring;
      const u32x4_t *src = (const u32x4_t *)sh.ring;
      for (uint64_t p = a + (uint64_t)lane * 16; p < b; p += 1024) {
        const uint32_t i = (uint32_t)(p & RING_MASK) >> 4;
        dst[i] = src[i];
      }
    }
    if (phase == SP_HUFF && btype == 2)
      for (int s = lane; s < 320; s += 64) rec->lens[s] = sh.lens[s];
  }
  if (lane == 0) {
    if (failed) {
      rec->status = status;
      rec->detail = detail;
    } else {
      rec->op = op;
      rec->phase = phase;
      rec->bfinal = bfinal;
      rec->btype = btype;
      rec->stored_left = stored_left;
      rec->hlit = hlit;
      rec->hdist = hdist;
      rec->bit_off = (uint32_t)(done_bits & 7);
    }
    SessResult r;
    r.end_bits = done_bits - rd.lo * 8;
    r.out_len = failed ? 0 : op - op0;
    const uint64_t pos = rd.pos_bits();
    r.read_bits = pos > start_bits ? pos - start_bits : 0;
    r.stop = stop;
    r.status = status;
    r.detail = detail;
    r.pad = 0;
    results[j] = r;
  }
}

}  // namespace

int session_jobs_dev(const SessJob *d_jobs, SessResult *d_res, int count, hipStream_t s) {
  if (count <= 0) return ZT_OK;
  session_kernel<<<count, 64, 0, s>>>(d_jobs, d_res, count);
  ZT_HIP(hipGetLastError());
  return ZT_OK;
}

}  // namespace zt
