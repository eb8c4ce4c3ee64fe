/*
 * zt_checkpoint.h -- checkpoint index for libzt.so: random access into raw
 * DEFLATE streams WITHOUT sync points -- what zlib, pigz, Python and Node
 * write, and the reference library's one-block RawDeflate output -- where the
 * sync-point index of zt_index.h answers ZT_E_NO_INDEX.
 *
 * zt_inflate_ckpt_build decodes the stream once on the general path
 * (speculative units cut at fixed bit positions) and keeps what that decode
 * proves: for every unit of the converged chain the exact decoder state at
 * its end -- a bit position, possibly in the middle of a block -- and that
 * state's output offset; and, every `span` output bytes, the 32 KiB of output
 * in front of such a state.  (Block boundaries alone would not do: a
 * one-block stream has a single one.)  With that blob zt_inflate_ckpt_range /
 * zt_inflate_ckpt_ranges upload and decode only the units between the last
 * window checkpoint at or before a range and the unit that holds its last
 * byte.
 *
 * Like zt_index.h: plain C, synchronous, GPU only, on the calling thread's
 * device.  A gzip or zlib caller passes the header length as `index`.  The
 * error codes are those of zt_index.h.
 *
 * The blob is a hint that is verified, never trusted: it is checked on the
 * host before any device work (no kernel sees an unchecked offset), and every
 * decoded unit is held to the next entry on the device -- end state, output
 * length, token count.  A stale or forged blob gives an error, or the given
 * stream's own bytes where the boundaries happen to hold.  The windows are
 * the one part the stream cannot prove: each carries a CRC-32 that is checked
 * on the device (ZT_E_INDEX).  That CRC guards against corruption, not
 * forgery: a forged window with a matching CRC yields wrong bytes -- never an
 * out-of-bounds access.
 *
 * Blob layout (flat, little-endian; free with zt_free; may be stored and
 * reloaded):
 *
 *   header, 64 bytes: "ZTCK" | u32 version = 1 | u32 nunits | u32 nwin
 *                     | u64 stream_start (= index) | u64 end_ip | u64 total_out
 *                     | u64 span | zero padding
 *   entries, (nunits + 1) x 48 bytes, the chain's unit boundaries in stream order:
 *                     u64 pos      bit position in `in` of the state
 *                     u64 hdr      kind 1: bit position of the block's header
 *                                  (ZT_CKPT_FIXED_HDR: fixed codes), else 0
 *                     u64 out_off  output offset of the state
 *                     u32 kind     0 a block start, 1 a token start inside a
 *                                  Huffman body, 2 a byte inside a stored
 *                                  payload, 3 a stored block's LEN field,
 *                                  4 the stream's end (the sentinel only)
 *                     u32 rem      kind 2: payload bytes left, else 0
 *                     u32 flags    bit 0: the entry has a window; bit 1: BFINAL
 *                                  of the block the state lies in (kinds 1-3)
 *                     u32 ntok     tokens between this state and the next entry's
 *                     u32 win      index of its window (flags bit 0), else 0
 *                     u32 zero
 *   entry 0 is the stream start: kind 0 at bit 8 * stream_start, out_off 0, no
 *   window.  The last entry is a sentinel: kind 4, (pos + 7) / 8 = end_ip,
 *   out_off = total_out, every other field 0.
 *   windows, nwin x 32784 bytes: the 32768 output bytes in front of the
 *                     entry | u32 CRC-32 of those bytes | 12 zero bytes
 *   A window is attached to the first entry (entry 0 and the sentinel apart)
 *   at or after every positive multiple of span.  span >= 64 KiB, so a window
 *   entry lies at least 32 KiB into the output and every window is whole; the
 *   readers refuse a blob that says otherwise.  Window indices ascend with
 *   the entries.
 *
 * Size: 32784 bytes per span of output plus 48 bytes per unit.
 *
 * Limits, out of scope: a host-pipelined build of streams too large for the
 * one-call device decode (ZT_E_NO_INDEX, as zt_inflate_index_build refuses
 * them), device resident and multi-GPU forms, compressed windows, container
 * parsing on the read side, the batch and zip paths.  The version-1
 * sync-point index of zt_index.h and its calls are unchanged.
 */
#ifndef ZT_CHECKPOINT_H
#define ZT_CHECKPOINT_H
#include "zt_index.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZT_CKPT_VERSION 1
#define ZT_CKPT_HEADER_BYTES 64
#define ZT_CKPT_ENTRY_BYTES 48
#define ZT_CKPT_WINDOW_BYTES 32768
#define ZT_CKPT_WINDOW_RECORD_BYTES 32784
#define ZT_CKPT_SPAN_DEFAULT 1048576
#define ZT_CKPT_SPAN_MIN 65536
#define ZT_CKPT_FIXED_HDR 0x4000000000000000ull

/* Decodes the raw stream at in[index..n) once, always on the general path
 * (whether or not it has sync points), and returns its checkpoint blob in
 * *idx (*idx_len bytes).  span: output bytes between window checkpoints; 0
 * means ZT_CKPT_SPAN_DEFAULT, anything else below ZT_CKPT_SPAN_MIN is
 * ZT_E_ARG.  With `out` non-NULL the decoded bytes come back too (*out,
 * *out_len, *end_ip as zt_inflate_raw gives them); with `out` NULL out_len and
 * end_ip may be NULL as well.  A stream below the general path's 16 KiB
 * minimum is decoded as one exact unit: one entry, the sentinel, no window.
 * A stream the general path does not finish returns ZT_E_NO_INDEX; a corrupt
 * stream its usual inflate status. */
int zt_inflate_ckpt_build(const uint8_t *in, size_t n, size_t index, uint64_t span, uint8_t **idx, size_t *idx_len,
                          uint8_t **out, size_t *out_len, size_t *end_ip);

/* Bytes [off, off + len) of the stream's output, pread style as
 * zt_inflate_range: off > total_out is ZT_E_ARG, len is clamped to total_out -
 * off, a clamped length of 0 returns an empty output without touching the
 * GPU.  `in` / `n` are the buffer the blob was built from. */
int zt_inflate_ckpt_range(const uint8_t *in, size_t n, const uint8_t *idx, size_t idx_len, uint64_t off, uint64_t len,
                          uint8_t **out, size_t *out_len);
/* `count` ranges in one call: unsorted, overlapping and repeated ranges are
 * fine, no unit is decoded twice.  out[i] is library memory (release each
 * with zt_free; they share one allocation); status[i] receives each range's
 * code and the call returns the first failing one.  A unit that fails its
 * verification, or a window that fails its CRC, abandons the decode of the
 * call: every non-empty range then reports a failure. */
int zt_inflate_ckpt_ranges(const uint8_t *in, size_t n, const uint8_t *idx, size_t idx_len, const uint64_t *off,
                           const uint64_t *len, size_t count, uint8_t **out, size_t *out_len, int *status);

/* Work counters of the three calls above, process-wide. */
typedef struct {
  uint64_t builds;                /* successful zt_inflate_ckpt_build calls */
  uint64_t range_calls;           /* range calls that reached the device */
  uint64_t ranges;                /* ranges asked for (empty ones included) */
  uint64_t units_tokenized;       /* units the range calls decoded */
  uint64_t in_bytes_uploaded;     /* compressed bytes (spans and block headers) the range calls uploaded */
  uint64_t out_bytes_decoded;     /* bytes the range calls decoded on the device */
  uint64_t out_bytes_returned;    /* bytes the range calls returned */
  uint64_t window_bytes_uploaded; /* window bytes the range calls uploaded */
} zt_ckpt_stats;
int zt_ckpt_stats_read(zt_ckpt_stats *out, int reset);

#ifdef __cplusplus
}
#endif
#endif
