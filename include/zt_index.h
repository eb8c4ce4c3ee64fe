/*
 * zt_index.h -- indexed random access for libzt.so: decode byte ranges of a
 * raw DEFLATE stream without decoding the whole stream.
 *
 * Streams with sync points (every stream this engine's deflate writes; zlib
 * streams flushed with Z_SYNC_FLUSH / Z_FULL_FLUSH) are decoded once by
 * zt_inflate_index_build, which records where their units start.  With that
 * index zt_inflate_range / zt_inflate_ranges upload and decode only the units
 * a range needs: from the last independent segment start at or before the
 * range up to the unit that holds its last byte.
 *
 * Like zt.h: plain C, synchronous, GPU only.  The calls run on the calling
 * thread's device (zt_set_devices does not apply).  A gzip or zlib caller
 * passes the header length as `index`.
 *
 * A stream this engine writes needs no second decode: the _indexed forms of
 * the raw, gzip and zlib writers (below) return the index with the stream.
 * The compressor knows its own unit boundaries, so this also covers inputs
 * of any size the writer takes and stored data that happens to contain the
 * sync bytes, where the build gives ZT_E_NO_INDEX.
 *
 * The index is a hint that is verified, never trusted: the blob is checked on
 * the host before any device work, and every decoded unit is checked against
 * its neighbouring entries on the device.  A stale or forged index gives an
 * error, or the given stream's own bytes where the boundaries happen to
 * hold; it never gives an out-of-bounds access.
 *
 * Index layout (flat, little-endian; free with zt_free; may be stored and
 * reloaded):
 *
 *   header, 64 bytes: "ZTIX" | u32 version = 1 | u32 nunits | u32 nseg
 *                     | u64 stream_start (= index) | u64 end_ip | u64 total_out | zero padding
 *   entries, (nunits + 1) x 24 bytes, on-chain units in stream order:
 *                     u64 in_off   byte position in `in` of the unit's first block
 *                     u64 out_off  output offset of the unit's first byte
 *                     u32 ntok     the unit's token count
 *                     u32 flags    bit 0: the unit starts an independent segment
 *                                  (unit 0, or after a restart marker)
 *   the last entry is a sentinel: in_off = end_ip, out_off = total_out, ntok = flags = 0
 *
 * Not covered here: streams without sync points (ZT_E_NO_INDEX from these
 * calls; zt_checkpoint.h has the checkpoint index that reads ranges of such
 * streams), an index *build* of streams too large for the one-call
 * device decode (the _indexed writers have no such limit), device resident
 * and multi-GPU forms, the batch and zip writers, container parsing on the
 * read side (the _indexed gzip and zlib writers set stream_start themselves).
 */
#ifndef ZT_INDEX_H
#define ZT_INDEX_H
#include "zt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZT_E_NO_INDEX -60       /* 'stream has no usable sync points' */
#define ZT_E_INDEX -61          /* the index blob is malformed, or does not fit the given input */
#define ZT_E_INDEX_MISMATCH -62 /* a decoded unit disagrees with the index (a stale index) */

#define ZT_INDEX_VERSION 1
#define ZT_INDEX_HEADER_BYTES 64
#define ZT_INDEX_ENTRY_BYTES 24

/* Decodes the raw stream at in[index..n) once and returns its index in *idx
 * (*idx_len bytes).  With `out` non-NULL the decoded bytes come back too
 * (*out, *out_len, *end_ip as zt_inflate_raw gives them); with `out` NULL only
 * the index leaves the device (out_len and end_ip may then be NULL as well).
 * A stream the sync-point path does not finish returns ZT_E_NO_INDEX; a
 * corrupt stream its usual inflate status. */
int zt_inflate_index_build(const uint8_t *in, size_t n, size_t index, uint8_t **idx, size_t *idx_len, uint8_t **out,
                           size_t *out_len, size_t *end_ip);

/* Bytes [off, off + len) of the stream's output, pread style: off >
 * total_out is ZT_E_ARG, len is clamped to total_out - off, a clamped length
 * of 0 returns an empty output without touching the GPU.  `in` / `n` are the
 * buffer the index was built from (the index holds positions in it). */
int zt_inflate_range(const uint8_t *in, size_t n, const uint8_t *idx, size_t idx_len, uint64_t off, uint64_t len,
                     uint8_t **out, size_t *out_len);
/* `count` ranges in one call: unsorted, overlapping and repeated ranges are
 * fine, no unit is decoded twice.  out[i] is library memory (release each
 * with zt_free; they share one allocation); status[i] receives each range's
 * code and the call returns the first failing one.  A unit that fails its
 * verification abandons the decode of the call: every non-empty range then
 * reports a failure. */
int zt_inflate_ranges(const uint8_t *in, size_t n, const uint8_t *idx, size_t idx_len, const uint64_t *off,
                      const uint64_t *len, size_t count, uint8_t **out, size_t *out_len, int *status);

/* Work counters of the three calls above, process-wide, counted whether
 * timing is on or not. */
typedef struct {
  uint64_t builds;            /* successful zt_inflate_index_build calls */
  uint64_t range_calls;       /* zt_inflate_range / zt_inflate_ranges calls that reached the device */
  uint64_t ranges;            /* ranges asked for (empty ones included) */
  uint64_t units_tokenized;   /* units the range calls decoded */
  uint64_t in_bytes_uploaded; /* compressed bytes the range calls uploaded */
  uint64_t out_bytes_decoded; /* bytes the range calls decoded on the device */
  uint64_t out_bytes_returned;/* bytes the range calls returned */
} zt_index_stats;
int zt_index_stats_read(zt_index_stats *out, int reset);

/* ---- the write side: the index of a stream as it is written --------------------
 * zt_deflate_raw / zt_gzip_compress / zt_zlib_compress with the index of
 * their output: *out is byte for byte what the plain call returns for the
 * same arguments, *idx (free with zt_free) a version-1 blob, byte-identical to
 * what zt_inflate_index_build returns for that output wherever that build
 * succeeds.  No second decode: one small kernel behind the encoder writes the
 * entries from what the deflate pipeline already holds.
 *
 * Raw: `stream_start` is where the caller will place the stream in the buffer
 * later handed to zt_inflate_range (a prefix of their own); it is the
 * header's stream_start and is added to every in_off and to end_ip.  gzip:
 * stream_start is the written header's length; zlib: 2 -- the container file
 * and its index go straight into zt_inflate_range.
 *
 * compression_type NONE (or level 0) writes stored blocks without sync points,
 * and the empty input one empty stored block: ZT_E_NO_INDEX as from the build,
 * before any device work, and no output.  (Preset dictionaries
 * have no indexed form: the range path has none.)
 *
 * ZT_INDEX_WRITER marks the write side's declarations, apart from the four
 * read-side calls above. */
#define ZT_INDEX_WRITER
ZT_INDEX_WRITER int zt_deflate_raw_indexed(const uint8_t *in, size_t n, const zt_deflate_opts *opts,
                                           size_t stream_start, uint8_t **out, size_t *out_len, uint8_t **idx,
                                           size_t *idx_len);
ZT_INDEX_WRITER int zt_gzip_compress_indexed(const uint8_t *in, size_t n, const zt_gzip_opts *opts, uint8_t **out,
                                             size_t *out_len, uint32_t *crc_out, uint8_t **idx, size_t *idx_len);
ZT_INDEX_WRITER int zt_zlib_compress_indexed(const uint8_t *in, size_t n, const zt_deflate_opts *opts, uint8_t **out,
                                             size_t *out_len, uint32_t *adler_out, uint8_t **idx, size_t *idx_len);

#ifdef __cplusplus
}
#endif
#endif
