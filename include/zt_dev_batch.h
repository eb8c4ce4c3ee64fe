/*
 * zt_dev_batch.h -- device-resident batch deflate and inflate over pointer
 * arrays: many buffers that already lie in GPU memory, compressed or decoded
 * in one call without crossing to the host.  The device-resident form of
 * zt_deflate_raw_batch, zt_zlib_compress_batch, zt_gzip_compress_batch and
 * zt_inflate_raw_batch.
 *
 * The pointer arrays themselves (d_in, n, d_out, out_cap, ...) are host
 * arrays; the buffers they point to are device memory at any address and
 * alignment.  The contract is the one of zt_deflate_dev / zt_inflate_dev
 * (zt.h):
 *   - all pointers belong to the calling thread's device (zt_set_device);
 *     zt_set_devices does not apply: no multi-GPU fan-out;
 *   - the work is ordered after what `stream` holds when the call is made and
 *     is visible to `stream` when the call returns; stream == NULL means the
 *     library's stream.  With a caller's stream the library's own streams are
 *     ordered against it by events in both directions;
 *   - host outputs (lengths, statuses, end positions, checksums) are valid on
 *     return; device bytes are valid once `stream` is synchronised;
 *   - the calls may synchronise internally (the pipelines read their offsets
 *     back).
 *
 * Capacity, both directions.  An item whose result is longer than out_cap[i]
 * gets status ZT_E_ARG ('output capacity too small'), out_len[i] = the length
 * it needs, and no byte of d_out[i] written; the other items are unaffected.
 * No byte outside [d_out[i], d_out[i] + out_cap[i]) is ever written, and no
 * byte outside [d_in[i], d_in[i] + n[i]) is read except within the aligned
 * 16-byte words that hold an item's first and last byte.  The call returns
 * the first failing item's code (in item order) with its message set
 * (zt_last_error_message); count == 0 returns ZT_OK.
 *
 * Device memory.  Inputs are gathered into library scratch, the pipeline
 * runs there, results are scattered to the caller's buffers.  A batch is cut
 * into groups of at most 128 MiB (deflate: every item rounded up to 32 KiB)
 * or 256 MiB (inflate) of packed input; an item larger than that is a group
 * of its own.  So for any count a deflate call holds at most about 6.5 bytes
 * of scratch per packed byte of its largest group (input, output bound, 4
 * bytes per input byte of match words, per-block tables) plus under 200
 * bytes per item of job tables; an inflate call holds a group's packed
 * input, up to 16 bytes of token slots per input byte, and the group's
 * decoded outputs with 2 bytes of descriptors per output byte.  The scratch
 * stays with the context (zt_release_scratch).
 *
 * Not covered here: preset dictionaries, multi-GPU, container parsing on the
 * inflate side (callers skip a header they know with `index`), sizes that
 * stay on the device, device-resident forms of the index, checkpoint, BGZF
 * and Zip calls.
 */
#ifndef ZT_DEV_BATCH_H
#define ZT_DEV_BATCH_H
#include "zt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZT_DEV_BATCH_RAW  0 /* raw DEFLATE streams                 (zt_deflate_raw_batch) */
#define ZT_DEV_BATCH_ZLIB 1 /* 2-byte header | stream | Adler-32   (zt_zlib_compress_batch) */
#define ZT_DEV_BATCH_GZIP 2 /* the fixed 10-byte header (no name, no comment, MTIME 0) | stream | CRC-32 | ISIZE
                               (zt_gzip_compress_batch with default options) */

/* Item i's bytes at d_out[i] are byte-identical to element i of the host
 * batch call of the same format, options and level over the same bytes (a
 * stream depends on its own bytes only).  Compression type 0 and level 0
 * write stored blocks of at most 65535 bytes; an empty input writes the final
 * empty stored block 01 00 00 FF FF, framed.  opts may be NULL (dynamic
 * codes, level 6).  status[i]: ZT_OK or ZT_E_ARG (capacity). */
int zt_deflate_dev_batch(const void *const *d_in, const size_t *n, size_t count, const zt_deflate_opts *opts,
                         int format, void *const *d_out, const size_t *out_cap, size_t *out_len, int *status,
                         void *stream);

/* Upper bound of one item's output for n input bytes: an out_cap of at least
 * this always succeeds.  Per 32 KiB parse block the pipeline writes at most
 * the stored form with its sync point (block + 10 bytes), a 10-byte restart
 * marker follows every 32nd block inside a stream, fixed codes alone
 * (compression type 1) are allowed n / 8 + 64 more, type 0 is exact; plus the
 * format's header and trailer.  Level 0 is compression type 0.  0 for an
 * unknown type or format. */
size_t zt_deflate_dev_batch_bound(size_t n, int compression_type, int format);

/* Raw DEFLATE streams decoded from index[i] (index NULL: 0).  Per item the
 * bytes, out_len, end_ip and status are zt_inflate_raw_batch's (ref_strict =
 * 0) for the same streams, the returned code and message too.  d_out == NULL:
 * sizes only -- out_len and status are filled, nothing is written and
 * out_cap is not read.  end_ip, crc_out, adler_out may be NULL; crc_out[i] /
 * adler_out[i]: CRC-32 / Adler-32 of item i's decoded bytes, taken from their
 * device copy (0 / 1 for an item that failed to decode). */
int zt_inflate_dev_batch(const void *const *d_in, const size_t *n, const size_t *index, size_t count,
                         void *const *d_out, const size_t *out_cap, size_t *out_len, size_t *end_ip, int *status,
                         uint32_t *crc_out, uint32_t *adler_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
