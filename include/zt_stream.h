/* zt_stream.h -- inflate sessions: streaming raw inflate that resumes at a
 * token, keeps its state on the device and is fed in batches.
 *
 * A session holds one raw DEFLATE stream being decoded.  Its history ring,
 * block state and checksums live in a device record; each feed uploads only
 * the new bytes, decodes every token they complete and returns the bytes
 * those tokens produce.  Concatenating the outputs of all feeds gives the
 * one-shot decode of the concatenated input, however the input is cut.
 *
 * Progress: after a feed with last == 0 every token (stored byte, block
 * header) that lies completely inside the bytes fed so far minus the last 8
 * has been decoded and returned; an error in such a token is reported by that
 * feed, with the code and text zt_inflate_raw gives on the whole stream.  An
 * error is sticky.  Running out of input is an error (ZT_E_INPUT_BROKEN) only
 * once last != 0.  After the final block further bytes are counted only:
 * total_in - ceil(end_bits / 8) of them trail the stream (a gzip / zlib
 * trailer).
 *
 * Throughput: one session is decoded by one wavefront, at the one-wave rate
 * of zt_inflate_raw_batch; the throughput of this interface comes from
 * feeding many sessions per call (zt_inflate_sessions_feed: one wavefront per
 * session per launch).  One huge stream belongs to zt_inflate_raw.
 * zt_set_devices does not apply: a session lives on the device that was
 * current when it was created.
 */
#ifndef ZT_STREAM_H
#define ZT_STREAM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zt_inflate_session zt_inflate_session;

/* window[0..wlen): preset history (a raw-deflate dictionary), may be NULL/0; the last 32 KiB count. */
int zt_inflate_session_create(const uint8_t *window, size_t wlen, zt_inflate_session **s);
void zt_inflate_session_destroy(zt_inflate_session *s);

/* Feed n NEW bytes. last != 0: no more input will come. *out (zt_free) receives this call's output bytes. */
int zt_inflate_session_feed(zt_inflate_session *s, const uint8_t *in, size_t n, int last, uint8_t **out,
                            size_t *out_len);

/* count distinct sessions of one device in one call; last may be NULL (all 0).
 * status[i] per item, the call returns the first failure (the batch calls' convention);
 * every out[i] is released with zt_free. */
int zt_inflate_sessions_feed(zt_inflate_session *const *s, const uint8_t *const *in, const size_t *n,
                             const int *last, size_t count, uint8_t **out, size_t *out_len, int *status);

typedef struct {
  uint64_t total_in;      /* bytes fed */
  uint64_t end_bits;      /* bits of the fed bytes consumed by decoded tokens / headers */
  uint64_t total_out;     /* bytes returned (preset window not counted) */
  uint64_t decoded_bits;  /* bits the kernel read over all launches, re-read headers included */
  uint32_t crc32, adler32;/* of the bytes returned so far */
  uint32_t pending;       /* fed bytes not yet consumed (held by the session) */
  int32_t  finished;      /* the BFINAL block's end was decoded */
  int32_t  status;        /* ZT_OK, or the sticky error */
  uint32_t launches;      /* kernel launches this session took part in */
} zt_inflate_session_info;
int zt_inflate_session_get_info(const zt_inflate_session *s, zt_inflate_session_info *info);
const char *zt_inflate_session_message(const zt_inflate_session *s); /* "" or the reference's text */

#ifdef __cplusplus
}
#endif
#endif
