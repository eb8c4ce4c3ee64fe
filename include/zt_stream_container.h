/* zt_stream_container.h -- container sessions: streaming gunzip (RFC 1952,
 * any number of members) and zlib inflate (RFC 1950, FDICT included) over the
 * inflate sessions of zt_stream.h.
 *
 * A container session is fed only the new bytes each time, many sessions per
 * call.  The host follows the framing -- member header, trailer, the next
 * member -- over the bytes it holds back; every DEFLATE body is decoded by
 * the inflate sessions' kernel, one wavefront per session per launch, and a
 * session that starts a new member has its device record turned over (output
 * position, phase and bit offset reset) before the next launch of the same
 * call, on the input already uploaded.
 *
 * The law.  For a byte string X cut into feeds in any way, last != 0 on the
 * final one: the concatenated outputs are the decode of X; the final status
 * and message are those of the one-shot call on X (gzip: zt_gunzip; zlib:
 * zt_zlib_decompress_dict with the session's dictionary and verify).  Bytes
 * returned before an error are a prefix of the true decode (a failing feed
 * returns what its earlier launches decoded), an error is sticky, and it is
 * reported by the first feed that can decide it: a bad header field when the
 * field is complete, a bad trailer when its last byte arrives.  Exceptions:
 *   1. truncation inside a Huffman code reports ZT_E_INPUT_BROKEN (the
 *      inflate sessions' behaviour; truncation inside a stored block's LEN /
 *      NLEN reports ZT_E_STORED_LEN / ZT_E_STORED_NLEN as the one-shot calls do);
 *   2. the FHCRC of a member after the first is taken over that member's own
 *      header, as RFC 1952 says (zt_gunzip follows the reference and starts
 *      at the beginning of the whole input, which a stream does not keep);
 *   3. header fields of one member totalling more than 1 MiB fail with
 *      ZT_E_ARG ("gzip header fields exceed 1 MiB"): the bound of the host's
 *      carry buffer.
 *
 * Progress.  A header is consumed as soon as it is complete.  In a body the
 * guarantee of zt_stream.h holds: every token lying completely in the bytes
 * fed so far minus the last 8 is decoded and returned.  A gzip trailer is 8
 * bytes, so it is checked by the feed that delivers its eighth byte.  A zlib
 * trailer is 4 bytes: the stream's final token can lie within 8 bytes of the
 * trailer's end, and then it is decoded, and the Adler-32 compared, only by
 * the feed with last != 0.  Several members inside one feed are all decoded
 * by that call.  With at_member_end set and no further bytes, last != 0
 * finishes the session cleanly.
 */
#ifndef ZT_STREAM_CONTAINER_H
#define ZT_STREAM_CONTAINER_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZT_SESSION_GZIP 1
#define ZT_SESSION_ZLIB 2
#define ZT_SESSION_AUTO 0 /* 1F 8B: gzip; a valid CMF / FLG pair: zlib; else the gzip signature error */

typedef struct zt_container_session zt_container_session;

/* dict[0..dict_len): the preset dictionary of a zlib stream with FDICT (NULL / 0: none); copied.
 * verify != 0: the zlib Adler-32 is compared (gzip members are always verified). */
int zt_container_session_create(int format, const uint8_t *dict, size_t dict_len, int verify,
                                zt_container_session **s);
void zt_container_session_destroy(zt_container_session *s);

/* Feed n NEW bytes. last != 0: no more input will come. *out (zt_free) receives this call's output bytes,
 * also when the call fails behind them. */
int zt_container_session_feed(zt_container_session *s, const uint8_t *in, size_t n, int last, uint8_t **out,
                              size_t *out_len);

/* count distinct sessions of the calling thread's device in one call (else ZT_E_ARG); last may be NULL
 * (all 0).  status[i] per item, the call returns the first failure; every out[i] is released with
 * zt_free; count == 0 returns ZT_OK without touching a device.  A call that fails as a whole (a device or
 * allocation error, every status[i] set to it) fails the sessions it fed for good. */
int zt_container_sessions_feed(zt_container_session *const *s, const uint8_t *const *in, const size_t *n,
                               const int *last, size_t count, uint8_t **out, size_t *out_len, int *status);

typedef struct {
  uint64_t total_in;      /* bytes fed */
  uint64_t total_out;     /* bytes returned, all members */
  uint64_t members_done;  /* members whose trailer was checked */
  uint64_t unused;        /* zlib: bytes fed behind the Adler-32 */
  uint64_t decoded_bits;  /* bits the kernel read over all launches, re-read block headers included */
  uint64_t end_bits;      /* bits of the fed bytes consumed: headers, decoded tokens, trailers */
  uint32_t crc32, adler32;/* of the current member's bytes returned so far (the last member's once it is done) */
  int32_t  at_member_end; /* every byte fed so far belongs to complete, verified members */
  int32_t  finished;      /* zlib: the trailer was passed; gzip: last != 0 was fed at a member's end */
  int32_t  status;        /* ZT_OK, or the sticky error */
  uint32_t launches;      /* kernel launches this session took part in */
  int32_t  format;        /* ZT_SESSION_GZIP / ZT_SESSION_ZLIB; ZT_SESSION_AUTO while undecided */
  uint32_t pending;       /* fed bytes not yet consumed (held by the session) */
} zt_container_session_info;
int zt_container_session_get_info(const zt_container_session *s, zt_container_session_info *info);

/* Member i < members_done: the fields of zt_gzip_member (zero for a zlib stream but crc32 = its
 * Adler-32), the name and comment bytes (owned by the session, valid until it is destroyed), and
 * 64-bit positions.  The name and comment pointers stay valid while later members are added. */
typedef struct {
  uint32_t flg, mtime, xfl, os, xlen;
  uint32_t has_crc16, crc16;
  uint32_t crc32, isize;
  uint32_t pad;
  const uint8_t *name;    /* valid when flg & FNAME */
  size_t name_len;
  const uint8_t *comment; /* valid when flg & FCOMMENT */
  size_t comment_len;
  uint64_t data_off, data_len; /* the member's bytes within the total output */
  uint64_t in_off;             /* the member's first header byte within the total input */
} zt_container_member;
int zt_container_session_member(const zt_container_session *s, size_t i, zt_container_member *m);
const char *zt_container_session_message(const zt_container_session *s); /* "" or the one-shot call's text */

#ifdef __cplusplus
}
#endif
#endif
