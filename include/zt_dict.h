/*
 * zt_dict.h -- preset dictionaries for libzt.so: raw DEFLATE streams that
 * start with a dictionary in their history, and RFC 1950 (zlib) streams with
 * the FDICT flag and DICTID.  What Python's zlib.compressobj(zdict=...) /
 * decompressobj(zdict=...) and Node's `dictionary` option read and write.
 *
 * Like zt.h: plain C, synchronous, GPU only.  Every call takes the dictionary
 * as dict[0 .. dict_len); dict_len == 0 behaves exactly like the call of zt.h
 * without the _dict suffix.
 *
 * Limits.  The encoder's matches reach at most 28352 bytes back, so only the
 * last 28352 bytes of a dictionary can be match sources (a longer dictionary
 * is accepted; its earlier bytes are never referenced).  The decoder uses the
 * last 32768 bytes, all a DEFLATE distance can reach.  Dictionary streams are
 * decoded by one wavefront per stream: the right shape for batches of small
 * messages; one large stream with a dictionary is bound by that one wave.
 */
#ifndef ZT_DICT_H
#define ZT_DICT_H
#include "zt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZT_E_ZLIB_DICTID -44 /* 'invalid dictionary id: 0x<stream> / 0x<given>' */

/* One raw stream.  zt_inflate_raw_dict: *end_ip as zt_inflate_raw; a distance
 * that reaches before the dictionary's first byte is ZT_E_INVALID_DISTANCE. */
int zt_deflate_raw_dict(const uint8_t *in, size_t n, const zt_deflate_opts *opts, const uint8_t *dict,
                        size_t dict_len, uint8_t **out, size_t *out_len);
int zt_inflate_raw_dict(const uint8_t *in, size_t n, size_t index, const zt_inflate_opts *opts, const uint8_t *dict,
                        size_t dict_len, uint8_t **out, size_t *out_len, size_t *end_ip);

/* One dictionary shared by `count` buffers; arguments and per-item status as
 * zt_deflate_raw_batch / zt_inflate_raw_batch.  Both honour zt_set_devices:
 * the buffers are split over the devices, each device gets one copy of the
 * dictionary. */
int zt_deflate_raw_batch_dict(const uint8_t *const *in, const size_t *n, size_t count, const zt_deflate_opts *opts,
                              const uint8_t *dict, size_t dict_len, uint8_t **out, size_t *out_len, int *status);
int zt_inflate_raw_batch_dict(const uint8_t *const *in, const size_t *n, size_t count, const zt_inflate_opts *opts,
                              const uint8_t *dict, size_t dict_len, uint8_t **out, size_t *out_len, size_t *end_ip,
                              int *status);

/* RFC 1950 with FDICT: CMF and FLEVEL as zt_zlib_compress writes them, bit
 * 0x20 of FLG set, FCHECK recomputed; DICTID = Adler-32 of the whole
 * dictionary as given, big-endian; then the raw stream and the Adler-32 of
 * the data. */
int zt_zlib_compress_dict(const uint8_t *in, size_t n, const zt_deflate_opts *opts, const uint8_t *dict,
                          size_t dict_len, uint8_t **out, size_t *out_len, uint32_t *adler_out);
int zt_zlib_compress_batch_dict(const uint8_t *const *in, const size_t *n, size_t count,
                                const zt_deflate_opts *opts, const uint8_t *dict, size_t dict_len, uint8_t **out,
                                size_t *out_len, int *status);

/* As zt_zlib_decompress, for streams that may carry FDICT:
 *   FDICT clear                      -- decoded as zt_zlib_decompress does, the dictionary is ignored;
 *   FDICT set, DICTID == Adler-32(dict) -- decoded with the dictionary;
 *   FDICT set, DICTID differs        -- ZT_E_ZLIB_DICTID;
 *   FDICT set, dict_len == 0         -- ZT_E_ZLIB_FDICT 'fdict flag is not supported'.
 * *end_ip: the position just past the DEFLATE stream. */
int zt_zlib_decompress_dict(const uint8_t *in, size_t n, size_t index, int verify, const uint8_t *dict,
                            size_t dict_len, uint8_t **out, size_t *out_len, size_t *end_ip, uint32_t *adler_out);

#ifdef __cplusplus
}
#endif
#endif
