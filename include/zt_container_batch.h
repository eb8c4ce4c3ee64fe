/*
 * zt_container_batch.h -- the read side of the batched containers: many gzip
 * files or zlib streams decoded and verified per call.  The inverse of
 * zt_gzip_compress_batch, zt_zlib_compress_batch and
 * zt_zlib_compress_batch_dict.
 *
 * Like zt.h: plain C, synchronous, GPU only.  Per device, a batch is packed
 * and uploaded once, every member of every item is decoded by the batch
 * decoder, and the CRC-32 / Adler-32 of the decoded bytes is taken from their
 * device copy: no decoded byte goes back to the device.  All three calls
 * honour zt_set_devices (items split by longest processing time, one host
 * thread per device, a dictionary copied once per device).
 *
 * Per item, the output bytes, the member fields, the status and the message
 * are what the single call on that item alone gives (zt_gunzip,
 * zt_zlib_decompress, zt_zlib_decompress_dict), with its order of checks.  A
 * failed item leaves out[i] = NULL, out_len[i] = 0, nmembers[i] = 0 and its
 * code in status[i]; the other items still decode.  The call returns the
 * first failing item's code with its message set (zt_last_error_message);
 * every item's message: zt_container_batch_message.  count == 0 returns
 * ZT_OK.  out[i] and members[i] are library memory released with zt_free;
 * outputs may share slabs, as zt_inflate_raw_batch's do.
 *
 * Limits.  A batch item decodes at the one-wave-per-member rate, like
 * zt_inflate_raw_batch and zt_unzip: the right shape for many small and
 * medium files, and for files of many members (bgzip, `cat a.gz b.gz`, this
 * engine's members joined).  One huge single-member file belongs to
 * zt_gunzip / zt_zlib_decompress, which decode one stream with the whole
 * device.
 */
#ifndef ZT_CONTAINER_BATCH_H
#define ZT_CONTAINER_BATCH_H
#include "zt_dict.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A loop of new GUnzip(in[i]).decompress() + getMembers()  src/GUnzip.ts:53-175.
 * members / nmembers: either may be NULL.  members[i][k].data_off indexes
 * out[i]; name_off / comment_off index in[i].
 *
 * Member starts are found on the device: every position where 1F 8B 08 starts
 * is a candidate (the reference checks no more), all candidates are decoded
 * in one batch, and the host follows each item's chain from offset 0, so
 * candidates inside data, comments or FEXTRA are never used. */
int zt_gunzip_batch(const uint8_t *const *in, const size_t *n, size_t count, uint8_t **out, size_t *out_len,
                    zt_gzip_member **members, size_t *nmembers, int *status);

/* A loop of new Inflate(in[i], {index: index[i], verify}).decompress()  src/Inflate.ts:34-93.
 * index, end_ip, adler_out may be NULL (index: every stream starts at 0).
 * adler_out[i]: the output's Adler-32 when verify is set, else 1. */
int zt_zlib_decompress_batch(const uint8_t *const *in, const size_t *n, const size_t *index, size_t count,
                             int verify, uint8_t **out, size_t *out_len, size_t *end_ip, uint32_t *adler_out,
                             int *status);

/* The same with one dictionary for the batch: per item the four FDICT cases
 * of zt_zlib_decompress_dict.  Items with FDICT decode with the dictionary
 * (one wavefront per stream), items without it as zt_zlib_decompress_batch
 * decodes them, in the same call. */
int zt_zlib_decompress_batch_dict(const uint8_t *const *in, const size_t *n, const size_t *index, size_t count,
                                  int verify, const uint8_t *dict, size_t dict_len, uint8_t **out, size_t *out_len,
                                  size_t *end_ip, uint32_t *adler_out, int *status);

/* Message of item i in this thread's last call of one of the three functions
 * above ("" for an item that decoded, or an index past that call's count).
 * Valid until this thread's next such call. */
const char *zt_container_batch_message(size_t i);

typedef struct {
  uint64_t items;         /* items of the call */
  uint64_t candidates;    /* member starts tested: every item's offset 0 and every 1F 8B 08 found */
  uint64_t members;       /* members accepted on the items' chains */
  uint64_t decode_passes; /* batch decode calls */
  uint64_t redecoded;     /* streams decoded after the first pass: members that outgrew their bound, starts that were not in the candidate list */
} zt_gunzip_batch_stats;

/* This thread's last zt_gunzip_batch call, summed over its devices. */
int zt_gunzip_batch_last_stats(zt_gunzip_batch_stats *out);

#ifdef __cplusplus
}
#endif
#endif
