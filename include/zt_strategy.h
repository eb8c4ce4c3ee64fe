/* zt_strategy.h -- deflate strategies: zlib's Z_RLE and Z_HUFFMAN_ONLY.
 *
 * A strategy replaces the hash-chain match search, the kernel that bounds
 * deflate, by a streaming producer of the same per-position match words; the
 * stages behind it (prices, parse, Huffman codes, encode, sync points,
 * restart markers) are the plain calls', so the streams keep every property
 * of theirs: any inflate decodes them, and this library's segment-parallel
 * inflate finds its restart markers.
 *
 *   ZT_STRATEGY_HUFFMAN_ONLY  no match at all: literals under the block's
 *                             Huffman code.  For decorrelated or nearly
 *                             incompressible data.
 *   ZT_STRATEGY_RLE           matches at distance 1 only (runs of one byte).
 *                             For filtered image rows (PNG, TIFF), delta-coded
 *                             columns, sparse tensors.
 *
 * The RLE match offered at stream position i (B = 32768, the block size; n =
 * the stream's length; a run never reaches back over the start of the stream,
 * of the halo, or -- from the second on -- of i's 1 MiB restart segment):
 *   run_end(i) = the smallest j > i with byte[j] != byte[i], or n
 *   cap(i)     = min(258, (i / B + 1) * B - i, n - i)
 *   L(i)       = min(cap(i), run_end(i) - i) when byte[i] == byte[i - 1], else 0;
 *                L(i) < 3 counts as 0
 * The parse takes, at the positions it visits, a length 3 <= l <= L(i) or a
 * literal, as it does with the search's matches.
 *
 * Each entry point mirrors the plain call of the same name and adds `strategy`:
 *   - a value other than the three below: ZT_E_ARG, "invalid strategy: N",
 *     before any device work;
 *   - ZT_STRATEGY_DEFAULT: the plain call, byte for byte;
 *   - compression_type 0 or level 0 still writes stored blocks;
 *     compression_type 1 (fixed codes) and 2 (best of stored / fixed /
 *     dynamic) work with both strategies;
 *   - `level` keeps its meaning for the parse (lazy / cost-based from 4 on;
 *     levels 1..3 write identical streams) and none for the producer; the
 *     zlib FLEVEL byte is the plain call's;
 *   - the ZT_DF_PARAMS / ZT_DF_ADAPT / ZT_DF_MQ / ZT_DF_HEADS search hooks
 *     have no effect on the strategies' kernel.
 *
 * Not covered: preset dictionaries (zt_dict.h), the indexed writers
 * (zt_index.h), BGZF (zt_bgzf.h), Zip (zt_zip_compress) and
 * zt_deflate_dev_batch (zt_dev_batch.h).  None of those calls takes a
 * strategy, so a strategy cannot reach them.
 */
#ifndef ZT_STRATEGY_H
#define ZT_STRATEGY_H

#include "zt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* zlib's numbers (Z_DEFAULT_STRATEGY, Z_HUFFMAN_ONLY, Z_RLE); Z_FILTERED (1)
 * and Z_FIXED (4: compression_type 1 here) are not strategies of this library */
#define ZT_STRATEGY_DEFAULT 0
#define ZT_STRATEGY_HUFFMAN_ONLY 2
#define ZT_STRATEGY_RLE 3

int zt_deflate_raw_strategy(const uint8_t *in, size_t n, const zt_deflate_opts *opts, int strategy, uint8_t **out,
                            size_t *out_len);
int zt_deflate_raw_batch_strategy(const uint8_t *const *in, const size_t *n, size_t count,
                                  const zt_deflate_opts *opts, int strategy, uint8_t **out, size_t *out_len,
                                  int *status);
int zt_zlib_compress_strategy(const uint8_t *in, size_t n, const zt_deflate_opts *opts, int strategy, uint8_t **out,
                              size_t *out_len, uint32_t *adler_out);
int zt_gzip_compress_strategy(const uint8_t *in, size_t n, const zt_gzip_opts *opts, int strategy, uint8_t **out,
                              size_t *out_len, uint32_t *crc_out);
int zt_zlib_compress_batch_strategy(const uint8_t *const *in, const size_t *n, size_t count,
                                    const zt_deflate_opts *opts, int strategy, uint8_t **out, size_t *out_len,
                                    int *status);
int zt_gzip_compress_batch_strategy(const uint8_t *const *in, const size_t *n, size_t count, const zt_gzip_opts *opts,
                                    int strategy, uint8_t **out, size_t *out_len, int *status);
/* The strategy of every later zt_deflate_dev call through `plan` (halo and
 * final == 0 forms included; a plan starts with ZT_STRATEGY_DEFAULT).  With a
 * halo whose first byte is not 16-byte aligned the kernel reads the input
 * bytewise: keep shards 16-byte aligned for full speed. */
int zt_deflate_plan_set_strategy(zt_deflate_plan *plan, int strategy);

#ifdef __cplusplus
}
#endif
#endif /* ZT_STRATEGY_H */
