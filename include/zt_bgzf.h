/*
 * zt_bgzf.h -- BGZF (blocked gzip, SAM spec 4.1) for libzt.so: the writer, an
 * exact one-pass reader, byte-range and virtual-offset reads that upload and
 * decode only the blocks they touch, and the .gzi index.
 *
 * A BGZF file is a chain of independent gzip members ("blocks") of at most
 * 64 KiB, each stating its own size in an extra field, closed by a fixed
 * 28-byte empty block.  All integers little endian:
 *
 *    0  ID1=31 ID2=139 CM=8 FLG=4
 *    4  MTIME=0 (u32)   8 XFL=0   9 OS=255
 *   10  XLEN=6 (u16)
 *   12  SI1='B' SI2='C' SLEN=2 (u16)
 *   16  BSIZE (u16) = total block size - 1
 *   18  CDATA: one complete raw DEFLATE stream (BSIZE - XLEN - 19 bytes)
 *   ..  CRC32 (u32) of the block's uncompressed bytes
 *   ..  ISIZE (u32), 0..65536
 *
 * A reader addresses data by *virtual offset*: coffset << 16 | uoffset, where
 * coffset (< 2^48) is a block's start in the file and uoffset a position
 * inside that block's uncompressed bytes.
 *
 * .gzi: u64 N, then N pairs (u64 compressed_offset, u64 uncompressed_offset).
 * The writer emits one pair for every block with ISIZE > 0 after the first
 * such block, in file order.  The reader accepts any .gzi whose pairs are
 * block starts of the file with the right cumulative ISIZE (pairs for empty
 * blocks or the end marker included).  The index is a hint that is verified:
 * every pair a call uses is checked against the file's own BSIZE chain.
 *
 * Like zt.h: plain C, synchronous, GPU only (zt_bgzf_index alone is a host
 * walk and touches no device).  The calls run on the calling thread's device
 * (zt_set_devices does not apply).  Outputs are library memory: zt_free.
 *
 * Not covered here: multi-GPU and device-resident forms; BAM, tabix or BAI
 * parsing (callers bring virtual offsets); repair of damaged files; block
 * sizes below 4096; an engine-native index for BGZF.  zt_gunzip and
 * zt_gunzip_batch are unchanged: they keep decoding BGZF files as plain
 * multi-member gzip.
 */
#ifndef ZT_BGZF_H
#define ZT_BGZF_H
#include "zt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZT_E_BGZF_FORMAT -70 /* 'not a BGZF block at offset N: <reason>' (also: truncated inside a block) */
#define ZT_E_BGZF_INDEX  -71 /* the .gzi blob is malformed or does not fit the file */

/* the largest (and default) input slice of one block; with it a block is at
 * most 65326 bytes */
#define ZT_BGZF_BLOCK_MAX 65280

typedef struct {
  zt_deflate_opts deflate;
  uint32_t block_size;   /* 0: 65280; else 4096..65280, otherwise ZT_E_ARG */
} zt_bgzf_opts;

typedef struct {
  uint64_t blocks;       /* blocks in the file, empty ones and markers included */
  uint64_t data_blocks;  /* blocks with ISIZE > 0 */
  uint64_t total_out;    /* sum of ISIZE */
  uint64_t error_offset; /* on failure: the file offset of the block that failed */
  int has_eof;           /* the file ends with the 28-byte marker */
} zt_bgzf_info;

/* Block k holds in[k * bs, min(n, (k + 1) * bs)), block k's CDATA being
 * byte-identical to element k of zt_deflate_raw_batch over the same slices
 * with the same options; the 28-byte marker follows the last block (n == 0:
 * the marker alone).  gzi / gzi_len (either or both may be NULL): the file's
 * .gzi, byte-identical to what zt_bgzf_index returns for *out.  A block that
 * would exceed 65536 bytes (fixed codes over incompressible bytes) is
 * ZT_E_INTERNAL; it is never written with a truncated BSIZE. */
int zt_bgzf_compress(const uint8_t *in, size_t n, const zt_bgzf_opts *opts, uint8_t **out, size_t *out_len,
                     uint8_t **gzi, size_t *gzi_len);

/* The .gzi of a file and its summary (info may be NULL), from a host walk of
 * the BSIZE chain and the trailers: no device is touched and no payload is
 * decoded.  ZT_E_BGZF_FORMAT (info->error_offset: the offending block) for a
 * file that is not a chain of BGZF blocks. */
int zt_bgzf_index(const uint8_t *in, size_t n, uint8_t **gzi, size_t *gzi_len, zt_bgzf_info *info);

/* The whole file, every block decoded once and checked against its ISIZE and
 * CRC-32 on the device.  n == 0 is an empty file (empty output, has_eof 0); a
 * missing final marker is not an error (has_eof 0); a marker in the middle
 * (cat a.bgz b.bgz) is an ordinary empty block.  A block whose payload fails
 * returns the code and message zt_gunzip gives for that block's bytes alone
 * (the inflate status, ZT_E_GZIP_CRC32 or ZT_E_GZIP_ISIZE) with
 * info->error_offset its start; the first failing block in file order wins
 * and there is no output. */
int zt_bgzf_decompress(const uint8_t *in, size_t n, uint8_t **out, size_t *out_len, zt_bgzf_info *info);

/* `count` ranges by uncompressed offset, pread style, as zt_inflate_ranges
 * documents: off > total is ZT_E_ARG, len is clamped, unsorted, overlapping
 * and repeated ranges are fine, no block is uploaded or decoded twice, the
 * outputs share one allocation (release each with zt_free).  gzi == NULL: the
 * chain is walked on the host for this call.  status[i] receives each range's
 * code and the call returns the first failing one.  Blocks are independent:
 * a range fails only if a block it touches fails. */
int zt_bgzf_read_ranges(const uint8_t *in, size_t n, const uint8_t *gzi, size_t gzi_len, const uint64_t *off,
                        const uint64_t *len, size_t count, uint8_t **out, size_t *out_len, int *status);

/* The bytes from virtual offset vbeg[i] up to vend[i], as tabix and BAI chunks
 * are given.  Only the chain from vbeg's block to vend's block is walked.  A
 * coffset that is not a valid block start is ZT_E_BGZF_FORMAT; a uoffset
 * greater than its block's ISIZE, or vend < vbeg, is ZT_E_ARG; vbeg == vend
 * returns empty without touching the GPU. */
int zt_bgzf_read_virtual(const uint8_t *in, size_t n, const uint64_t *vbeg, const uint64_t *vend, size_t count,
                         uint8_t **out, size_t *out_len, int *status);

/* Work counters of the two read calls above, process-wide, counted whether
 * timing is on or not. */
typedef struct {
  uint64_t range_calls;        /* zt_bgzf_read_ranges / _virtual calls that reached the device */
  uint64_t ranges;             /* ranges and chunks asked for (empty ones included) */
  uint64_t blocks_decoded;     /* blocks the calls decoded */
  uint64_t in_bytes_uploaded;  /* bytes of those blocks (whole blocks, header and trailer included) */
  uint64_t out_bytes_decoded;  /* bytes the calls decoded on the device */
  uint64_t out_bytes_returned; /* bytes the calls returned */
} zt_bgzf_stats;
int zt_bgzf_stats_read(zt_bgzf_stats *out, int reset);

#ifdef __cplusplus
}
#endif
#endif
