/*
 * zt_zipcrypto.h -- ZipCrypto (the traditional PKWARE cipher) for libzt.so:
 * raw cipher streams and password-protected Zip / Unzip.
 *
 * Replaces src/ZipCrypto.ts and the password paths of src/Zip.ts:152-187,
 * 247-249 and src/Unzip.ts:263-282.  Encryption runs as prefix scans over the
 * known plaintext (every lane of the GPU works on one stream); decryption is
 * serial per stream, so its parallelism is the entries of an archive (one lane
 * per stream).  Like zt.h: plain C, synchronous, GPU only (ZT_E_NO_DEVICE
 * without one).  The library draws no randomness: every output is a function
 * of the arguments.
 */
#ifndef ZT_ZIPCRYPTO_H
#define ZT_ZIPCRYPTO_H
#include "zt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Raw cipher streams (no container).  Stream i is in[i][0 .. n[i]) under the
 * key of password pw[i][0 .. pw_len[i]) (ZipCrypto.createKey, then encode /
 * decode per byte: src/ZipCrypto.ts:35-69).  out[i] receives n[i] bytes of
 * library memory (zt_free each; never NULL on success). */
int zt_zipcrypto_encrypt_batch(const uint8_t *const *in, const size_t *n, size_t count, const uint8_t *const *pw,
                               const size_t *pw_len, uint8_t **out);
int zt_zipcrypto_decrypt_batch(const uint8_t *const *in, const size_t *n, size_t count, const uint8_t *const *pw,
                               const size_t *pw_len, uint8_t **out);
/* Geometry of the encrypt kernels: a stream is cut into tiles of T bytes (one
 * workgroup each), a tile into per-lane chunks of C bytes. */
size_t zt_zipcrypto_tile_bytes(void);
size_t zt_zipcrypto_chunk_bytes(void);
/* Device time (HIP events around the kernels, ms) of this thread's last
 * zt_zipcrypto_*_batch call. */
int zt_zipcrypto_last_kernel_ms(double *ms);

typedef struct {
  const uint8_t *password; /* password == NULL: entry not encrypted */
  size_t password_len;
  int header_mode;         /* 0: reference (bytes 10,11 = crc>>8, crc);  1: PKWARE (crc>>16, crc>>24) */
  uint8_t lead[10];        /* plaintext of header bytes 0..9 (the reference writes zeros) */
} zt_zip_crypt;

/* zt_zip_compress with crypt[count] (or NULL: no entry encrypted):
 * src/Zip.ts:152-187,247-249.  An encrypted entry's data is E(header12 | body),
 * general-purpose flag bit 0 is set in both headers and the compressed size
 * counts the 12 header bytes. */
int zt_zip_compress_pw(const uint8_t *const *in, const size_t *n, const zt_zip_file *files,
                       const zt_zip_crypt *crypt, size_t count, const uint8_t *comment, size_t comment_len,
                       uint8_t **out, size_t *out_len);
/* zt_unzip with one password for the archive's encrypted entries
 * (src/Unzip.ts:263-282).  password == NULL: as zt_unzip (encrypted entries
 * get ZT_E_ZIP_ENCRYPTED).  The input is never written.  An encrypted entry
 * shorter than its 12-byte header: ZT_E_ZIP_FORMAT 'invalid encryption header
 * size'.  A wrong password shows as an inflate error or, under verify, as
 * ZT_E_ZIP_CRC. */
int zt_unzip_pw(const uint8_t *in, size_t n, int verify, const uint8_t *password, size_t password_len,
                uint8_t **out, size_t *out_len, zt_unzip_entry **entries, size_t *count);

#ifdef __cplusplus
}
#endif
#endif
