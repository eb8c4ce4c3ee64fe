// zipcrypto.h -- internal declarations of the ZipCrypto path (not installed).
//
// The first part is host-only and needs neither HIP nor a device (key setup,
// the encryption header, the size / offset arithmetic of an encrypted entry):
// a stand-alone program can include it (tools/zipcrypto_host_check.cpp).  The
// launchers of zipcrypto.hip follow unless ZT_ZIPCRYPTO_HOST_ONLY is defined.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/zt_zipcrypto.h"

namespace zt {
namespace zc {

constexpr uint32_t kChunk = 64;           // C: bytes one lane walks
constexpr uint32_t kLanes = 256;          // lanes of a tile's workgroup
constexpr uint32_t kTile = kChunk * kLanes;  // T = 16 KiB
constexpr uint32_t kMul = 134775813u;

struct Keys {
  uint32_t k[3];
};

// one step of the raw (reflected) CRC-32 register: CRC32.single, src/CRC32.ts
inline uint32_t crc_step_host(uint32_t c, uint32_t b) {
  c ^= b & 0xFF;
  for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
  return c;
}
// ZipCrypto.updateKeys (src/ZipCrypto.ts:24-29)
inline void update_keys(Keys &k, uint32_t p) {
  k.k[0] = crc_step_host(k.k[0], p);
  k.k[1] = (k.k[1] + (k.k[0] & 0xFF)) * kMul + 1;
  k.k[2] = crc_step_host(k.k[2], k.k[1] >> 24);
}
// ZipCrypto.getByte (src/ZipCrypto.ts:13-17)
inline uint32_t stream_byte(const Keys &k) {
  const uint32_t t = (k.k[2] & 0xFFFF) | 2;
  return ((t * (t ^ 1)) >> 8) & 0xFF;
}
// ZipCrypto.createKey (src/ZipCrypto.ts:35-45)
inline Keys create_key(const uint8_t *pw, size_t n) {
  Keys k{{305419896u, 591751049u, 878082192u}};
  for (size_t i = 0; i < n; ++i) update_keys(k, pw[i]);
  return k;
}
// plaintext of the 12-byte encryption header: src/Zip.ts:169-174 (mode 0) or
// APPNOTE 6.1.6 as other tools check it (mode 1: the CRC's two high bytes)
inline void crypt_header(const zt_zip_crypt &c, uint32_t crc, uint8_t h[12]) {
  memcpy(h, c.lead, 10);
  if (c.header_mode == 1) {
    h[10] = (crc >> 16) & 0xFF;
    h[11] = (crc >> 24) & 0xFF;
  } else {
    h[10] = (crc >> 8) & 0xFF;
    h[11] = crc & 0xFF;
  }
}
// bytes an entry's data takes in the archive
inline size_t entry_data_len(bool encrypted, size_t body_len) { return body_len + (encrypted ? 12 : 0); }

// Where an encrypted entry's cipher stream lies in an archive of n bytes: the
// local compressed size, or the central directory's when the local one is 0
// (data descriptor).  Returns false when the stream is shorter than its
// 12-byte header ('invalid encryption header size'); *len is clipped to the
// archive.
inline bool encrypted_span(size_t n, size_t data_off, uint32_t local_csize, uint32_t central_csize, size_t *len) {
  size_t cs = local_csize ? local_csize : central_csize;
  if (data_off > n) data_off = n;
  if (cs > n - data_off) cs = n - data_off;
  *len = cs;
  return cs >= 12;
}

// One batch through the device (zipcrypto_api.cpp): item i is head (the 12
// bytes of an entry's encryption header, or none) then body, under keys[i];
// the result goes to dst[i] (head_len + body_len bytes, the caller's memory).
struct Src {
  const uint8_t *head;
  size_t head_len;
  const uint8_t *body;
  size_t body_len;
};
int crypt_items(bool encrypt, const Src *src, const Keys *keys, size_t count, uint8_t *const *dst);

}  // namespace zc
}  // namespace zt

#ifndef ZT_ZIPCRYPTO_HOST_ONLY
#include <hip/hip_runtime.h>
namespace zt {
namespace zc {

// encrypt: streams packed from tile boundaries; tile t's bytes at data + t * kTile
struct Tile {
  uint32_t item;
  uint32_t len;  // bytes of the stream in this tile (kTile for all but an item's last)
};
struct Item {
  uint64_t first_tile;
  uint64_t ntiles;
  uint32_t key[3];
  uint32_t pad;
};
// decrypt: one lane per stream, in place at data + off
struct Stream {
  uint64_t off;
  uint64_t len;
  uint32_t key[3];
  uint32_t pad;
};
// device work memory of an encrypt of ntiles tiles
size_t encrypt_work_bytes(size_t ntiles);
// in place over the packed tiles; every pointer is device memory
int encrypt_dev(uint8_t *d_data, const Tile *d_tiles, size_t ntiles, const Item *d_items, size_t nitems,
                void *d_work, hipStream_t s);
int decrypt_dev(uint8_t *d_data, const Stream *d_streams, size_t count, hipStream_t s);

}  // namespace zc
}  // namespace zt
#endif
