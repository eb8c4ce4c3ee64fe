// member_frame.h -- a gzip, zlib or raw member is prefix | DEFLATE body |
// trailer, and this is the one place that knows the bytes: the frame's
// description, the constructors of every prefix the library writes, the
// trailer writer (host and device: the framing kernels of member_frame.hip
// call it too) and the stored blocks of compression type NONE.  No HIP
// includes; checked on the CPU under ASan / UBSan by
// tools/member_frame_host_check.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/zt.h"
#include "bgzf_host.h"     // bgzf_eof_marker
#include "gunzip_chain.h"  // crc32_small

#ifdef __HIP__
#define ZT_HOST_DEVICE __host__ __device__
#else
#define ZT_HOST_DEVICE
#endif

namespace zt {

// (the values of ZT_DEV_BATCH_RAW / ZLIB / GZIP, include/zt_dev_batch.h)
enum MemberKind { kFmtRaw = 0, kFmtZlib = 1, kFmtGzip = 2 };

// gzip: CRC-32 and ISIZE, little endian (src/GZip.ts:179-185); zlib: Adler-32,
// big endian (src/Deflate.ts:95); raw: nothing
ZT_HOST_DEVICE inline uint32_t member_trailer_len(MemberKind kind) {
  return kind == kFmtGzip ? 8u : kind == kFmtZlib ? 4u : 0u;
}
ZT_HOST_DEVICE inline void put_trailer(uint8_t *t, MemberKind kind, uint32_t crc, uint32_t adler, uint32_t isize) {
  if (kind == kFmtGzip) {
    for (int k = 0; k < 4; ++k) t[k] = (uint8_t)(crc >> (8 * k));
    for (int k = 0; k < 4; ++k) t[4 + k] = (uint8_t)(isize >> (8 * k));
  } else if (kind == kFmtZlib) {
    for (int k = 0; k < 4; ++k) t[k] = (uint8_t)(adler >> (24 - 8 * k));
  }
}

struct MemberFrame {
  MemberKind kind;
  std::vector<uint8_t> prefix;
  uint32_t prefix_len() const { return (uint32_t)prefix.size(); }
  uint32_t trailer_len() const { return member_trailer_len(kind); }
};

// RFC 1950: CMF = 0x78 (deflate, 32 KiB window); FLG: FLEVEL in bits 6-7 (the
// caller's compression type, src/Deflate.ts:61-78), FDICT 0x20, FCHECK so that
// CMF * 256 + FLG is a multiple of 31
inline std::vector<uint8_t> zlib_cmf_flg(uint32_t flevel, bool fdict) {
  const uint32_t cmf = 0x78, flg0 = ((flevel & 3u) << 6) | (fdict ? 0x20u : 0u);
  const uint32_t rem = ((cmf << 8) + flg0) % 31;
  return {(uint8_t)cmf, (uint8_t)(flg0 | (rem ? 31 - rem : 0))};
}

inline MemberFrame frame_raw() { return MemberFrame{kFmtRaw, {}}; }
inline MemberFrame frame_zlib(uint32_t flevel) { return MemberFrame{kFmtZlib, zlib_cmf_flg(flevel, false)}; }
// FDICT: DICTID big endian behind the two bytes
inline MemberFrame frame_zlib_dict(uint32_t flevel, uint32_t dictid) {
  MemberFrame f{kFmtZlib, zlib_cmf_flg(flevel, true)};
  for (int k = 0; k < 4; ++k) f.prefix.push_back((uint8_t)(dictid >> (24 - 8 * k)));
  return f;
}
// member header: src/GZip.ts:104-158 (null: the fixed 10 bytes)
inline MemberFrame frame_gzip(const zt_gzip_opts *opts) {
  MemberFrame f{kFmtGzip, {0x1F, 0x8B, 8}};
  std::vector<uint8_t> &hd = f.prefix;
  uint8_t flg = 0;
  if (opts && opts->fname) flg |= 0x08;
  if (opts && opts->fcomment) flg |= 0x10;
  if (opts && opts->fhcrc) flg |= 0x02;
  hd.push_back(flg);
  const uint32_t mtime = opts ? opts->mtime : 0;
  for (int k = 0; k < 4; ++k) hd.push_back((mtime >> (8 * k)) & 0xFF);
  hd.push_back(0);  // XFL
  hd.push_back(3);  // OS: UNIX (src/GZip.ts:128)
  if (opts && opts->fname) {
    hd.insert(hd.end(), opts->name, opts->name + opts->name_len);
    hd.push_back(0);
  }
  if (opts && opts->fcomment) {
    hd.insert(hd.end(), opts->comment, opts->comment + opts->comment_len);
    hd.push_back(0);
  }
  if (opts && opts->fhcrc) {
    const uint32_t c16 = crc32_small(hd.data(), hd.size()) & 0xFFFF;
    hd.push_back(c16 & 0xFF);
    hd.push_back(c16 >> 8);
  }
  return f;
}
// a BGZF block: the end marker's 18 header bytes (the writer patches BSIZE)
inline MemberFrame frame_bgzf() {
  return MemberFrame{kFmtGzip, std::vector<uint8_t>(bgzf_eof_marker(), bgzf_eof_marker() + kBgzfHeaderBytes)};
}
// the frame of a format of the device-resident batch (zt_dev_batch.h): no
// gzip options; flevel as zt_zlib_compress_batch writes it
inline MemberFrame frame_of(MemberKind kind, uint32_t flevel) {
  return kind == kFmtGzip ? frame_gzip(nullptr) : kind == kFmtZlib ? frame_zlib(flevel) : frame_raw();
}

// ---- stored blocks (compression type NONE, level 0; the empty input) ----------------
// the 5 header bytes of a stored block of l <= 65535 bytes, little endian in a word
inline uint64_t stored_header(uint32_t l, bool last) {
  return (uint64_t)(last ? 1 : 0) | (uint64_t)(l & 0xFFFF) << 8 | (uint64_t)(~l & 0xFFFF) << 24;
}
// n bytes as stored blocks of <= 65535 bytes (src/RawDeflate.ts:93-100,122-153);
// the empty input is one final empty block
inline size_t stored_len(size_t n) { return n ? n + 5 * ((n + 65534) / 65535) : 5; }
// the blocks themselves: stored_len(n) bytes at dst, BFINAL on the last
inline void stored_write(const uint8_t *src, uint64_t n, uint8_t *dst) {
  uint64_t p = 0;
  do {
    const uint32_t l = (uint32_t)(n - p < 65535 ? n - p : 65535);
    const uint64_t h = stored_header(l, p + l == n);
    for (int k = 0; k < 5; ++k) dst[k] = (uint8_t)(h >> (8 * k));
    if (l) memcpy(dst + 5, src + p, l);
    dst += 5 + (uint64_t)l;
    p += l;
  } while (p < n);
}

}  // namespace zt
