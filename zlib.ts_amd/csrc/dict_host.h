// dict_host.h -- host-only arithmetic of the preset-dictionary calls
// (include/zt_dict.h): which bytes of a dictionary the engines use, where they
// sit in the match kernel's history, and the checks of the RFC 1950 header
// (its writer: member_frame.h).  No device code and no HIP types:
// tools/dict_host_check.cpp runs it under ASan / UBSan.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/zt.h"

namespace zt {

// deflate: match distances end at DF_MAXDIST (deflate.hip), so only that much
// of a dictionary's end can be a match source; the history is loaded in whole
// sub-chunks of DF_SUB bytes
constexpr uint32_t kDictMaxTail = 28352;
constexpr uint32_t kDictSub = 4096;
// inflate: RFC 1951 distances reach 32768 back
constexpr uint32_t kDictWindow = 32768;

// History of a dictionary stream's first match workgroup: `hist` bytes (a
// multiple of kDictSub), of which the first `floor` are zero padding and the
// last `tail` = hist - floor are dict[dict_len - tail .. dict_len).
struct DictLayout {
  uint32_t tail;   // dictionary bytes used, min(dict_len, kDictMaxTail)
  uint32_t hist;   // round_up(tail, kDictSub); 0 without a dictionary
  uint32_t floor;  // hist - tail < kDictSub: rel positions below it are never match sources
  size_t src_off;  // dict_len - tail: first dictionary byte used
};

inline DictLayout dict_layout(size_t dict_len) {
  DictLayout L;
  L.tail = dict_len < kDictMaxTail ? (uint32_t)dict_len : kDictMaxTail;
  L.hist = (L.tail + kDictSub - 1) / kDictSub * kDictSub;
  L.floor = L.hist - L.tail;
  L.src_off = dict_len - L.tail;
  return L;
}

// dst[0 .. L.hist) := padding | tail (dst holds L.hist bytes)
inline void dict_fill_history(const DictLayout &L, const uint8_t *dict, uint8_t *dst) {
  if (L.floor) memset(dst, 0, L.floor);
  if (L.tail) memcpy(dst + L.floor, dict + L.src_off, L.tail);
}

// inflate: the decoder's history is the last kDictWindow bytes
inline size_t dict_window_off(size_t dict_len) { return dict_len > kDictWindow ? dict_len - kDictWindow : 0; }
inline uint32_t dict_window_len(size_t dict_len) { return dict_len > kDictWindow ? kDictWindow : (uint32_t)dict_len; }

// Header of the zlib stream at in[index ..): the checks of src/Inflate.ts:44-58
// in their order, then DICTID when FDICT is set.
enum ZlibHdr {
  ZH_OK = 0,
  ZH_METHOD,     // CMF missing or not deflate
  ZH_FCHECK_NAN, // FLG missing
  ZH_FCHECK,     // (CMF * 256 + FLG) % 31 != 0, the remainder in `fcheck`
  ZH_BROKEN,     // FDICT set and fewer than 4 bytes of DICTID
};
struct ZlibHeader {
  int fdict;
  int fcheck;
  uint32_t dictid;
  size_t body;  // index of the first DEFLATE byte
};
inline ZlibHdr zlib_parse_header(const uint8_t *in, size_t n, size_t index, ZlibHeader *h) {
  h->fdict = 0;
  h->fcheck = 0;
  h->dictid = 0;
  h->body = index;
  if (index >= n || (in[index] & 0x0F) != 8) return ZH_METHOD;
  if (index + 1 >= n) return ZH_FCHECK_NAN;
  const uint32_t cmf = in[index], flg = in[index + 1];
  if (((cmf << 8) + flg) % 31 != 0) {
    h->fcheck = (int)(((cmf << 8) + flg) % 31);
    return ZH_FCHECK;
  }
  h->body = index + 2;
  if (flg & 0x20) {
    h->fdict = 1;
    if (n - (index + 2) < 4) return ZH_BROKEN;
    for (int k = 0; k < 4; ++k) h->dictid = (h->dictid << 8) | in[index + 2 + k];
    h->body = index + 6;
  }
  return ZH_OK;
}
// The reference's status and message for the three header results (true: the
// header is refused).  What follows -- FDICT without a dictionary, ZH_BROKEN,
// the dictionary id -- is each caller's own, in its own order.
inline bool zlib_header_status(ZlibHdr hs, const ZlibHeader &h, int *code, std::string *msg) {
  if (hs != ZH_METHOD && hs != ZH_FCHECK_NAN && hs != ZH_FCHECK) return false;
  *code = hs == ZH_METHOD ? ZT_E_ZLIB_METHOD : ZT_E_ZLIB_FCHECK;
  *msg = hs == ZH_METHOD       ? "unsupported compression method"
         : hs == ZH_FCHECK_NAN ? "invalid fcheck flag:NaN"
                               : "invalid fcheck flag:" + std::to_string(h.fcheck);
  return true;
}

}  // namespace zt
