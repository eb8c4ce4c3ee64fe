// tools/dict_host_check.cpp -- drives the host-only arithmetic of the preset
// dictionary calls (zlib.ts_amd/csrc/dict_host.h) without a device: which
// bytes of a dictionary the engines use and where they sit in the match
// kernel's history, and the RFC 1950 FDICT header with its DICTID.  Meant to
// be built with a sanitizer and run on its own (tests/test_dict_host.py):
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o dict_host_check tools/dict_host_check.cpp
//   ./dict_host_check
//
// Every buffer is a heap allocation of exactly the bytes the code may touch,
// so a read or write outside it stops the run.  Prints "dict_host_check ok";
// exit 1 on a broken invariant.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../zlib.ts_amd/csrc/dict_host.h"
#include "../zlib.ts_amd/csrc/member_frame.h"  // frame_zlib_dict: the FDICT header's writer

using namespace zt;

static int fails = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);            \
      ++fails;                                                   \
    }                                                            \
  } while (0)

static uint32_t adler32(const uint8_t *p, size_t n) {
  uint32_t a = 1, b = 0;
  for (size_t i = 0; i < n; ++i) {
    a = (a + p[i]) % 65521;
    b = (b + a) % 65521;
  }
  return b << 16 | a;
}

int main() {
  const size_t lens[] = {0, 1, 4095, 4096, 28352, 28353, 32768, 100000};
  for (size_t n : lens) {
    std::vector<uint8_t> dict(n);
    for (size_t i = 0; i < n; ++i) dict[i] = (uint8_t)(1 + (i * 2654435761u >> 13) % 255);  // never 0
    // ---- the deflate history ----
    const DictLayout L = dict_layout(n);
    CHECK(L.tail == (n < kDictMaxTail ? n : kDictMaxTail));
    CHECK(L.hist % kDictSub == 0 && L.hist >= L.tail && L.hist - L.tail < kDictSub);
    CHECK(L.hist <= 28672);  // DF_HIST: what a match workgroup can load
    CHECK(L.floor == L.hist - L.tail && L.src_off + L.tail == n);
    CHECK((n == 0) == (L.hist == 0));
    std::vector<uint8_t> img(L.hist);
    dict_fill_history(L, dict.data(), img.data());
    for (uint32_t r = 0; r < L.hist; ++r) {
      // rel r of the first workgroup: padding below the floor, then the tail;
      // the stream's byte k is rel hist + k, so its distance to the oldest
      // usable byte is at most tail + k
      if (r < L.floor)
        CHECK(img[r] == 0);
      else
        CHECK(img[r] == dict[n - (L.hist - r)]);
    }
    // ---- the inflate window ----
    const size_t wo = dict_window_off(n);
    const uint32_t wl = dict_window_len(n);
    CHECK(wo + wl == n && wl <= kDictWindow && (n <= kDictWindow ? wo == 0 : wl == kDictWindow));
    std::vector<uint8_t> win(dict.begin() + (long)wo, dict.begin() + (long)(wo + wl));
    CHECK(win.size() == wl && (wl == 0 || win.back() == dict.back()));
    // ---- the FDICT header ----
    const uint32_t id = adler32(dict.data(), n);
    for (uint32_t flevel = 0; flevel < 4; ++flevel) {
      const std::vector<uint8_t> hd = frame_zlib_dict(flevel, id).prefix;
      CHECK(hd.size() == 6);
      CHECK(hd[0] == 0x78 && (hd[1] & 0x20) && (hd[1] >> 6) == flevel && ((hd[0] << 8) + hd[1]) % 31 == 0);
      CHECK(((uint32_t)hd[2] << 24 | (uint32_t)hd[3] << 16 | (uint32_t)hd[4] << 8 | hd[5]) == id);
      // parsed back, whole and at every truncation (0..5 bytes) and offset
      for (size_t pre = 0; pre < 3; ++pre) {
        for (size_t keep = 0; keep <= 6; ++keep) {
          std::vector<uint8_t> in(pre + keep, 0xEE);
          for (size_t k = 0; k < keep; ++k) in[pre + k] = hd[k];
          ZlibHeader h;
          const ZlibHdr rc = zlib_parse_header(in.data(), in.size(), pre, &h);
          if (keep == 0)
            CHECK(rc == ZH_METHOD && !h.fdict);
          else if (keep == 1)
            CHECK(rc == ZH_FCHECK_NAN && !h.fdict);
          else if (keep < 6)
            CHECK(rc == ZH_BROKEN && h.fdict == 1 && h.body == pre + 2);
          else
            CHECK(rc == ZH_OK && h.fdict == 1 && h.dictid == id && h.body == pre + 6);
        }
      }
    }
  }
  // headers without FDICT, a wrong method and a wrong FCHECK
  {
    const uint8_t plain[2] = {0x78, 0x9C};
    ZlibHeader h;
    CHECK(zlib_parse_header(plain, 2, 0, &h) == ZH_OK && !h.fdict && h.body == 2);
    const uint8_t meth[2] = {0x77, 0x9C};
    CHECK(zlib_parse_header(meth, 2, 0, &h) == ZH_METHOD);
    const uint8_t fchk[2] = {0x78, 0x9D};
    CHECK(zlib_parse_header(fchk, 2, 0, &h) == ZH_FCHECK && h.fcheck == (0x789D % 31));
    CHECK(zlib_parse_header(plain, 2, 5, &h) == ZH_METHOD);  // index past the end
  }
  if (fails) return fprintf(stderr, "dict_host_check: %d checks failed\n", fails), 1;
  printf("dict_host_check ok\n");
  return 0;
}
