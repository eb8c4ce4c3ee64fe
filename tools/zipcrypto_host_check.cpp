// tools/zipcrypto_host_check.cpp -- drives the host-only parts of the ZipCrypto
// path (zlib.ts_amd/csrc/zipcrypto.h: key setup, the encryption header, the
// span arithmetic of an encrypted entry) over an archive, without a device.
// Meant to be built with a sanitizer and run on its own:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -DZT_ZIPCRYPTO_HOST_ONLY -o zipcrypto_host_check tools/zipcrypto_host_check.cpp
//   ./zipcrypto_host_check tests/golden/streams/<archive>.bin <password as hex>
//
// For every encrypted entry it finds the cipher stream (also at every
// truncation of the archive, where the span must stay inside it), decrypts it
// with the serial cipher and checks the header bytes the reference writes
// (src/Zip.ts:169-174) and, for STORE entries, the CRC-32 of the plaintext.
// Prints "entries E encrypted N matched M"; exit 1 on a read error or a broken
// invariant.  (M < N: entries under another password.)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../zlib.ts_amd/csrc/zipcrypto.h"

using namespace zt::zc;

static uint32_t rd(const std::vector<uint8_t> &b, size_t p, int n) {
  uint32_t v = 0;
  for (int k = 0; k < n; ++k) v |= (p + k < b.size() ? (uint32_t)b[p + k] : 0u) << (8 * k);
  return v;
}

int main(int argc, char **argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s archive password-hex\n", argv[0]), 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 1;
  std::vector<uint8_t> a;
  uint8_t buf[4096];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) a.insert(a.end(), buf, buf + k);
  fclose(f);
  std::vector<uint8_t> pw;
  const std::string hx = argv[2];
  for (size_t i = 0; i + 1 < hx.size(); i += 2) pw.push_back((uint8_t)strtoul(hx.substr(i, 2).c_str(), nullptr, 16));
  const Keys key0 = create_key(pw.data(), pw.size());
  long eo = -1;
  for (long ip = (long)a.size() - 12; ip > 0; --ip)
    if (rd(a, (size_t)ip, 4) == 0x06054b50u) {
      eo = ip;
      break;
    }
  if (eo < 0) return fprintf(stderr, "no end record\n"), 1;
  const uint32_t total = rd(a, eo + 10, 2);
  size_t c = rd(a, eo + 16, 4);
  unsigned enc = 0, matched = 0;
  for (uint32_t i = 0; i < total; ++i) {
    if (rd(a, c, 4) != 0x02014b50u) return fprintf(stderr, "bad central signature\n"), 1;
    const uint32_t crc = rd(a, c + 16, 4), ccs = rd(a, c + 20, 4), loff = rd(a, c + 42, 4);
    const uint32_t nl = rd(a, c + 28, 2), xl = rd(a, c + 30, 2), cl = rd(a, c + 32, 2);
    c += 46 + nl + xl + cl;
    const uint32_t flags = rd(a, loff + 6, 2), method = rd(a, loff + 8, 2), lcs = rd(a, loff + 18, 4);
    const size_t doff = (size_t)loff + 30 + rd(a, loff + 26, 2) + rd(a, loff + 28, 2);
    if (!(flags & 1)) continue;
    ++enc;
    // the span stays inside every truncation of the archive
    for (size_t n = 0; n <= a.size(); n += (a.size() / 64) + 1) {
      size_t len = 0;
      const bool ok = encrypted_span(n, doff, lcs, ccs, &len);
      if ((doff <= n && doff + len > n) || (doff > n && len != 0) || (ok && len < 12)) return fprintf(stderr, "span\n"), 1;
    }
    size_t len = 0;
    if (!encrypted_span(a.size(), doff, lcs, ccs, &len)) continue;
    if (entry_data_len(true, len - 12) != len) return fprintf(stderr, "entry_data_len\n"), 1;
    Keys k = key0;
    std::vector<uint8_t> pt(len);
    for (size_t j = 0; j < len; ++j) {
      pt[j] = (uint8_t)(a[doff + j] ^ stream_byte(k));
      update_keys(k, pt[j]);
    }
    zt_zip_crypt zc{};
    uint8_t h[12];
    crypt_header(zc, crc, h);
    if (memcmp(h, pt.data(), 12) != 0) continue;  // another password
    if (method == 0) {
      uint32_t r = 0xFFFFFFFFu;
      for (size_t j = 12; j < len; ++j) r = crc_step_host(r, pt[j]);
      if ((r ^ 0xFFFFFFFFu) != crc) return fprintf(stderr, "entry %u: crc\n", i), 1;
    }
    // and encrypting the plaintext again gives the archive's bytes
    k = key0;
    for (size_t j = 0; j < len; ++j) {
      if ((uint8_t)(pt[j] ^ stream_byte(k)) != a[doff + j]) return fprintf(stderr, "entry %u: re-encrypt\n", i), 1;
      update_keys(k, pt[j]);
    }
    ++matched;
  }
  printf("entries %u encrypted %u matched %u\n", total, enc, matched);
  return 0;
}
