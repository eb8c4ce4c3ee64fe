// tools/gunzip_chain_check.cpp -- drives the host-only logic of the gzip read
// side (zlib.ts_amd/csrc/gunzip_chain.h) without a device: the member header
// and trailer checks, the input bound of a speculative candidate, and the walk
// of an item's member chain through hand-made candidate and decode tables.
// Meant to be built with a sanitizer and run on its own
// (tests/test_container_batch_host.py):
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o gunzip_chain_check tools/gunzip_chain_check.cpp
//   ./gunzip_chain_check
//
// Every input is a heap allocation of exactly its bytes, so a read outside it
// stops the run.  Prints "gunzip_chain_check ok"; exit 1 on a broken invariant.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../zlib.ts_amd/csrc/gunzip_chain.h"

using namespace zt;

static int fails = 0;
#define CHECK(c)                                      \
  do {                                                \
    if (!(c)) {                                       \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
      ++fails;                                        \
    }                                                 \
  } while (0)

typedef std::vector<uint8_t> Bytes;

static void put32(Bytes &b, uint32_t v) {
  for (int k = 0; k < 4; ++k) b.push_back((v >> (8 * k)) & 0xFF);
}

// A member whose "body" is `body` opaque bytes (the walk never decodes: the
// tables say what a decoder found), with the trailer of an output of out_len
// bytes and CRC-32 crc.
static Bytes member(size_t body, uint32_t crc, uint32_t out_len, uint8_t flg = 0, const Bytes &opt = Bytes()) {
  Bytes m = {0x1F, 0x8B, 8, flg, 1, 2, 3, 4, 0, 3};
  m.insert(m.end(), opt.begin(), opt.end());
  for (size_t i = 0; i < body; ++i) m.push_back((uint8_t)(0xA0 + i % 7));
  put32(m, crc);
  put32(m, out_len);
  return m;
}

static GzDecoded decoded(size_t start, size_t hdr, size_t body, size_t bound, uint32_t crc, size_t out_len,
                         size_t slot, int status = ZT_OK, int detail = 0) {
  GzDecoded d;
  d.start = start;
  d.bound = bound;
  d.status = status;
  d.detail = detail;
  d.end_ip = start + hdr + body;
  d.out_len = out_len;
  d.crc = crc;
  d.slot = slot;
  return d;
}

// exact-size heap copy (ASan sees every read past the item)
struct Item {
  uint8_t *p;
  size_t n;
  explicit Item(const Bytes &b) : p(b.empty() ? nullptr : (uint8_t *)malloc(b.size())), n(b.size()) {
    if (n) memcpy(p, b.data(), n);
  }
  ~Item() { free(p); }
};

static Bytes cat(std::initializer_list<Bytes> parts) {
  Bytes r;
  for (const Bytes &b : parts) r.insert(r.end(), b.begin(), b.end());
  return r;
}

int main() {
  const Bytes m0 = member(40, 0x11111111u, 100), m1 = member(25, 0x22222222u, 7), m2 = member(60, 0x33333333u, 0);
  const size_t s1 = m0.size(), s2 = m0.size() + m1.size();
  // ---- headers and trailers ---------------------------------------------------
  {
    // FEXTRA (xlen 3) | FNAME "ab" | FCOMMENT "c" | FHCRC, behind another member: the
    // CRC-16 is taken from the start of the whole input (src/GUnzip.ts:127-131)
    Bytes opt = {3, 0, 9, 9, 9, 'a', 'b', 0, 'c', 0};
    Bytes hd = {0x1F, 0x8B, 8, 0x1E, 1, 2, 3, 4, 0, 3};
    hd.insert(hd.end(), opt.begin(), opt.end());
    Bytes whole = cat({m0, hd});
    const uint32_t c16 = crc32_small(whole.data(), whole.size()) & 0xFFFF;
    whole.push_back(c16 & 0xFF);
    whole.push_back(c16 >> 8);
    const size_t body_at = whole.size();
    whole.insert(whole.end(), 12, 0x55);
    Item it(whole);
    zt_gzip_member m;
    GzError e;
    size_t body = 0;
    CHECK(gzip_parse_header(it.p, it.n, s1, &m, &body, &e) == ZT_OK && body == body_at);
    CHECK(m.flg == 0x1E && m.xlen == 3 && m.mtime == 0x04030201u && m.os == 3);
    CHECK(m.name_off == s1 + 15 && m.name_len == 2 && m.comment_off == s1 + 18 && m.comment_len == 1);
    CHECK(m.has_crc16 == 1 && m.crc16 == c16);
    // the member alone: its CRC-16 no longer matches
    Item alone(Bytes(whole.begin() + s1, whole.end()));
    CHECK(gzip_parse_header(alone.p, alone.n, 0, &m, &body, &e) == ZT_E_GZIP_HCRC);
    CHECK(std::string(e.msg) == "invalid header crc16");
    CHECK(gzip_parse_header(alone.p, alone.n, 0, &m, &body, &e, false) == ZT_OK && m.has_crc16 == 1);
    // cut inside the optional fields, at every length: never a read past the end
    for (size_t cut = 0; cut < body_at - s1; ++cut) {
      Item part(Bytes(whole.begin() + s1, whole.begin() + s1 + cut));
      const int rc = gzip_parse_header(part.p, part.n, 0, &m, &body, &e, false);
      CHECK(rc == (cut < 2 ? ZT_E_GZIP_SIGNATURE : cut < 3 ? ZT_E_GZIP_METHOD : ZT_E_INPUT_BROKEN) ||
            (rc == ZT_OK && body <= part.n));
    }
    Item sig(Bytes{0x1F});
    CHECK(gzip_parse_header(sig.p, sig.n, 0, &m, &body, &e) == ZT_E_GZIP_SIGNATURE);
    CHECK(std::string(e.msg) == "invalid file signature:31,undefined");
    Item cm(Bytes{0x1F, 0x8B, 7, 0});
    CHECK(gzip_parse_header(cm.p, cm.n, 0, &m, &body, &e) == ZT_E_GZIP_METHOD);
    CHECK(std::string(e.msg) == "unknown compression method: 7");
    // trailer: past the end reads as 0
    Item t(m1);
    size_t next = 0;
    CHECK(gzip_check_trailer(t.p, t.n, t.n - 8, 0x22222222u, 7, &m, &next, &e) == ZT_OK && next == t.n);
    CHECK(m.crc32 == 0x22222222u && m.isize == 7);
    CHECK(gzip_check_trailer(t.p, t.n, t.n - 8, 0x22222223u, 7, &m, &next, &e) == ZT_E_GZIP_CRC32);
    CHECK(std::string(e.msg) == "invalid CRC-32 checksum: 0x22222223 / 0x22222222");
    CHECK(gzip_check_trailer(t.p, t.n, t.n - 8, 0x22222222u, 8, &m, &next, &e) == ZT_E_GZIP_ISIZE);
    CHECK(std::string(e.msg) == "invalid input size: 8 / 7");
    CHECK(gzip_check_trailer(t.p, t.n, t.n - 2, 0u, 0, &m, &next, &e) == ZT_OK && next == t.n + 6);
  }
  // ---- bounds -----------------------------------------------------------------
  {
    const std::vector<size_t> c = {0, 100, 5000, 200000};
    CHECK(gz_bound(c, 0, 1u << 20) == 100 + kGzSlack);
    CHECK(gz_bound(c, 100, 1u << 20) == 5000 + kGzSlack);
    CHECK(gz_bound(c, 150, 1u << 20) == 5000 + kGzSlack);  // a start that is not in the list
    CHECK(gz_bound(c, 200000, 1u << 20) == (1u << 20));    // the last candidate: the item's end
    CHECK(gz_bound(c, 5000, 200000 + kGzSlack) == 200000 + kGzSlack);  // never past the item
    CHECK(gz_bound(c, 5000, 200001) == 200001);
    CHECK(gz_bound(std::vector<size_t>(), 0, 77) == 77);
    // the slack: 64 KiB up to one candidate per 4 KiB, then in proportion, never below the minimum
    CHECK(gz_slack(1u << 20, 1) == kGzSlack && gz_slack(1u << 20, 256) == kGzSlack);
    CHECK(gz_slack(1u << 20, 512) == kGzSlack / 2 && gz_slack(393216, 131072) == kGzSlackMin);
    CHECK(gz_slack(0, 0) == kGzSlack && gz_slack(0, 1) == kGzSlackMin);
    CHECK(gz_bound(c, 100, 1u << 20, 300) == 5300 && gz_bound(c, 5000, 200200, 300) == 200200);
    // the bounded inputs of an item's candidates: at most 17 items + the minimum each
    for (size_t nc : {1u, 7u, 300u, 5000u, 40000u}) {
      const size_t n = 1u << 20;
      std::vector<size_t> cs;
      for (size_t i = 0; i < nc; ++i) cs.push_back(i * (n / nc));
      size_t sum = 0;
      for (size_t st : cs) sum += gz_bound(cs, st, n, gz_slack(n, nc)) - st;
      CHECK(sum <= 17 * n + nc * kGzSlackMin);
    }
  }
  // ---- the host scan ----------------------------------------------------------
  {
    Item it(cat({Bytes{0x1F, 0x8B, 8, 0x1F, 0x1F, 0x8B, 8}, Bytes{0x1F, 0x8B, 7, 0x1F, 0x8B}, Bytes{0x1F, 0x8B, 8},
                 Bytes{0x1F, 0x8B}}));
    std::vector<size_t> f;
    gz_scan(it.p, it.n, 0, 100, &f);
    CHECK(f == (std::vector<size_t>{4, 12}));  // after `from`; the cut pattern at the end is none
    f.clear();
    gz_scan(it.p, it.n, 4, 100, &f);
    CHECK(f == (std::vector<size_t>{12}));
    f.clear();
    gz_scan(it.p, it.n, 0, 1, &f);
    CHECK(f == (std::vector<size_t>{4}));
    f.clear();
    gz_scan(it.p, it.n, it.n - 1, 5, &f);
    gz_scan(it.p, it.n, it.n + 9, 5, &f);
    gz_scan(nullptr, 0, 0, 5, &f);
    CHECK(f.empty());
  }
  // ---- the walk ---------------------------------------------------------------
  const Bytes three = cat({m0, m1, m2});
  {  // a clean chain
    Item it(three);
    std::vector<GzDecoded> tab = {decoded(0, 10, 40, it.n, 0x11111111u, 100, 5),
                                  decoded(s1, 10, 25, it.n, 0x22222222u, 7, 6),
                                  decoded(s2, 10, 60, it.n, 0x33333333u, 0, 7)};
    GzWalk w;
    CHECK(gz_walk(it.p, it.n, tab, &w) == GZ_DONE && w.members.size() == 3 && w.total == 107);
    CHECK(w.slots == (std::vector<size_t>{5, 6, 7}));
    CHECK(w.members[1].data_off == 100 && w.members[1].data_len == 7 && w.members[2].data_off == 107);
    CHECK(w.members[2].crc32 == 0x33333333u && w.members[2].isize == 0);
    CHECK(gz_walk(it.p, it.n, tab, &w) == GZ_DONE && w.members.size() == 3);  // a finished walk stays
  }
  {  // a false candidate inside a member (and one that even "decoded"): never used
    Item it(three);
    std::vector<GzDecoded> tab = {decoded(0, 10, 40, it.n, 0x11111111u, 100, 0),
                                  decoded(17, 10, 3, it.n, 0xDEADBEEFu, 5, 1),
                                  decoded(30, 10, 2, it.n, 0, 0, 2, ZT_E_INPUT_BROKEN),
                                  decoded(s1, 10, 25, it.n, 0x22222222u, 7, 3),
                                  decoded(s2, 10, 60, it.n, 0x33333333u, 0, 4)};
    GzWalk w;
    CHECK(gz_walk(it.p, it.n, tab, &w) == GZ_DONE && w.slots == (std::vector<size_t>{0, 3, 4}));
  }
  {  // a truncated list: the chain asks for the start it misses, then goes on
    Item it(three);
    std::vector<GzDecoded> tab = {decoded(0, 10, 40, it.n, 0x11111111u, 100, 0),
                                  decoded(s2, 10, 60, it.n, 0x33333333u, 0, 2)};
    GzWalk w;
    CHECK(gz_walk(it.p, it.n, tab, &w) == GZ_NEED && w.need_start == s1 && !w.need_full && w.members.size() == 1);
    tab.insert(tab.begin() + 1, decoded(s1, 10, 25, it.n, 0x22222222u, 7, 9));
    CHECK(gz_walk(it.p, it.n, tab, &w) == GZ_DONE && w.slots == (std::vector<size_t>{0, 9, 2}));
  }
  {  // a member past its bound: failed inside it, or ended beyond it -- decoded again to the item's end
    Item it(three);
    std::vector<GzDecoded> tab = {decoded(0, 10, 40, 30, 0, 0, 0, ZT_E_STORED_LEN),
                                  decoded(s1, 10, 25, s1 + 20, 0x22222222u, 7, 1),
                                  decoded(s2, 10, 60, it.n, 0x33333333u, 0, 2)};
    GzWalk w;
    CHECK(gz_walk(it.p, it.n, tab, &w) == GZ_NEED && w.need_start == 0 && w.need_full && w.need_bound == 30 &&
          !w.need_exact);
    tab[0] = decoded(0, 10, 40, it.n, 0x11111111u, 100, 3);
    CHECK(gz_walk(it.p, it.n, tab, &w) == GZ_NEED && w.need_start == s1 && w.need_full && w.members.size() == 1);
    tab[1] = decoded(s1, 10, 25, it.n, 0x22222222u, 7, 4);
    CHECK(gz_walk(it.p, it.n, tab, &w) == GZ_DONE && w.slots == (std::vector<size_t>{3, 4, 2}));
    // settled: finished with every consumed byte inside the bound
    CHECK(gz_settled(decoded(0, 10, 40, 50, 0, 0, 0), it.n) && !gz_settled(decoded(0, 10, 40, 49, 0, 0, 0), it.n));
    CHECK(gz_settled(decoded(0, 10, 40, it.n, 0, 0, 0, ZT_E_STORED_LEN), it.n));
    // a speculative failure is no verdict, even at the item's end: once more, for the decoder's own status
    std::vector<GzDecoded> t2 = {decoded(0, 10, 40, it.n, 0, 0, 0, ZT_E_INPUT_BROKEN)};
    t2[0].exact = false;
    GzWalk w2;
    CHECK(!gz_settled(t2[0], it.n));
    CHECK(gz_walk(it.p, it.n, t2, &w2) == GZ_NEED && w2.need_full && w2.need_exact && w2.need_bound == it.n);
    CHECK(gz_wider(0, w2.need_bound, it.n) == it.n);
    t2[0] = decoded(0, 10, 40, it.n, 0, 0, 0, ZT_E_UNKNOWN_BTYPE, 3);
    CHECK(gz_walk(it.p, it.n, t2, &w2) == GZ_FAILED && w2.err.code == ZT_E_UNKNOWN_BTYPE && w2.detail == 3);
    // a finished decode at the item's end stands, speculative or not
    t2[0] = decoded(0, 10, 40, it.n, 0x11111111u, 100, 0);
    t2[0].exact = false;
    CHECK(gz_settled(t2[0], it.n));
    // wider bounds: 8 times the input it had, at least 1 MiB, the item's end at the latest
    CHECK(gz_wider(100, 100 + (256u << 10), 64u << 20) == 100 + (2u << 20));
    CHECK(gz_wider(100, 1100, 64u << 20) == 100 + (1u << 20));
    CHECK(gz_wider(100, 1100, 5000) == 5000 && gz_wider(4990, 5000, 5000) == 5000);
    CHECK(gz_wider(1u << 20, 10u << 20, 64u << 20) == (64u << 20));
    for (size_t b = 200, steps = 0; b < (64u << 20); b = gz_wider(100, b, 64u << 20)) CHECK(++steps < 6);
  }
  {  // garbage after the last member: the reference's signature error; the members before it do not count
    Item it(cat({m0, m1, Bytes{'g', 'a', 'r'}}));
    std::vector<GzDecoded> tab = {decoded(0, 10, 40, it.n, 0x11111111u, 100, 0),
                                  decoded(s1, 10, 25, it.n, 0x22222222u, 7, 1)};
    GzWalk w;
    CHECK(gz_walk(it.p, it.n, tab, &w) == GZ_FAILED && w.err.code == ZT_E_GZIP_SIGNATURE);
    CHECK(std::string(w.err.msg) == "invalid file signature:103,97");
    CHECK(gz_walk(it.p, it.n, tab, &w) == GZ_FAILED);
  }
  {  // empty input: no member, no error
    Item it((Bytes()));
    GzWalk w;
    CHECK(gz_walk(it.p, it.n, std::vector<GzDecoded>(), &w) == GZ_DONE && w.members.empty() && w.total == 0);
  }
  {  // the decoder's own error, a wrong CRC-32, a wrong ISIZE, a trailer cut off: zt_gunzip's order
    Item it(three);
    std::vector<GzDecoded> tab = {decoded(0, 10, 40, it.n, 0x11111111u, 100, 0),
                                  decoded(s1, 10, 25, it.n, 0, 0, 1, ZT_E_INVALID_CODE_LENGTH, 19)};
    GzWalk w;
    CHECK(gz_walk(it.p, it.n, tab, &w) == GZ_FAILED && w.err.code == ZT_E_INVALID_CODE_LENGTH && w.detail == 19 &&
          w.err.msg[0] == 0);
    tab[1] = decoded(s1, 10, 25, it.n, 0x22222220u, 8, 1);  // CRC-32 comes before ISIZE
    GzWalk w2;
    CHECK(gz_walk(it.p, it.n, tab, &w2) == GZ_FAILED && w2.err.code == ZT_E_GZIP_CRC32);
    tab[1] = decoded(s1, 10, 25, it.n, 0x22222222u, 8, 1);
    GzWalk w3;
    CHECK(gz_walk(it.p, it.n, tab, &w3) == GZ_FAILED && w3.err.code == ZT_E_GZIP_ISIZE);
    Item cut(Bytes(m0.begin(), m0.end() - 3));
    std::vector<GzDecoded> t1 = {decoded(0, 10, 40, cut.n, 0x11111111u, 100, 0)};
    GzWalk w4;
    // (ISIZE = 64 00 00 00 cut after its first byte: the bytes past the end read as 0, as the reference reads them)
    CHECK(gz_walk(cut.p, cut.n, t1, &w4) == GZ_DONE && w4.members.size() == 1 && w4.ip == cut.n + 3);
    Item cut5(Bytes(m0.begin(), m0.end() - 5));
    t1[0].bound = cut5.n;
    GzWalk w5;
    CHECK(gz_walk(cut5.p, cut5.n, t1, &w5) == GZ_FAILED && w5.err.code == ZT_E_GZIP_CRC32);
    CHECK(std::string(w5.err.msg) == "invalid CRC-32 checksum: 0x11111111 / 0x111111");
  }
  if (fails) return fprintf(stderr, "gunzip_chain_check: %d checks failed\n", fails), 1;
  printf("gunzip_chain_check ok\n");
  return 0;
}
