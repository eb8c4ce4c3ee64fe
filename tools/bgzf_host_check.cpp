// tools/bgzf_host_check.cpp -- drives the host-only half of BGZF
// (zlib.ts_amd/csrc/bgzf_host.h) without a device: the block header parse, the
// BSIZE chain walk, the end marker, the expansion bound, virtual offsets, the
// .gzi blob and its structural validation, the lookup from byte ranges and
// virtual-offset chunks to blocks (with and without an index) and the dedup,
// each against a slow restatement.  Meant to be built with a sanitizer and run
// on its own (tests/test_bgzf_host.py):
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o bgzf_host_check tools/bgzf_host_check.cpp
//   ./bgzf_host_check
//
// Every file is a heap allocation of exactly its bytes, so a read outside it
// stops the run.  The payloads are never decoded here: CDATA is filler.
// Prints "bgzf_host_check ok"; exit 1 on a broken invariant.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../zlib.ts_amd/csrc/bgzf_host.h"

using namespace zt;

static int fails = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      if (fails < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
      ++fails;                                                   \
    }                                                            \
  } while (0)

typedef std::vector<uint8_t> Bytes;

static void put16(Bytes &b, uint32_t v) {
  b.push_back(v & 0xFF);
  b.push_back((v >> 8) & 0xFF);
}
static void put32(Bytes &b, uint32_t v) {
  put16(b, v & 0xFFFF);
  put16(b, v >> 16);
}

// a block with `cdata` filler bytes, the given trailer and extra subfields in front of BC
static Bytes make_block(uint32_t cdata, uint32_t isize, uint32_t crc = 0x11223344u, const Bytes &extra = Bytes()) {
  Bytes b = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255};
  put16(b, 6 + (uint32_t)extra.size());
  b.insert(b.end(), extra.begin(), extra.end());
  b.push_back('B');
  b.push_back('C');
  put16(b, 2);
  put16(b, 12 + 6 + (uint32_t)extra.size() + cdata + 8 - 1);
  for (uint32_t i = 0; i < cdata; ++i) b.push_back((uint8_t)(i * 7 + 1));
  put32(b, crc);
  put32(b, isize);
  return b;
}
static Bytes eof_block() { return Bytes(bgzf_eof_marker(), bgzf_eof_marker() + kBgzfEofBytes); }

// a heap copy of exactly the bytes (a read past them is the sanitizer's)
struct Exact {
  uint8_t *p;
  size_t n;
  explicit Exact(const Bytes &b) : p((uint8_t *)malloc(b.size() ? b.size() : 1)), n(b.size()) {
    if (n) memcpy(p, b.data(), n);
  }
  ~Exact() { free(p); }
};

static const char *parse(const Bytes &b, uint64_t off, BgzfBlock *out) {
  Exact e(b);
  return bgzf_parse_block(e.p, e.n, off, out);
}

static void check_parse() {
  BgzfBlock b;
  const Bytes good = make_block(100, 4000);
  CHECK(parse(good, 0, &b) == nullptr);
  CHECK(b.off == 0 && b.size == good.size() && b.cdata_off == 18 && b.cdata_len == 100 && b.isize == 4000 &&
        b.crc == 0x11223344u);
  // the marker sits exactly on the minimum size and must pass
  CHECK(parse(eof_block(), 0, &b) == nullptr);
  CHECK(b.size == 28 && b.cdata_len == 2 && b.isize == 0 && b.crc == 0);
  {
    Exact e(eof_block());
    CHECK(bgzf_is_eof(e.p, b));
  }
  {
    Bytes other = eof_block();  // an empty block that is not the marker (stored form would differ; here: OS byte)
    other[9] = 3;
    Exact e(other);
    BgzfBlock o;
    CHECK(bgzf_parse_block(e.p, e.n, 0, &o) == nullptr && !bgzf_is_eof(e.p, o));
  }
  // every malformed header
  for (int field = 0; field < 4; ++field) {
    Bytes x = good;
    x[field] ^= 1;
    CHECK(parse(x, 0, &b) != nullptr);
  }
  {
    Bytes x = good;
    x[3] = 0x0C;  // FLG with FNAME as well
    CHECK(parse(x, 0, &b) != nullptr);
  }
  {
    Bytes x = good;
    x[10] = 5;  // XLEN < 6
    CHECK(parse(x, 0, &b) != nullptr);
  }
  {
    Bytes x = good;
    x[12] = 'X';  // no BC subfield
    CHECK(parse(x, 0, &b) != nullptr && std::string(parse(x, 0, &b)) == "no BC subfield");
  }
  {
    Bytes x = good;
    x[14] = 3;  // BC with SLEN 3: overruns XLEN
    CHECK(parse(x, 0, &b) != nullptr);
  }
  {
    Bytes x = make_block(2, 0);  // exactly the minimum: header + 2 + trailer
    CHECK(x.size() == 28 && x[16] == 27 && parse(x, 0, &b) == nullptr && b.size == 28 && b.cdata_len == 2);
    x[16] = 26;  // BSIZE smaller than that
    CHECK(parse(x, 0, &b) != nullptr && std::string(parse(x, 0, &b)) == "BSIZE smaller than the header");
    x = good;
    x[16] = 5;
    x[17] = 0;
    CHECK(parse(x, 0, &b) != nullptr && std::string(parse(x, 0, &b)) == "BSIZE smaller than the header");
  }
  for (size_t cut = 0; cut < good.size(); ++cut) {  // truncated anywhere
    Bytes x(good.begin(), good.begin() + (long)cut);
    CHECK(parse(x, 0, &b) != nullptr);
  }
  CHECK(parse(good, good.size(), &b) != nullptr && parse(good, good.size() + 5, &b) != nullptr);
  CHECK(parse(make_block(100, 65536), 0, &b) == nullptr);
  CHECK(parse(make_block(100, 65537), 0, &b) != nullptr);
  // the expansion bound: 1032 bytes per CDATA byte
  CHECK(parse(make_block(2, 2064), 0, &b) == nullptr);
  CHECK(parse(make_block(2, 2065), 0, &b) != nullptr);
  CHECK(parse(make_block(63, 65016), 0, &b) == nullptr && parse(make_block(63, 65017), 0, &b) != nullptr);
  // a foreign 6-byte subfield in front of BC (XLEN 12), and one behind it
  {
    const Bytes extra = {'Z', 'T', 2, 0, 9, 9};
    const Bytes x = make_block(50, 300, 7, extra);
    CHECK(parse(x, 0, &b) == nullptr && b.cdata_off == 24 && b.cdata_len == 50 && b.size == x.size() && b.crc == 7);
    Bytes y = make_block(50, 300);
    y[10] = 12;  // XLEN 12: the six bytes behind BC become a subfield 'xx' with SLEN 2
    const uint8_t tail[6] = {'x', 'x', 2, 0, 1, 2};
    y.insert(y.begin() + 18, tail, tail + 6);
    const uint32_t bs = (uint32_t)y.size() - 1;
    y[16] = bs & 0xFF;
    y[17] = bs >> 8;
    CHECK(parse(y, 0, &b) == nullptr && b.cdata_off == 24 && b.cdata_len == 50);
  }
}

struct Made {
  Bytes file;
  std::vector<uint64_t> off, uoff;  // per block
  std::vector<uint32_t> isize, size;
  uint64_t total = 0;
};
// blocks of the given ISIZEs (0: an empty block; -1: the marker)
static Made make_file(const std::vector<int> &isizes) {
  Made m;
  for (int is : isizes) {
    const Bytes b = is < 0 ? eof_block() : make_block(is == 0 ? 2 : 10 + (uint32_t)is / 40, (uint32_t)is);
    m.off.push_back(m.file.size());
    m.uoff.push_back(m.total);
    m.isize.push_back(is < 0 ? 0 : (uint32_t)is);
    m.size.push_back((uint32_t)b.size());
    m.file.insert(m.file.end(), b.begin(), b.end());
    m.total += is < 0 ? 0 : (uint64_t)is;
  }
  return m;
}

static void check_walk_and_gzi() {
  const Made m = make_file({4096, 4096, 0, 100, -1, 65536, 1, -1});
  Exact e(m.file);
  const BgzfWalk w = bgzf_walk(e.p, e.n);
  CHECK(!w.why && w.blocks.size() == 8 && w.data_blocks == 5 && w.has_eof && w.uoff.back() == m.total);
  for (size_t k = 0; k < w.blocks.size(); ++k)
    CHECK(w.blocks[k].off == m.off[k] && w.uoff[k] == m.uoff[k] && w.blocks[k].isize == m.isize[k] &&
          w.blocks[k].size == m.size[k]);
  // the writer's pairs: every data block after the first
  const std::vector<GziPair> p = bgzf_gzi_pairs(w);
  CHECK(p.size() == 4 && p[0].coff == m.off[1] && p[1].coff == m.off[3] && p[2].coff == m.off[5] &&
        p[3].coff == m.off[6] && p[3].uoff == m.uoff[6]);
  const Bytes g = bgzf_gzi_encode(p);
  CHECK(g.size() == 8 + 16 * 4 && g[0] == 4);
  std::vector<GziPair> back;
  {
    Exact ge(g);
    CHECK(bgzf_gzi_decode(ge.p, ge.n, e.n, &back) == nullptr && back.size() == 4);
    for (size_t i = 0; i < back.size(); ++i) CHECK(back[i].coff == p[i].coff && back[i].uoff == p[i].uoff);
    // every structural rejection
    CHECK(bgzf_gzi_decode(ge.p, ge.n - 1, e.n, &back) != nullptr);
    CHECK(bgzf_gzi_decode(ge.p, 7, e.n, &back) != nullptr);
    CHECK(bgzf_gzi_decode(nullptr, 0, e.n, &back) != nullptr);
  }
  {
    Bytes x = g;
    x[0] = 5;  // the count disagrees with the length
    Exact ge(x);
    CHECK(bgzf_gzi_decode(ge.p, ge.n, e.n, &back) != nullptr);
  }
  {
    std::vector<GziPair> q = p;
    std::swap(q[1], q[2]);
    const Bytes x = bgzf_gzi_encode(q);
    Exact ge(x);
    CHECK(bgzf_gzi_decode(ge.p, ge.n, e.n, &back) != nullptr);
    q = p;
    q[2].coff = q[1].coff;  // not strictly increasing
    const Bytes y = bgzf_gzi_encode(q);
    Exact gy(y);
    CHECK(bgzf_gzi_decode(gy.p, gy.n, e.n, &back) != nullptr);
    q = p;
    q[2].uoff = q[1].uoff - 1;  // decreasing output offsets
    const Bytes z = bgzf_gzi_encode(q);
    Exact gz(z);
    CHECK(bgzf_gzi_decode(gz.p, gz.n, e.n, &back) != nullptr);
    q = p;
    q[3].coff = e.n - 17;  // offset + 18 > n
    const Bytes v = bgzf_gzi_encode(q);
    Exact gv(v);
    CHECK(bgzf_gzi_decode(gv.p, gv.n, e.n, &back) != nullptr);
    q[3].coff = e.n - 18;
    const Bytes u = bgzf_gzi_encode(q);
    Exact gu(u);
    CHECK(bgzf_gzi_decode(gu.p, gu.n, e.n, &back) == nullptr);
  }
  // a file without the final marker, a truncated one, garbage behind a block
  {
    const Made a = make_file({100, 200});
    Exact ea(a.file);
    const BgzfWalk wa = bgzf_walk(ea.p, ea.n);
    CHECK(!wa.why && !wa.has_eof && wa.blocks.size() == 2);
    const BgzfWalk wt = bgzf_walk(ea.p, ea.n - 3);
    CHECK(wt.why && wt.error_offset == a.off[1] && wt.blocks.size() == 1);
    Bytes x = a.file;
    x[a.off[1]] = 0;
    Exact ex(x);
    const BgzfWalk wx = bgzf_walk(ex.p, ex.n);
    CHECK(wx.why && wx.error_offset == a.off[1] && std::string(wx.why) == "wrong magic");
    CHECK(bgzf_format_message(wx.error_offset, wx.why) ==
          "not a BGZF block at offset " + std::to_string(a.off[1]) + ": wrong magic");
  }
  {
    const BgzfWalk w0 = bgzf_walk(nullptr, 0);
    CHECK(!w0.why && w0.blocks.empty() && !w0.has_eof && w0.uoff.size() == 1 && w0.uoff[0] == 0);
  }
}

static void check_voffsets() {
  CHECK(bgzf_voffset(0, 0) == 0 && bgzf_voffset(1, 0) == 65536 && bgzf_voffset(3, 7) == (3u << 16 | 7));
  const uint64_t v = bgzf_voffset((1ull << 48) - 1, 65535);
  CHECK(bgzf_coffset(v) == (1ull << 48) - 1 && bgzf_uoffset(v) == 65535 && v == ~0ull);
}

// the slow restatement: every data block overlapping [off, off + len)
static void slow_locate(const Made &m, uint64_t off, uint64_t len, std::vector<uint64_t> *blocks,
                        std::vector<BgzfPiece> *pieces) {
  for (size_t k = 0; k < m.off.size(); ++k) {
    const uint64_t lo = std::max(m.uoff[k], off), hi = std::min(m.uoff[k] + m.isize[k], off + len);
    if (lo >= hi) continue;
    blocks->push_back(m.off[k]);
    pieces->push_back(BgzfPiece{m.off[k], (uint32_t)(lo - m.uoff[k]), (uint32_t)(hi - lo), lo - off});
  }
}

static uint32_t rng_state = 0x2545F491u;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

static void check_lookup() {
  const Made m = make_file({4096, 4096, 0, 100, -1, 65536, 1, 0, 4000, -1});
  Exact e(m.file);
  BgzfLookup look;
  const BgzfLocator whole(e.p, e.n, &look);
  CHECK(!look.err && whole.total() == m.total);
  const BgzfWalk w = bgzf_walk(e.p, e.n);
  // three indexes: the writer's, a sparse one, one with pairs on empty blocks and the marker
  std::vector<std::vector<GziPair>> indexes;
  indexes.push_back(bgzf_gzi_pairs(w));
  indexes.push_back({GziPair{m.off[5], m.uoff[5]}});
  indexes.push_back({GziPair{m.off[2], m.uoff[2]}, GziPair{m.off[4], m.uoff[4]}, GziPair{m.off[7], m.uoff[7]},
                     GziPair{m.off[9], m.uoff[9]}});
  indexes.push_back({});
  for (const auto &pairs : indexes) {
    BgzfLookup l2;
    const BgzfLocator loc(e.p, e.n, pairs, &l2);
    CHECK(!l2.err && loc.total() == m.total);
    for (int it = 0; it < 400; ++it) {
      uint64_t off = rnd() % m.total, len = 1 + rnd() % (it % 4 == 0 ? m.total : 5000);
      if (it == 0) off = 0, len = m.total;
      if (it == 1) off = m.total - 1, len = 1;
      if (it == 2) off = 4095, len = 2;
      CHECK(bgzf_clamp(m.total, off, &len) && len > 0);
      std::vector<uint64_t> want;
      std::vector<BgzfPiece> wp, gp, hp;
      slow_locate(m, off, len, &want, &wp);
      std::vector<BgzfNeed> a, b;
      const BgzfLookup ra = whole.locate(off, len, &a, &gp), rb = loc.locate(off, len, &b, &hp);
      CHECK(!ra.err && !rb.err && a.size() == want.size() && b.size() == want.size());
      for (size_t k = 0; k < want.size() && k < a.size() && k < b.size(); ++k) {
        CHECK(a[k].b.off == want[k] && b[k].b.off == want[k] && a[k].uoff == b[k].uoff);
        CHECK(gp[k].boff == wp[k].boff && gp[k].lo == wp[k].lo && gp[k].len == wp[k].len && gp[k].dst == wp[k].dst);
        CHECK(hp[k].boff == wp[k].boff && hp[k].lo == wp[k].lo && hp[k].len == wp[k].len && hp[k].dst == wp[k].dst);
      }
    }
  }
  // clamp
  {
    uint64_t len = 10;
    CHECK(bgzf_clamp(100, 95, &len) && len == 5);
    len = 10;
    CHECK(bgzf_clamp(100, 100, &len) && len == 0);
    len = 10;
    CHECK(!bgzf_clamp(100, 101, &len));
    len = ~0ull;
    CHECK(bgzf_clamp(100, 1, &len) && len == 99);
  }
  // an index that does not fit the file: a pair off a block start, an output offset off by one
  {
    std::vector<GziPair> bad = bgzf_gzi_pairs(w);
    bad[1].coff += 1;
    BgzfLookup l2;
    const BgzfLocator loc(e.p, e.n, bad, &l2);
    std::vector<BgzfNeed> need;
    std::vector<BgzfPiece> pc;
    CHECK(!l2.err);  // (the last pair is fine: the total walks from it)
    CHECK(loc.locate(0, m.total, &need, &pc).err == kBgzfLookIndex);
    CHECK(loc.locate(m.uoff[3], 50, &need, &pc).err == kBgzfLookIndex);  // starts from the bad pair
    CHECK(loc.locate(0, 100, &need, &pc).err == kBgzfLookOk);            // never reaches it
  }
  {
    std::vector<GziPair> bad = bgzf_gzi_pairs(w);
    bad[2].uoff += 1;
    BgzfLookup l2;
    const BgzfLocator loc(e.p, e.n, bad, &l2);
    std::vector<BgzfNeed> need;
    std::vector<BgzfPiece> pc;
    CHECK(loc.locate(0, m.total, &need, &pc).err == kBgzfLookIndex);
  }
  {
    std::vector<GziPair> bad = bgzf_gzi_pairs(w);
    bad.back().coff += 3;  // the last pair is no block start: the total's walk finds it
    BgzfLookup l2;
    const BgzfLocator loc(e.p, e.n, bad, &l2);
    CHECK(l2.err == kBgzfLookIndex);
  }
  // dedup
  {
    std::vector<BgzfNeed> need;
    std::vector<BgzfPiece> pc;
    whole.locate(4000, 5000, &need, &pc);
    whole.locate(0, 10, &need, &pc);
    whole.locate(m.total - 10, 10, &need, &pc);
    whole.locate(100, 4100, &need, &pc);
    const std::vector<BgzfNeed> u = bgzf_dedup(need);
    std::set<uint64_t> want;
    for (const BgzfNeed &x : need) want.insert(x.b.off);
    CHECK(u.size() == want.size() && u.size() == 5 && need.size() == 8);
    for (size_t k = 0; k < u.size(); ++k) {
      CHECK(want.count(u[k].b.off) == 1 && (k == 0 || u[k - 1].b.off < u[k].b.off));
      CHECK(bgzf_slot_of(u, u[k].b.off) == k);
    }
  }
  // virtual-offset chunks
  {
    std::vector<BgzfNeed> need;
    std::vector<BgzfPiece> pc;
    // inside one block
    BgzfChunk c = bgzf_locate_virtual(e.p, e.n, bgzf_voffset(m.off[1], 10), bgzf_voffset(m.off[1], 300), &need, &pc);
    CHECK(!c.look.err && !c.arg && c.len == 290 && need.size() == 1 && pc[0].lo == 10 && pc[0].len == 290);
    need.clear(), pc.clear();
    // across blocks 1..5 (an empty block and a marker between them)
    c = bgzf_locate_virtual(e.p, e.n, bgzf_voffset(m.off[1], 4000), bgzf_voffset(m.off[5], 7), &need, &pc);
    CHECK(!c.look.err && !c.arg && c.len == 96 + 100 + 7 && need.size() == 3 && pc.size() == 3);
    CHECK(pc[0].dst == 0 && pc[1].dst == 96 && pc[2].dst == 196 && pc[2].lo == 0 && pc[2].len == 7);
    need.clear(), pc.clear();
    // beg == end, the end of a block, the end of the file
    c = bgzf_locate_virtual(e.p, e.n, bgzf_voffset(m.off[3], 5), bgzf_voffset(m.off[3], 5), &need, &pc);
    CHECK(!c.look.err && !c.arg && c.len == 0 && need.empty());
    c = bgzf_locate_virtual(e.p, e.n, bgzf_voffset(m.off[8], 3990), bgzf_voffset(e.n, 0), &need, &pc);
    CHECK(!c.look.err && !c.arg && c.len == 10 && need.size() == 1);
    need.clear(), pc.clear();
    c = bgzf_locate_virtual(e.p, e.n, bgzf_voffset(e.n, 0), bgzf_voffset(e.n, 0), &need, &pc);
    CHECK(!c.look.err && !c.arg && c.len == 0);
    // a coffset in the middle of a block, at either end
    c = bgzf_locate_virtual(e.p, e.n, bgzf_voffset(m.off[1] + 20, 0), bgzf_voffset(m.off[3], 5), &need, &pc);
    CHECK(c.look.err == kBgzfLookFormat);
    c = bgzf_locate_virtual(e.p, e.n, bgzf_voffset(m.off[1], 0), bgzf_voffset(m.off[3] + 1, 5), &need, &pc);
    CHECK(c.look.err == kBgzfLookFormat);
    c = bgzf_locate_virtual(e.p, e.n, bgzf_voffset(e.n + 1, 0), bgzf_voffset(e.n + 1, 1), &need, &pc);
    CHECK(c.look.err == kBgzfLookFormat);
    // uoffset above ISIZE, end before begin
    c = bgzf_locate_virtual(e.p, e.n, bgzf_voffset(m.off[3], 101), bgzf_voffset(m.off[5], 5), &need, &pc);
    CHECK(!c.look.err && c.arg);
    c = bgzf_locate_virtual(e.p, e.n, bgzf_voffset(m.off[1], 0), bgzf_voffset(m.off[3], 101), &need, &pc);
    CHECK(!c.look.err && c.arg);
    c = bgzf_locate_virtual(e.p, e.n, bgzf_voffset(m.off[3], 5), bgzf_voffset(m.off[3], 4), &need, &pc);
    CHECK(c.arg);
    c = bgzf_locate_virtual(e.p, e.n, bgzf_voffset(m.off[3], 100), bgzf_voffset(m.off[3], 100), &need, &pc);
    CHECK(!c.look.err && !c.arg && c.len == 0);  // uoffset == ISIZE is the block's end
  }
}

static void check_bounds() {
  // the writer's block bound: a full slice fits a block with room to spare
  CHECK(bgzf_cdata_bound(2, 65280) == 65300 && 18 + bgzf_cdata_bound(2, 65280) + 8 == 65326);
  CHECK(bgzf_cdata_bound(0, 65280) == 65285 && bgzf_cdata_bound(2, 4096) == 4106 && bgzf_cdata_bound(2, 32769) == 32768 + 10 + 1 + 10);
  for (uint64_t len = 1; len <= 65280; len += 997) CHECK(18 + bgzf_cdata_bound(2, len) + 8 <= 65536);
  CHECK(bgzf_cdata_bound(1, 65280) > 65536);  // fixed codes alone can overflow: checked at run time
}

int main() {
  check_parse();
  check_walk_and_gzi();
  check_voffsets();
  check_lookup();
  check_bounds();
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("bgzf_host_check ok\n");
  return 0;
}
