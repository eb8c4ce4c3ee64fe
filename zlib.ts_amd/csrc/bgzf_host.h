// bgzf_host.h -- the host arithmetic of BGZF (include/zt_bgzf.h), no HIP: the
// block header parse, the BSIZE chain walk, the end marker, virtual offsets,
// the .gzi blob (encode, decode, structural validation), the lookup that
// turns byte ranges and virtual-offset chunks into the blocks they touch, and
// the dedup of the blocks a call needs.  Pure functions, checked on the CPU by
// tools/bgzf_host_check.cpp.
//
// Rule: no kernel sees an offset or a size that was not bounds-checked here.
// Every BgzfBlock this header hands out lies inside [0, n) with its CDATA and
// trailer, and its ISIZE is at most 65536 and at most 1032 x its CDATA length.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace zt {

constexpr uint32_t kBgzfBlockMax = 65280;     // ZT_BGZF_BLOCK_MAX: the largest input slice
constexpr uint32_t kBgzfBlockMin = 4096;      // the smallest block_size option
constexpr uint32_t kBgzfBlockBytes = 65536;   // BSIZE is 16 bits: the largest block
constexpr uint32_t kBgzfIsizeMax = 65536;
constexpr uint32_t kBgzfHeaderBytes = 18;     // the writer's header (XLEN 6)
constexpr uint32_t kBgzfTrailerBytes = 8;
constexpr uint32_t kBgzfEofBytes = 28;
constexpr uint64_t kBgzfExpandMax = 1032;     // RFC 1951: 258 bytes per 2 bits
constexpr uint64_t kBgzfCoffMax = 1ull << 48;

// the fixed end-of-file marker; its first 18 bytes with BSIZE patched are
// every written block's header
inline const uint8_t *bgzf_eof_marker() {
  static const uint8_t m[kBgzfEofBytes] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                                           0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  return m;
}

struct BgzfBlock {
  uint64_t off;        // block start in the file
  uint32_t size;       // BSIZE + 1
  uint32_t cdata_off;  // from the block start (12 + XLEN)
  uint32_t cdata_len;  // >= 2
  uint32_t isize;
  uint32_t crc;
};

inline uint32_t bgzf_le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t bgzf_le32(const uint8_t *p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
inline uint64_t bgzf_le64(const uint8_t *p) { return (uint64_t)bgzf_le32(p) | ((uint64_t)bgzf_le32(p + 4) << 32); }
inline void bgzf_put64(uint8_t *p, uint64_t v) {
  for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(v >> (8 * k));
}

// The block at in[off ..): null and *b filled, or the reason it is not one.
inline const char *bgzf_parse_block(const uint8_t *in, uint64_t n, uint64_t off, BgzfBlock *b) {
  if (off > n || n - off < 12) return "truncated header";
  const uint8_t *p = in + off;
  if (p[0] != 31 || p[1] != 139) return "wrong magic";
  if (p[2] != 8) return "unknown compression method";
  if (p[3] != 4) return "FLG is not FEXTRA alone";
  const uint32_t xlen = bgzf_le16(p + 10);
  if (xlen < 6) return "extra field too short";
  if (n - off < 12 + (uint64_t)xlen) return "truncated extra field";
  // subfields: SI1 SI2 SLEN data; the BC subfield (SLEN 2) need not be first
  uint32_t at = 0, bsize = 0;
  bool found = false;
  while (at + 4 <= xlen) {
    const uint8_t *s = p + 12 + at;
    const uint32_t slen = bgzf_le16(s + 2);
    if (at + 4 + slen > xlen) return "extra subfield overruns XLEN";
    if (s[0] == 66 && s[1] == 67) {
      if (slen != 2) return "BC subfield has the wrong length";
      if (!found) bsize = bgzf_le16(s + 4);
      found = true;
    }
    at += 4 + slen;
  }
  if (at != xlen) return "extra field has trailing bytes";
  if (!found) return "no BC subfield";
  const uint64_t size = (uint64_t)bsize + 1;
  if (size < 12 + (uint64_t)xlen + 2 + 8) return "BSIZE smaller than the header";
  if (n - off < size) return "truncated block";
  b->off = off;
  b->size = (uint32_t)size;
  b->cdata_off = 12 + xlen;
  b->cdata_len = (uint32_t)(size - 12 - xlen - 8);
  b->crc = bgzf_le32(p + size - 8);
  b->isize = bgzf_le32(p + size - 4);
  if (b->isize > kBgzfIsizeMax) return "ISIZE above 65536";
  if ((uint64_t)b->isize > kBgzfExpandMax * b->cdata_len) return "ISIZE above what its CDATA can expand to";
  return nullptr;
}

inline bool bgzf_is_eof(const uint8_t *in, const BgzfBlock &b) {
  return b.size == kBgzfEofBytes && memcmp(in + b.off, bgzf_eof_marker(), kBgzfEofBytes) == 0;
}

// ---- the chain walk ------------------------------------------------------------
struct BgzfWalk {
  std::vector<BgzfBlock> blocks;
  std::vector<uint64_t> uoff;  // blocks.size() + 1: output offset of every block, then the total
  uint64_t data_blocks = 0;
  bool has_eof = false;        // the last block is the marker and ends the file
  uint64_t error_offset = 0;
  const char *why = nullptr;   // non-null: the walk stopped at error_offset
};
// Blocks from `from` (a block start; output offset u0) until the file ends or,
// with stop != ~0, until a block starts at or after `stop`.
inline BgzfWalk bgzf_walk(const uint8_t *in, uint64_t n, uint64_t from = 0, uint64_t u0 = 0, uint64_t stop = ~0ull) {
  BgzfWalk w;
  uint64_t at = from, u = u0;
  while (at < n && at < stop) {
    BgzfBlock b;
    if (const char *why = bgzf_parse_block(in, n, at, &b)) {
      w.why = why;
      w.error_offset = at;
      break;
    }
    w.blocks.push_back(b);
    w.uoff.push_back(u);
    u += b.isize;
    if (b.isize) ++w.data_blocks;
    at += b.size;
  }
  w.uoff.push_back(u);
  w.has_eof = !w.why && at == n && !w.blocks.empty() && bgzf_is_eof(in, w.blocks.back());
  return w;
}

// "not a BGZF block at offset N: <reason>"
inline std::string bgzf_format_message(uint64_t off, const char *why) {
  return "not a BGZF block at offset " + std::to_string(off) + ": " + why;
}

// ---- virtual offsets ---------------------------------------------------------
inline uint64_t bgzf_voffset(uint64_t coffset, uint32_t uoffset) { return (coffset << 16) | (uoffset & 0xFFFFu); }
inline uint64_t bgzf_coffset(uint64_t v) { return v >> 16; }
inline uint32_t bgzf_uoffset(uint64_t v) { return (uint32_t)(v & 0xFFFFu); }

// ---- .gzi ------------------------------------------------------------------
struct GziPair {
  uint64_t coff, uoff;
};
// the writer's rule: one pair per block with ISIZE > 0 after the first such block
inline std::vector<GziPair> bgzf_gzi_pairs(const BgzfWalk &w) {
  std::vector<GziPair> p;
  bool first = true;
  for (size_t k = 0; k < w.blocks.size(); ++k) {
    if (!w.blocks[k].isize) continue;
    if (!first) p.push_back(GziPair{w.blocks[k].off, w.uoff[k]});
    first = false;
  }
  return p;
}
inline std::vector<uint8_t> bgzf_gzi_encode(const std::vector<GziPair> &p) {
  std::vector<uint8_t> g(8 + 16 * p.size());
  bgzf_put64(g.data(), p.size());
  for (size_t i = 0; i < p.size(); ++i) {
    bgzf_put64(g.data() + 8 + 16 * i, p[i].coff);
    bgzf_put64(g.data() + 16 + 16 * i, p[i].uoff);
  }
  return g;
}
// Structure only (the pairs are checked against the file where they are used):
// length = 8 + 16 N, compressed offsets strictly increasing, uncompressed
// offsets non-decreasing, every offset + 18 <= n.  Null and *pairs, or why not.
inline const char *bgzf_gzi_decode(const uint8_t *gzi, uint64_t len, uint64_t n, std::vector<GziPair> *pairs) {
  pairs->clear();
  if (!gzi || len < 8) return "shorter than its count";
  const uint64_t cnt = bgzf_le64(gzi);
  if ((len - 8) % 16 || cnt != (len - 8) / 16) return "length is not 8 + 16 N";
  pairs->resize(cnt);
  for (uint64_t i = 0; i < cnt; ++i) {
    GziPair &p = (*pairs)[i];
    p.coff = bgzf_le64(gzi + 8 + 16 * i);
    p.uoff = bgzf_le64(gzi + 16 + 16 * i);
    if (p.coff > n || n - p.coff < kBgzfHeaderBytes) return "offset past the file";
    if (i && p.coff <= (*pairs)[i - 1].coff) return "compressed offsets do not increase";
    if (i && p.uoff < (*pairs)[i - 1].uoff) return "uncompressed offsets decrease";
  }
  return nullptr;
}

// ---- lookup --------------------------------------------------------------------
// A block a call needs, with the output offset of its first byte.
struct BgzfNeed {
  BgzfBlock b;
  uint64_t uoff;
};
// One piece of a requested range: bytes [lo, lo + len) of the block at `boff`
// go to the range's output at `dst`.
struct BgzfPiece {
  uint64_t boff;  // the block's file offset (its identity for the dedup)
  uint32_t lo, len;
  uint64_t dst;   // offset in the range's own output
};
enum BgzfLookupError { kBgzfLookOk = 0, kBgzfLookFormat = 1, kBgzfLookIndex = 2 };
struct BgzfLookup {
  int err = kBgzfLookOk;
  uint64_t error_offset = 0;
  const char *why = nullptr;
};

// Where a file's output offsets come from: the whole chain walked once (no
// index), or .gzi pairs from which only the needed stretches are walked.
// Every pair a walk starts from or passes must be a block start of the file
// at exactly its uncompressed offset (kBgzfLookIndex otherwise).
class BgzfLocator {
 public:
  // no index: walk the file (look: a format error of the chain)
  BgzfLocator(const uint8_t *in, uint64_t n, BgzfLookup *look) : in_(in), n_(n) {
    BgzfWalk w = bgzf_walk(in, n);
    if (w.why) {
      look->err = kBgzfLookFormat;
      look->error_offset = w.error_offset;
      look->why = w.why;
    }
    total_ = w.uoff.back();
    walk_ = std::move(w);
    whole_ = true;
  }
  // with validated pairs: the total comes from a walk behind the last pair
  BgzfLocator(const uint8_t *in, uint64_t n, const std::vector<GziPair> &pairs, BgzfLookup *look)
      : in_(in), n_(n), pairs_(pairs) {
    const GziPair last = pairs_.empty() ? GziPair{0, 0} : pairs_.back();
    BgzfWalk w = bgzf_walk(in, n, last.coff, last.uoff);
    if (w.why) {
      // a pair that is no block start is the index's fault, a bad block behind it the file's
      look->err = (w.blocks.empty() && !pairs_.empty()) ? kBgzfLookIndex : kBgzfLookFormat;
      look->error_offset = w.error_offset;
      look->why = w.why;
    }
    total_ = w.uoff.back();
  }
  uint64_t total() const { return total_; }

  // The blocks with bytes in [off, off + len) (len > 0, off + len <= total),
  // in file order, appended to *need, and the range's pieces.
  BgzfLookup locate(uint64_t off, uint64_t len, std::vector<BgzfNeed> *need, std::vector<BgzfPiece> *pieces) const {
    BgzfLookup look;
    if (whole_) {
      // the last block that starts at or before off (empty blocks share an offset: skipped below)
      size_t k = (size_t)(std::upper_bound(walk_.uoff.begin(), walk_.uoff.end() - 1, off) - walk_.uoff.begin()) - 1;
      for (; k < walk_.blocks.size() && walk_.uoff[k] < off + len; ++k) take(walk_.blocks[k], walk_.uoff[k], off, len, need, pieces);
      return look;
    }
    // the last pair at or before off (none: the file start)
    size_t pi = (size_t)(std::upper_bound(pairs_.begin(), pairs_.end(), off,
                                          [](uint64_t v, const GziPair &p) { return v < p.uoff; }) -
                         pairs_.begin());
    uint64_t at = pi ? pairs_[pi - 1].coff : 0, u = pi ? pairs_[pi - 1].uoff : 0;
    bool from_pair = pi != 0;
    while (u < off + len) {
      // a pair the walk reaches or passes must sit exactly here
      while (pi < pairs_.size() && pairs_[pi].coff <= at) {
        if (pairs_[pi].coff != at || pairs_[pi].uoff != u) return fail(kBgzfLookIndex, pairs_[pi].coff, "pair is not on the chain");
        ++pi;
      }
      BgzfBlock b;
      if (at >= n_) return fail(kBgzfLookIndex, at, "chain ends before the range");
      if (const char *why = bgzf_parse_block(in_, n_, at, &b)) return fail(from_pair ? kBgzfLookIndex : kBgzfLookFormat, at, why);
      from_pair = false;
      take(b, u, off, len, need, pieces);
      u += b.isize;
      at += b.size;
    }
    // the pair behind the range's last block, where the walk stops
    if (pi < pairs_.size() && pairs_[pi].coff <= at && (pairs_[pi].coff != at || pairs_[pi].uoff != u))
      return fail(kBgzfLookIndex, pairs_[pi].coff, "pair is not on the chain");
    return look;
  }

 private:
  static BgzfLookup fail(int err, uint64_t off, const char *why) {
    BgzfLookup l;
    l.err = err;
    l.error_offset = off;
    l.why = why;
    return l;
  }
  static void take(const BgzfBlock &b, uint64_t u, uint64_t off, uint64_t len, std::vector<BgzfNeed> *need,
                   std::vector<BgzfPiece> *pieces) {
    const uint64_t lo = std::max(u, off), hi = std::min(u + b.isize, off + len);
    if (lo >= hi) return;
    need->push_back(BgzfNeed{b, u});
    pieces->push_back(BgzfPiece{b.off, (uint32_t)(lo - u), (uint32_t)(hi - lo), lo - off});
  }
  const uint8_t *in_;
  uint64_t n_;
  std::vector<GziPair> pairs_;
  BgzfWalk walk_;
  bool whole_ = false;
  uint64_t total_ = 0;
};

// pread clamp of zt_inflate_ranges: false when off > total (ZT_E_ARG)
inline bool bgzf_clamp(uint64_t total, uint64_t off, uint64_t *len) {
  if (off > total) return false;
  if (*len > total - off) *len = total - off;
  return true;
}

// A virtual-offset chunk [vbeg, vend): the chain from vbeg's block to vend's.
// kBgzfLookFormat: a coffset is no block start; arg: uoffset above its block's
// ISIZE or vend < vbeg.  A coffset equal to n with uoffset 0 is the file's end.
struct BgzfChunk {
  BgzfLookup look;
  bool arg = false;
  uint64_t len = 0;
};
inline BgzfChunk bgzf_locate_virtual(const uint8_t *in, uint64_t n, uint64_t vbeg, uint64_t vend,
                                     std::vector<BgzfNeed> *need, std::vector<BgzfPiece> *pieces) {
  BgzfChunk c;
  if (vend < vbeg) {
    c.arg = true;
    return c;
  }
  const uint64_t cb = bgzf_coffset(vbeg), ce = bgzf_coffset(vend);
  const uint32_t ub = bgzf_uoffset(vbeg), ue = bgzf_uoffset(vend);
  auto bad = [&](uint64_t off, const char *why) {
    c.look.err = kBgzfLookFormat;
    c.look.error_offset = off;
    c.look.why = why;
    return c;
  };
  uint64_t at = cb, dst = 0;
  for (;;) {
    if (at == n) {  // the end of the file: only (n, 0) points here
      if (at != ce) return bad(ce, "coffset is not a block start");
      if ((at == cb && ub) || ue) c.arg = true;
      break;
    }
    if (at > ce) return bad(ce, "coffset is not a block start");
    BgzfBlock b;
    if (const char *why = bgzf_parse_block(in, n, at, &b)) return bad(at, why);
    const uint32_t lo = at == cb ? ub : 0, hi = at == ce ? ue : b.isize;
    if (lo > b.isize || hi > b.isize) {
      c.arg = true;
      break;
    }
    if (hi > lo) {
      need->push_back(BgzfNeed{b, 0});
      pieces->push_back(BgzfPiece{b.off, lo, hi - lo, dst});
      dst += hi - lo;
    }
    if (at == ce) break;
    at += b.size;
  }
  c.len = dst;
  return c;
}

// ---- dedup ---------------------------------------------------------------------
// The distinct blocks of `need` in file order; slot_of(boff) finds a block's
// place in the result.
inline std::vector<BgzfNeed> bgzf_dedup(std::vector<BgzfNeed> need) {
  std::sort(need.begin(), need.end(), [](const BgzfNeed &a, const BgzfNeed &b) { return a.b.off < b.b.off; });
  need.erase(std::unique(need.begin(), need.end(), [](const BgzfNeed &a, const BgzfNeed &b) { return a.b.off == b.b.off; }),
             need.end());
  return need;
}
inline size_t bgzf_slot_of(const std::vector<BgzfNeed> &uniq, uint64_t boff) {
  return (size_t)(std::lower_bound(uniq.begin(), uniq.end(), boff,
                                   [](const BgzfNeed &a, uint64_t v) { return a.b.off < v; }) -
                  uniq.begin());
}

// ---- the writer's sizes ----------------------------------------------------------
// The largest CDATA of a slice of `len` bytes: stored
// blocks, or per 32 KiB parse block the smallest of stored, fixed and dynamic,
// never more than blen + 5 ceil(blen / 65535) + 5 with its sync point.  Fixed
// codes alone (compression type 1) have no such bound: 9 bits per byte.
inline uint64_t bgzf_cdata_bound(int ctype, uint64_t len) {
  if (ctype == 0) return len + 5 * ((len + 65534) / 65535);
  if (ctype == 1) return len + len / 8 + 16 * ((len + 32767) / 32768) + 16;
  uint64_t b = 0;
  for (uint64_t p = 0; p < len; p += 32768) {
    const uint64_t blen = std::min<uint64_t>(32768, len - p);
    b += blen + 5 * ((blen + 65534) / 65535) + 5;
  }
  return b;
}
static_assert(65280 + 2 * 10 + 26 <= 65536, "a full slice fits a block");

}  // namespace zt
