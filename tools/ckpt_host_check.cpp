// tools/ckpt_host_check.cpp -- drives the host-only half of the checkpoint
// index (zlib.ts_amd/csrc/ckpt_host.h) without a device: the validation of a
// blob and the planner that turns ranges into packed headers, spans, exact
// units, chain units and copy segments.  Meant to be built with a sanitizer
// and run on its own (tests/test_ckpt_host.py):
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o ckpt_host_check tools/ckpt_host_check.cpp
//   ./ckpt_host_check
//
// Every blob is a heap allocation of exactly its bytes, so a read outside it
// stops the run.  Prints "ckpt_host_check ok"; exit 1 on a broken invariant.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../zlib.ts_amd/csrc/ckpt_host.h"

using namespace zt;

static int fails = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      if (fails < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

static uint32_t rng_state = 0x2545F491u;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

// A synthetic chain of `nunits` units from byte `stream_start`: one long
// dynamic block first (its header at the stream's first bit: every entry
// inside names it, as the one-block streams do), then fixed blocks, stored
// payloads, a length field, block starts and short dynamic blocks in turn.
// Some units are empty.  Windows are placed by the build's rule.
struct Synth {
  std::vector<CkEntry> e;  // with the sentinel
  uint64_t n = 0, stream_start = 0, span = 0;
  uint32_t nwin = 0;
};
static Synth synth(size_t nunits, uint64_t stream_start, uint64_t span) {
  Synth s;
  s.stream_start = stream_start;
  s.span = span;
  uint64_t pos = stream_start * 8, out = 0, hdr = pos;
  for (size_t k = 0; k < nunits; ++k) {
    CkEntry x{};
    x.pos = pos;
    x.out_off = out;
    if (k == 0) {
      x.kind = CK_BLOCK;
    } else if (k < nunits / 2 || k % 7 == 1) {
      x.kind = CK_HUFF;
      x.hdr = k < nunits / 2 ? hdr : (k % 14 == 1 ? kCkFixedHdr : pos - 900 - (k & 7));
    } else if (k % 7 == 2) {
      x.kind = CK_STORED;
      x.pos = pos = (pos + 7) & ~7ull;
      x.rem = 1 + k % 500;
      x.flags = k % 3 == 0 ? 2u : 0u;
    } else if (k % 7 == 3) {
      x.kind = CK_SHDR;
      x.pos = pos = (pos + 7) & ~7ull;
    } else if (k % 7 == 4) {
      x.kind = CK_BLOCK;
    } else {
      x.kind = CK_HUFF;
      x.hdr = pos - 2000;
      x.flags = k + 1 == nunits ? 2u : 0u;
    }
    const bool empty = k % 11 == 5;
    const uint64_t bits = empty ? 0 : 40000 + 977 * (k % 13);
    x.ntok = empty ? 0 : (uint32_t)(bits / 9);
    const uint64_t ol = empty ? 0 : (uint64_t)x.ntok * (k % 5 == 0 ? 40 : 3) + k % 3;
    s.e.push_back(x);
    pos += bits;
    out += ol;
  }
  CkEntry se{};
  se.pos = pos + 3;
  se.kind = CK_FINAL;
  se.out_off = out;
  s.e.push_back(se);
  s.nwin = ckpt_place_windows(s.e, span);
  s.n = (se.pos + 7) / 8 + 4;
  return s;
}
static std::vector<uint8_t> blob_of(const Synth &s) {
  const size_t nunits = s.e.size() - 1;
  std::vector<uint8_t> b(ckpt_blob_bytes(nunits, s.nwin));
  ckpt_write_header(b.data(), (uint32_t)nunits, s.nwin, s.stream_start, (s.e.back().pos + 7) / 8, s.e.back().out_off,
                    s.span);
  for (size_t k = 0; k <= nunits; ++k) ckpt_write_entry(b.data(), k, s.e[k]);
  for (uint32_t w = 0; w < s.nwin; ++w) {
    uint8_t *p = ckpt_window_at(b.data(), nunits, w);
    for (size_t i = 0; i < kCkWindow; ++i) p[i] = (uint8_t)(w * 31 + i);
    idx_put32(p + kCkWindow, 0xC0FFEE00u + w);
    memset(p + kCkWindow + 4, 0, kCkWinRec - kCkWindow - 4);
  }
  return b;
}
// validation on a heap copy of exactly `len` bytes
static const char *validate(const std::vector<uint8_t> &b, size_t len, size_t n, CkptView *v) {
  uint8_t *h = (uint8_t *)malloc(len ? len : 1);
  memcpy(h, b.data(), len);
  const char *why = ckpt_validate(h, len, n, v);
  v->wins = nullptr;  // (points into h)
  free(h);
  return why;
}

// every invariant of a plan, against a serial restatement
static void check_plan(const CkptView &v, const CkptPlan &p, const uint64_t *off, const uint64_t *len, size_t count,
                       size_t n) {
  CHECK(p.ranges.size() == count);
  CHECK(p.units.size() == p.chain.size());
  // serial restatement: the units each range needs, one by one
  std::vector<uint8_t> need(v.nunits, 0);
  uint64_t ret = 0;
  for (size_t i = 0; i < count; ++i) {
    const PlannedRange &r = p.ranges[i];
    if (off[i] > v.total_out) {
      CHECK(r.status == ZT_E_ARG && r.span < 0);
      continue;
    }
    const uint64_t l = len[i] < v.total_out - off[i] ? len[i] : v.total_out - off[i];
    CHECK(r.status == ZT_OK && r.off == off[i] && r.len == l);
    CHECK(r.dst % 256 == 0 && r.dst + (l ? l : 1) <= p.dst_total);
    ret += l;
    if (l == 0) {
      CHECK(r.span < 0);
      continue;
    }
    uint32_t first = 0, last = 0;
    for (uint32_t k = 0; k < v.nunits; ++k) {
      if ((k == 0 || (v.e[k].flags & 1)) && v.e[k].out_off <= off[i]) first = k;
      if (v.e[k].out_off <= off[i] + l - 1) last = k;
    }
    for (uint32_t k = first; k <= last; ++k) need[k] = 1;
    CHECK(r.span >= 0 && (size_t)r.span < p.spans.size());
    if (r.span < 0 || (size_t)r.span >= p.spans.size()) continue;
    const CkSpan &s = p.spans[r.span];
    CHECK(s.first <= first && last <= s.last);
    CHECK(r.src == s.out_pos + (off[i] - v.e[s.first].out_off));
    CHECK(r.src + l <= s.out_pos + s.out_len);
  }
  CHECK(p.ret_bytes == ret);
  // the planned units are exactly the needed ones, each once; spans are the maximal runs
  std::vector<uint8_t> got(v.nunits, 0);
  for (const CkUnit &j : p.units) {
    CHECK(j.entry < v.nunits && !got[j.entry]);
    if (j.entry < v.nunits) got[j.entry]++;
  }
  CHECK(got == need);
  std::set<uint64_t> hdr_want;
  uint64_t units = 0, tok = 0, dec = 0, inb = 0;
  for (size_t k = 0; k < p.spans.size(); ++k) {
    const CkSpan &s = p.spans[k];
    CHECK(s.first <= s.last && s.last < v.nunits);
    CHECK(s.first == 0 || (v.e[s.first].flags & 1));
    if (k) CHECK(s.first > p.spans[k - 1].last + 1);
    CHECK(s.unit0 == units);
    CHECK(s.in_pos % 64 == 0 && s.out_pos % 256 == 0);
    CHECK(s.byte0 == v.e[s.first].pos / 8);
    CHECK(s.byte0 + s.in_len == (v.e[s.last + 1].pos + 7) / 8);
    CHECK(s.byte0 + s.in_len <= n);  // what the host copies out of the caller's input
    CHECK(s.in_pos + s.in_len <= p.in_total && s.out_pos + s.out_len <= p.dec_total);
    CHECK(s.in_pos >= p.hdrs.size() * kCkHdrSlot);
    // only the stream's first segment lies at decode offset 0
    CHECK((s.out_pos == 0) == (k == 0 && s.first == 0));
    if (k) {
      CHECK(s.in_pos >= p.spans[k - 1].in_pos + p.spans[k - 1].in_len);
      CHECK(s.out_pos >= p.spans[k - 1].out_pos + p.spans[k - 1].out_len);
    }
    CHECK(s.out_len == v.e[s.last + 1].out_off - v.e[s.first].out_off);
    dec += s.out_len;
    inb += s.in_len;
    const uint64_t shift = s.in_pos * 8 - s.byte0 * 8;
    for (uint32_t u = s.first; u <= s.last; ++u, ++units) {
      const CkUnit &j = p.units[units];
      const ChainUnit &c = p.chain[units];
      const CkEntry &e = v.e[u], &nx = v.e[u + 1];
      CHECK(j.entry == u);
      CHECK(j.pos == e.pos + shift && j.e_pos == nx.pos + shift);
      CHECK(j.pos / 8 >= s.in_pos && (j.e_pos + 7) / 8 <= s.in_pos + s.in_len);
      CHECK(j.stop == (u + 1 == v.nunits ? kCkNoStop : j.e_pos));
      CHECK(j.kind == e.kind && j.rem == e.rem && j.bfinal == ((e.flags >> 1) & 1));
      CHECK(j.e_kind == nx.kind && j.e_rem == nx.rem && j.e_bfinal == ((nx.flags >> 1) & 1));
      // headers: fixed as it is, inside the span moved with it, before the span in a slot that keeps hdr & 7
      const CkEntry *both[2] = {&e, &nx};
      const uint64_t got_h[2] = {j.hdr, j.e_hdr};
      for (int q = 0; q < 2; ++q) {
        const CkEntry &x = *both[q];
        if (x.kind != CK_HUFF) {
          CHECK(got_h[q] == 0);
        } else if (x.hdr == kCkFixedHdr) {
          CHECK(got_h[q] == kCkFixedHdr);
        } else if (x.hdr / 8 >= s.byte0) {
          CHECK(got_h[q] == x.hdr + shift);
        } else {
          hdr_want.insert(x.hdr);
          bool found = false;
          for (const CkHdr &h : p.hdrs)
            if (h.hdr == x.hdr) {
              found = true;
              CHECK(got_h[q] == h.slot * 8 + (x.hdr & 7));
              // the whole header lies before every span's first bit
              CHECK(h.slot + kCkHdrSlot <= p.spans[0].in_pos);
            }
          CHECK(found);
        }
      }
      CHECK(j.ntok == e.ntok && j.tok_cap == e.ntok && j.tok_off == tok && j.tok_off % 64 == 0);
      tok += (e.ntok + 1 + 63) / 64 * 64;
      CHECK(c.tok_off == j.tok_off && c.ntok == e.ntok);
      CHECK(c.out_off == s.out_pos + e.out_off - v.e[s.first].out_off);
      CHECK(c.out_len == nx.out_off - e.out_off && j.out_len == c.out_len);
      CHECK(c.out_off + c.out_len <= p.dec_total);
      CHECK(c.seg_off <= c.out_off && c.seg_off >= s.out_pos);
    }
  }
  CHECK(units == p.units.size() && tok == p.tok_total && dec == p.dec_bytes);
  // header packing: exactly the wanted ones, once each, ascending, copied from inside the input
  CHECK(p.hdrs.size() == hdr_want.size());
  for (size_t i = 0; i < p.hdrs.size(); ++i) {
    const CkHdr &h = p.hdrs[i];
    CHECK(hdr_want.count(h.hdr) == 1);
    if (i) CHECK(h.hdr > p.hdrs[i - 1].hdr);
    CHECK(h.src == h.hdr / 8 && h.len <= kCkHdrBytesMax && h.src + h.len <= n && h.len <= kCkHdrSlot);
    CHECK(h.slot == i * kCkHdrSlot);
    inb += h.len;
  }
  CHECK(inb == p.in_bytes);
  // segments: tile the chain; one starts with every span and at every window
  // entry inside it that has output since; each names its own uploaded window
  uint32_t at = 0;
  std::set<uint32_t> wins_seen;
  CHECK(p.seg_win.size() == p.segs.size());
  for (size_t g = 0; g < p.segs.size() && g < p.seg_win.size(); ++g) {
    const SegJob &sg = p.segs[g];
    const int32_t win = p.seg_win[g];
    CHECK(sg.first == at && sg.count >= 1);
    const CkEntry &e = v.e[p.units[sg.first].entry];
    if (e.flags & 1) {
      CHECK(win >= 0 && (size_t)win < p.wins.size() && p.wins[win] == e.win);
      CHECK(wins_seen.insert(e.win).second);
    } else {
      CHECK(win < 0 && p.units[sg.first].entry == 0);
    }
    const uint64_t seg_off = p.chain[sg.first].out_off;
    CHECK(p.chain[sg.first].desc_off % 512 == 0);
    if (g) {
      const ChainUnit &pl = p.chain[at - 1];
      CHECK(p.chain[sg.first].desc_off >= pl.desc_off + pl.out_len);
    }
    for (uint32_t k = 0; k < sg.count; ++k) {
      const ChainUnit &c = p.chain[sg.first + k];
      CHECK(c.seg_off == seg_off);
      CHECK(c.desc_off == p.chain[sg.first].desc_off + (c.out_off - seg_off));
      CHECK(c.desc_off + c.out_len <= p.desc_total);
      // no window entry with output behind it in the middle of a segment
      if (k) {
        const CkEntry &x = v.e[p.units[sg.first + k].entry];
        const bool same_span = p.units[sg.first + k].entry == p.units[sg.first + k - 1].entry + 1;
        CHECK(same_span);
        CHECK(!(x.flags & 1) || c.out_off == seg_off);
      }
    }
    at += sg.count;
  }
  CHECK(at == p.chain.size());
  CHECK(wins_seen.size() == p.wins.size());
}

static void run_plan(const CkptView &v, size_t n, const std::vector<uint64_t> &off, const std::vector<uint64_t> &len) {
  const CkptPlan p = ckpt_plan(v, n, off.data(), len.data(), off.size());
  check_plan(v, p, off.data(), len.data(), off.size(), n);
}

int main() {
  const size_t sizes[] = {1, 2, 300};
  for (size_t nunits : sizes) {
    for (uint64_t start : {0ull, 10ull}) {
      const Synth s = synth(nunits, start, 1u << 20);
      const std::vector<uint8_t> b = blob_of(s);
      CkptView v;
      const char *why = validate(b, b.size(), s.n, &v);
      if (why) fprintf(stderr, "units %zu: %s\n", nunits, why);
      CHECK(why == nullptr);
      if (why) continue;
      CHECK(v.nunits == nunits && v.nwin == s.nwin && v.total_out == s.e.back().out_off);
      CHECK(v.win_units.size() == s.nwin + 1 && v.win_units[0] == 0);
      if (nunits == 300) CHECK(s.nwin >= 5);
      // windows: exactly the first entry at or after each positive multiple of span
      std::set<uint32_t> want;
      for (uint64_t m = s.span; m < v.total_out; m += s.span)
        for (uint32_t k = 1; k < v.nunits; ++k)
          if (v.e[k].out_off >= m) {
            want.insert(k);
            break;
          }
      std::set<uint32_t> have(v.win_units.begin() + 1, v.win_units.end());
      CHECK(want == have);
      const uint64_t T = v.total_out;
      // single ranges at the edges
      run_plan(v, s.n, {0}, {1});
      run_plan(v, s.n, {0}, {T});
      run_plan(v, s.n, {T ? T - 1 : 0}, {1});
      run_plan(v, s.n, {T}, {0});
      run_plan(v, s.n, {T}, {5});
      run_plan(v, s.n, {T + 1}, {1});
      run_plan(v, s.n, {T > 3 ? T - 3 : 0}, {100});  // across the last unit, clamped
      run_plan(v, s.n, {0}, {~0ull});
      run_plan(v, s.n, {}, {});
      // around every window entry: one byte before, at, straddling
      for (size_t i = 1; i < v.win_units.size(); ++i) {
        const uint64_t o = v.e[v.win_units[i]].out_off;
        run_plan(v, s.n, {o - 1}, {2});
        run_plan(v, s.n, {o}, {1});
        run_plan(v, s.n, {o - 1}, {1});
        // overlapping and touching ranges merge; a segment is cut at the window entry
        run_plan(v, s.n, {o - 10, o - 5, o + 5}, {5, 10, 7});
        const uint64_t o1[1] = {o - 1}, l1[1] = {2};
        const CkptPlan p = ckpt_plan(v, s.n, o1, l1, 1);
        CHECK(p.spans.size() == 1 && p.segs.size() == 2);
        if (p.segs.size() == 2)
          CHECK(p.seg_win.size() == 2 && p.seg_win[1] >= 0 && p.wins[p.seg_win[1]] == v.e[v.win_units[i]].win &&
                p.units[p.segs[1].first].entry == v.win_units[i]);
      }
      // random batches: unsorted, overlapping, repeated, some empty, some past the end
      for (int round = 0; round < 40; ++round) {
        std::vector<uint64_t> off, len;
        const int cnt = 1 + (int)(rnd() % 64);
        for (int i = 0; i < cnt; ++i) {
          off.push_back(T ? rnd() % (T + (rnd() % 8 == 0 ? 3 : 1)) : rnd() % 3);
          len.push_back(rnd() % 4 == 0 ? rnd() % 3 : rnd() % 200000);
          if (i && rnd() % 5 == 0) {
            off.back() = off[rnd() % i];
            len.back() = len[rnd() % i];
          }
        }
        run_plan(v, s.n, off, len);
      }
      if (nunits != 300) continue;
      // two ranges in neighbouring window spans that touch: one span, no unit twice
      {
        const uint64_t o = v.e[v.win_units[2]].out_off;
        const uint64_t o2[2] = {o, o - 1}, l2[2] = {1, 1};
        const CkptPlan p = ckpt_plan(v, s.n, o2, l2, 2);
        CHECK(p.spans.size() == 1);
      }
      // a far header named by every unit of the one-block half: packed once
      {
        const uint64_t o = v.e[v.win_units[1]].out_off, o2 = v.e[v.win_units[2]].out_off;
        const uint64_t o3[2] = {o, o2 + 1}, l3[2] = {1, 1};
        const CkptPlan p = ckpt_plan(v, s.n, o3, l3, 2);
        size_t far = 0;
        for (const CkHdr &h : p.hdrs) far += h.hdr == start * 8;
        CHECK(far == 1);
      }
      // ---- structural defects: each one alone must be refused
      auto refused = [&](std::vector<uint8_t> m, size_t len, size_t n_in) {
        CkptView t;
        return validate(m, len, n_in, &t) != nullptr;
      };
      CHECK(refused(b, b.size() - 1, s.n));                       // truncated
      CHECK(refused(b, kCkHeader, s.n));
      CHECK(refused(b, 0, s.n));
      CHECK(refused(b, b.size(), (s.e.back().pos + 7) / 8 - 1));   // end_ip past the input
      auto mutate = [&](size_t at, uint64_t val, int width) {
        std::vector<uint8_t> m = b;
        if (width == 4)
          idx_put32(m.data() + at, (uint32_t)val);
        else
          idx_put64(m.data() + at, val);
        return m;
      };
      const size_t E = kCkHeader, K = kCkEntry;
      const uint32_t wu = v.win_units[1], wu2 = v.win_units[2];
      CHECK(refused(mutate(0, 0x58495A54u, 4), b.size(), s.n));     // "TZIX": magic
      {
        std::vector<uint8_t> m = b;
        memcpy(m.data(), "ZTIX", 4);
        CHECK(refused(m, b.size(), s.n));
      }
      CHECK(refused(mutate(4, 2, 4), b.size(), s.n));               // version
      CHECK(refused(mutate(8, nunits + 1, 4), b.size(), s.n));      // nunits against the length
      CHECK(refused(mutate(8, 0, 4), b.size(), s.n));
      CHECK(refused(mutate(12, s.nwin + 1, 4), b.size(), s.n));     // nwin against the length
      CHECK(refused(mutate(12, s.nwin - 1, 4), b.size(), s.n));
      CHECK(refused(mutate(16, start + 1, 8), b.size(), s.n));      // stream_start against entry 0
      CHECK(refused(mutate(24, v.end_ip + 1, 8), b.size(), s.n));   // end_ip against the sentinel
      CHECK(refused(mutate(32, T + 1, 8), b.size(), s.n));          // total_out against the sentinel
      CHECK(refused(mutate(40, 65535, 8), b.size(), s.n));          // span below the minimum
      CHECK(refused(mutate(56, 1, 4), b.size(), s.n));              // header padding
      CHECK(refused(mutate(E + 24, CK_HUFF, 4), b.size(), s.n));    // entry 0: not a block start
      CHECK(refused(mutate(E + 32, 1, 4), b.size(), s.n));          // entry 0: a window
      CHECK(refused(mutate(E + 16, 1, 8), b.size(), s.n));          // entry 0: out_off
      CHECK(refused(mutate(E + 5 * K, 8 * s.n + 8, 8), b.size(), s.n));           // pos beyond n
      CHECK(refused(mutate(E + 5 * K, v.e[4].pos - 1, 8), b.size(), s.n));        // pos decreases
      CHECK(refused(mutate(E + 5 * K + 16, v.e[4].out_off - 1, 8), b.size(), s.n));  // out_off decreases
      CHECK(refused(mutate(E + 5 * K + 16, T + 1, 8), b.size(), s.n));
      CHECK(refused(mutate(E + 5 * K + 24, 4, 4), b.size(), s.n));  // kind FINAL before the sentinel
      CHECK(refused(mutate(E + 5 * K + 24, 9, 4), b.size(), s.n));  // unknown kind
      CHECK(refused(mutate(E + 6 * K + 8, v.e[6].pos, 8), b.size(), s.n));        // hdr not before pos
      CHECK(refused(mutate(E + 6 * K + 8, v.e[6].pos + 99, 8), b.size(), s.n));
      CHECK(refused(mutate(E + 6 * K + 32, 4, 4), b.size(), s.n));  // unknown flag
      CHECK(refused(mutate(E + 6 * K + 44, 1, 4), b.size(), s.n));  // entry padding
      CHECK(refused(mutate(E + 6 * K + 36, (uint32_t)(v.e[7].pos - v.e[6].pos) + 1, 4), b.size(), s.n));  // ntok over the bits
      CHECK(refused(mutate(E + 6 * K + 36, 1, 4), b.size(), s.n));  // output over what the tokens give
      CHECK(refused(mutate(E + 6 * K + 28, 1, 4), b.size(), s.n));  // rem on a Huffman entry
      {
        // a stored entry: rem past the input, rem 0, a bit position off the byte, a header
        uint32_t st = 0;
        for (uint32_t k = 1; k < v.nunits; ++k)
          if (v.e[k].kind == CK_STORED) st = k;
        CHECK(st != 0);
        CHECK(refused(mutate(E + st * K + 28, 65536, 4), b.size(), s.n));
        CHECK(refused(mutate(E + st * K + 28, 0, 4), b.size(), s.n));
        CHECK(refused(mutate(E + st * K + 8, 8 * start + 1, 8), b.size(), s.n));
        std::vector<uint8_t> m = b;
        idx_put32(m.data() + E + (nunits - 1) * K + 24, CK_STORED);
        idx_put64(m.data() + E + (nunits - 1) * K + 8, 0);
        idx_put64(m.data() + E + (nunits - 1) * K, v.e[nunits - 1].pos & ~7ull);
        idx_put32(m.data() + E + (nunits - 1) * K + 28, 60000);  // the payload runs past end_ip
        CHECK(refused(m, b.size(), s.n));
      }
      // windows: index out of range, repeated, on an entry without the flag, too early, count
      CHECK(refused(mutate(E + wu * K + 40, s.nwin, 4), b.size(), s.n));
      CHECK(refused(mutate(E + wu2 * K + 40, 0, 4), b.size(), s.n));              // window 0 named twice
      CHECK(refused(mutate(E + wu * K + 32, v.e[wu].flags & ~1u, 4), b.size(), s.n));  // flag gone: win without it, count
      CHECK(refused(mutate(E + 2 * K + 32, v.e[2].flags | 1u, 4), b.size(), s.n));     // an extra window entry
      // sentinel
      const size_t S = E + nunits * K;
      CHECK(refused(mutate(S + 24, CK_BLOCK, 4), b.size(), s.n));
      CHECK(refused(mutate(S + 16, T - 1, 8), b.size(), s.n));
      CHECK(refused(mutate(S + 36, 1, 4), b.size(), s.n));
      CHECK(refused(mutate(S + 32, 2, 4), b.size(), s.n));
      CHECK(refused(mutate(S, v.e[nunits].pos + 8, 8), b.size(), s.n));
      // a sync-point index is not a checkpoint blob, nor the other way round
      {
        std::vector<uint8_t> ix(index_blob_bytes(1));
        index_write_header(ix.data(), 1, 1, 0, 8, 100);
        index_write_entry(ix.data(), 0, IdxEntry{0, 0, 50, 1});
        index_write_entry(ix.data(), 1, IdxEntry{8, 100, 0, 0});
        IndexView iv;
        CHECK(index_validate(ix.data(), ix.size(), 8, &iv) == nullptr);
        CHECK(refused(ix, ix.size(), 8));
        CHECK(index_validate(b.data(), b.size(), s.n, &iv) != nullptr);
      }
    }
  }
  // a window entry less than 32 KiB into the output (no build writes one)
  {
    Synth s = synth(300, 0, 1u << 20);
    s.e[1].out_off = 1000;
    for (CkEntry &x : s.e)
      if (x.flags & 1) x.win++;
    s.e[1].flags |= 1;
    s.e[1].win = 0;
    s.nwin++;
    CHECK(s.e[1].out_off < 32768);
    const std::vector<uint8_t> b = blob_of(s);
    CkptView v;
    CHECK(validate(b, b.size(), s.n, &v) != nullptr);
  }
  if (fails) {
    fprintf(stderr, "ckpt_host_check: %d checks failed\n", fails);
    return 1;
  }
  printf("ckpt_host_check ok\n");
  return 0;
}
