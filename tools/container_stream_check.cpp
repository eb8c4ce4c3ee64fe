// container_stream_check.cpp -- host-only check of the container sessions'
// framing (zlib.ts_amd/csrc/container_stream_host.h): the incremental header
// test at every split of headers with every flag combination against
// gzip_parse_header on the whole header, the AUTO decision, ISIZE modulo 2^32,
// the dictionary id, and cs_step driven over whole files cut at every
// position with a model body decoder (the body's length, CRC-32 and Adler-32
// are known to the model): members, offsets, the trailer split across feeds,
// the first feed that can decide an error, the zlib FDICT cases.
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/container_stream_check.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../zlib.ts_amd/csrc/container_stream_host.h"

using namespace zt;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

typedef std::vector<uint8_t> Bytes;

static void put32(Bytes &b, uint32_t v) {
  for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(v >> (8 * k)));
}

// a gzip header: flags, FEXTRA of xlen bytes, name / comment with or without their terminator
static Bytes gz_header(uint32_t flg, size_t xlen, const char *name, bool name_z, const char *comment, bool comment_z,
                       bool good_hcrc = true) {
  Bytes h = {0x1F, 0x8B, 8, (uint8_t)flg, 1, 2, 3, 4, 2, 3};
  if (flg & 0x04) {
    h.push_back((uint8_t)(xlen & 0xFF));
    h.push_back((uint8_t)(xlen >> 8));
    for (size_t k = 0; k < xlen; ++k) h.push_back((uint8_t)(k * 7 + 1));  // (zeros inside are no terminators)
  }
  if (flg & 0x08) {
    h.insert(h.end(), name, name + strlen(name));
    if (name_z) h.push_back(0);
  }
  if (flg & 0x10) {
    h.insert(h.end(), comment, comment + strlen(comment));
    if (comment_z) h.push_back(0);
  }
  if (flg & 0x02) {
    const uint32_t c = crc32_small(h.data(), h.size()) & 0xFFFF;
    h.push_back((uint8_t)(good_hcrc ? c : c ^ 1));
    h.push_back((uint8_t)(c >> 8));
  }
  return h;
}

// ---- the header test at every split -------------------------------------------------
static void check_header_scan() {
  size_t cases = 0;
  for (uint32_t flg = 0; flg < 32; flg += 2)  // FHCRC, FEXTRA, FNAME, FCOMMENT
    for (const size_t xlen : {size_t(0), size_t(5), size_t(65535)})
      for (const char *name : {"", "n.txt"})
        for (const char *comment : {"", "a comment"}) {
          if (!(flg & 0x04) && xlen) continue;
          const Bytes h = gz_header(flg, xlen, name, true, comment, true);
          zt_gzip_member whole;
          size_t body = 0;
          GzError ge;
          CHECK(gzip_parse_header(h.data(), h.size(), 0, &whole, &body, &ge) == ZT_OK && body == h.size());
          // with body bytes behind it the answer is the same
          Bytes more = h;
          more.insert(more.end(), 40, 0);
          for (size_t cut = 0; cut <= more.size(); ++cut) {
            if (xlen == 65535 && cut > 40 && cut + 40 < h.size() && cut % 977) continue;  // (inside FEXTRA: sampled)
            const GzHeaderScan sc = gz_header_scan(more.data(), cut);
            CHECK(sc.decided == (cut >= h.size()));
            if (sc.decided) {
              CHECK(sc.len == h.size());
              zt_gzip_member m;
              size_t b2 = 0;
              CHECK(gzip_parse_header(more.data(), sc.len, 0, &m, &b2, &ge) == ZT_OK && b2 == body);
              CHECK(!memcmp(&m, &whole, sizeof m));
            } else {
              // an incomplete header is what gzip_parse_header refuses on the same bytes
              zt_gzip_member m;
              size_t b2 = 0;
              CHECK(gzip_parse_header(more.data(), cut, 0, &m, &b2, &ge) != ZT_OK);
            }
          }
          cases++;
        }
  CHECK(cases == 16 * 4 + 8 * 8);
  // unterminated strings: never complete, however many bytes
  for (const uint32_t flg : {0x08u, 0x10u, 0x18u, 0x1Au}) {
    const Bytes h = gz_header(flg & ~0x02u, 0, "name", (flg & 0x18) == 0x18, "comment", false);
    for (size_t cut = 0; cut <= h.size(); ++cut) CHECK(!gz_header_scan(h.data(), cut).decided);
    zt_gzip_member m;
    size_t body = 0;
    GzError ge;
    CHECK(gzip_parse_header(h.data(), h.size(), 0, &m, &body, &ge) == ZT_E_INPUT_BROKEN);
  }
  // fields that fail are decided when they are complete
  const uint8_t sig[] = {0x1F, 0x8C, 8, 0};
  CHECK(!gz_header_scan(sig, 1).decided);
  CHECK(gz_header_scan(sig, 2).decided && gz_header_scan(sig, 2).len == 2 && gz_header_scan(sig, 4).len == 2);
  const uint8_t cm[] = {0x1F, 0x8B, 7, 0};
  CHECK(!gz_header_scan(cm, 2).decided && gz_header_scan(cm, 3).decided && gz_header_scan(cm, 4).len == 3);
}

static void check_auto_isize_adler() {
  for (uint32_t a = 0; a < 256; ++a)
    for (uint32_t b = 0; b < 256; ++b) {
      const uint8_t p[2] = {(uint8_t)a, (uint8_t)b};
      const bool gz = a == 0x1F && b == 0x8B;
      const bool zl = (a & 15) == 8 && (a * 256 + b) % 31 == 0;
      CHECK(!(gz && zl));
      CHECK(cs_auto(p, 2) == (zl ? CS_ZLIB : CS_GZIP));
      CHECK(cs_auto(p, 1) == CS_GZIP && cs_auto(p, 0) == CS_GZIP);
    }
  CHECK(cs_isize(0) == 0 && cs_isize(0xFFFFFFFFull) == 0xFFFFFFFFu);
  CHECK(cs_isize(1ull << 32) == 0 && cs_isize((1ull << 32) + 5) == 5 && cs_isize((7ull << 32) | 0x80000001u) == 0x80000001u);
  for (uint64_t len : {0ull, 1ull, 0xFFFFFFFFull, 0x100000000ull, 0x1234567890ull}) {
    // the trailer check of a member that long: ISIZE is the length's low word
    Bytes t;
    put32(t, 0xCAFEF00Du);
    put32(t, (uint32_t)(len % 4294967296ull));
    zt_gzip_member m;
    size_t next = 0;
    GzError ge;
    CHECK(gzip_check_trailer(t.data(), 8, 0, 0xCAFEF00Du, (size_t)cs_isize(len), &m, &next, &ge) == ZT_OK && next == 8);
    CHECK(gzip_check_trailer(t.data(), 8, 0, 0xCAFEF00Du, (size_t)cs_isize(len + 1), &m, &next, &ge) == ZT_E_GZIP_ISIZE);
  }
  Bytes d(70000);
  for (size_t k = 0; k < d.size(); ++k) d[k] = (uint8_t)(k * 31 + (k >> 8));
  for (const size_t n : {size_t(0), size_t(1), size_t(5552), size_t(5553), size_t(70000)}) {
    uint32_t s1 = 1, s2 = 0;
    for (size_t k = 0; k < n; ++k) {
      s1 = (s1 + d[k]) % 65521;
      s2 = (s2 + s1) % 65521;
    }
    CHECK(adler32_small(d.data(), n) == (s1 | (s2 << 16)));
  }
  CHECK(cs_end_bits(100, 0, 10, 3) == 90 * 8 + 3 && cs_end_bits(100, 7, 0, 0) == 93 * 8);
}

// ---- cs_step over whole files, with a model body ---------------------------------------
struct ModelMember {
  size_t body_at, body_len;  // the DEFLATE bytes in the file
  uint32_t crc, adler;
  uint64_t out_len;
};
struct Outcome {
  int code = ZT_OK;
  std::string msg;
  size_t decided_at = 0;  // bytes fed when the error was reported
  bool finished = false;
  uint64_t members_done = 0, unused = 0;
  bool at_member_end = false;
  std::deque<CsMember> members;
  size_t turns = 0;
};
// Feeds file[0 .. cuts[0]), [cuts[0] .. cuts[1]) ...; the last feed has `last`.
// The model body decoder consumes a body's bytes as they arrive and knows its end.
static Outcome drive(CsFrame f, const Bytes &file, const std::vector<ModelMember> &model, std::vector<size_t> cuts) {
  Outcome o;
  Bytes pending;
  size_t fed = 0, body_left = 0, mi = 0;
  cuts.push_back(file.size());
  for (size_t c = 0; c < cuts.size(); ++c) {
    const int last = c + 1 == cuts.size();
    pending.insert(pending.end(), file.begin() + fed, file.begin() + cuts[c]);
    fed = cuts[c];
    if (f.state == CS_DONE) {
      f.unused += pending.size();
      pending.clear();
      continue;
    }
    size_t used = 0;
    for (;;) {
      if (f.state == CS_BODY) {
        const size_t take = std::min(body_left, pending.size() - used);
        used += take;
        body_left -= take;
        if (body_left) {
          if (last) {
            o.code = ZT_E_INPUT_BROKEN;
            o.msg = "input buffer is broken";
            o.decided_at = fed;
            return o;
          }
          break;
        }
        f.crc = model[mi].crc;
        f.adler = model[mi].adler;
        f.member_out = model[mi].out_len;
        mi++;
        f.state = CS_TRAILER;
      }
      const CsStep st = cs_step(&f, pending.data() + used, pending.size() - used, last, fed - pending.size() + used);
      used += st.consumed;
      CHECK(used <= pending.size());
      if (st.action == CS_ACT_ERROR) {
        o.code = f.code;
        o.msg = f.msg;
        o.decided_at = fed;
        o.members_done = f.members_done;
        return o;
      }
      if (st.action == CS_ACT_DONE) {
        f.unused += pending.size() - used;
        used = pending.size();
        break;
      }
      if (st.action == CS_ACT_WAIT) break;
      CHECK(st.action == CS_ACT_BODY && f.state == CS_BODY);
      CHECK(mi < model.size() && fed - pending.size() + used == model[mi].body_at);
      o.turns += st.turn;
      body_left = model[mi].body_len;
    }
    pending.erase(pending.begin(), pending.begin() + used);
    CHECK(pending.size() <= 8 || f.state == CS_HEADER || f.state == CS_START);  // only a header is carried whole
  }
  o.finished = f.state == CS_DONE;
  o.members_done = f.members_done;
  o.unused = f.unused;
  o.at_member_end = f.at_member_end() && pending.empty();
  o.members = f.members;
  return o;
}

static void check_gzip_files() {
  // three members: all header fields, a bare one with an empty-ish body, FHCRC on a later member
  Bytes file;
  std::vector<ModelMember> model;
  std::vector<size_t> starts, hlens;
  const Bytes heads[3] = {gz_header(0x1E, 9, "first", true, "c", true), gz_header(0, 0, "", true, "", true),
                          gz_header(0x0A, 0, "third", true, "", true)};
  const size_t blen[3] = {23, 2, 11};
  const uint64_t olen[3] = {1000, 0, (1ull << 32) + 77};
  for (int k = 0; k < 3; ++k) {
    starts.push_back(file.size());
    hlens.push_back(heads[k].size());
    file.insert(file.end(), heads[k].begin(), heads[k].end());
    ModelMember mm{file.size(), blen[k], 0x1000u + k, 0x2000u + k, olen[k]};
    model.push_back(mm);
    for (size_t b = 0; b < blen[k]; ++b) file.push_back((uint8_t)(0xA0 + b));
    put32(file, mm.crc);
    put32(file, (uint32_t)olen[k]);
  }
  CsFrame f0;
  f0.init(CS_GZIP, 1);
  CsFrame fa;
  fa.init(CS_AUTO, 1);
  for (size_t cut = 0; cut <= file.size(); ++cut)
    for (size_t cut2 = cut; cut2 <= file.size(); cut2 += (cut % 5 ? 97 : 1)) {
      const Outcome o = drive(cut2 % 2 ? f0 : fa, file, model, {cut, cut2});
      CHECK(o.code == ZT_OK && o.finished && o.members_done == 3 && o.at_member_end && o.unused == 0);
      CHECK(o.turns == 2);
      uint64_t off = 0;
      for (int k = 0; k < 3; ++k) {
        const CsMember &m = o.members[k];
        CHECK(m.in_off == starts[k] && m.data_off == off && m.data_len == olen[k]);
        CHECK(m.m.crc32 == model[k].crc && m.m.isize == (uint32_t)olen[k]);
        off += olen[k];
      }
      CHECK(o.members[0].name == "first" && o.members[0].comment == "c" && o.members[0].m.xlen == 9);
      CHECK(o.members[2].name == "third" && o.members[2].m.has_crc16 == 1);  // (its CRC over its own header)
      CHECK(o.members[1].name.empty() && o.members[1].m.flg == 0);
    }
  // one byte per feed
  {
    std::vector<size_t> cuts;
    for (size_t k = 1; k < file.size(); ++k) cuts.push_back(k);
    const Outcome o = drive(f0, file, model, cuts);
    CHECK(o.code == ZT_OK && o.finished && o.members_done == 3);
  }
  // without `last` knowledge: at every member end the session is at_member_end
  for (int k = 0; k < 3; ++k) {
    const size_t end = model[k].body_at + model[k].body_len + 8;
    Bytes part(file.begin(), file.begin() + end);
    const Outcome o = drive(f0, part, model, {end / 2});
    CHECK(o.code == ZT_OK && o.finished && o.members_done == (uint64_t)k + 1);
  }
  // errors: decided by the first feed that can, with the one-shot text
  struct Bad {
    size_t at;        // byte to flip
    int code;
    size_t decided;   // bytes that decide
  };
  const size_t t0 = model[0].body_at + model[0].body_len;
  const Bad bads[] = {{0, ZT_E_GZIP_SIGNATURE, 2},
                      {2, ZT_E_GZIP_METHOD, 3},
                      {hlens[0] - 1, ZT_E_GZIP_HCRC, hlens[0]},
                      {t0 + 1, ZT_E_GZIP_CRC32, t0 + 8},
                      {t0 + 6, ZT_E_GZIP_ISIZE, t0 + 8},
                      {starts[1] + 1, ZT_E_GZIP_SIGNATURE, starts[1] + 2},
                      {starts[2] + hlens[2] - 2, ZT_E_GZIP_HCRC, starts[2] + hlens[2]}};
  for (const Bad &b : bads) {
    Bytes bad = file;
    bad[b.at] ^= 0x40;
    for (size_t cut = 0; cut <= bad.size(); ++cut) {
      const Outcome o = drive(f0, bad, model, {cut});
      CHECK(o.code == b.code);
      CHECK(o.decided_at == (cut >= b.decided ? cut : bad.size()));
      if (b.at < starts[1]) {  // the one-shot text of the first member's checks
        zt_gzip_member m;
        size_t body = 0, next = 0;
        GzError ge;
        if (b.at < hlens[0])
          gzip_parse_header(bad.data(), bad.size(), 0, &m, &body, &ge);
        else
          gzip_check_trailer(bad.data(), bad.size(), t0, model[0].crc, (size_t)olen[0], &m, &next, &ge);
        CHECK(ge.code == b.code && o.msg == ge.msg);
      }
    }
  }
  // truncation at every length, `last` on the one feed: what the one-shot
  // checks give on the same bytes (the body's own truncation is the decoder's)
  for (size_t n = 0; n < file.size(); ++n) {
    Bytes part(file.begin(), file.begin() + n);
    const Outcome o = drive(f0, part, model, {n / 2});
    size_t ip = 0;
    int want = ZT_OK;
    std::string text;
    for (int k = 0; k < 3 && ip < n; ++k) {
      zt_gzip_member m;
      size_t body = 0, next = 0;
      GzError ge;
      // (later members: the header check on the member's own bytes)
      if (gzip_parse_header(part.data() + ip, n - ip, 0, &m, &body, &ge)) {
        want = ge.code;
        text = ge.msg;
        break;
      }
      if (model[k].body_at + model[k].body_len > n) {
        want = ZT_E_INPUT_BROKEN;
        text = "input buffer is broken";
        break;
      }
      if (gzip_check_trailer(part.data(), n, model[k].body_at + model[k].body_len, model[k].crc, (size_t)cs_isize(olen[k]),
                             &m, &next, &ge)) {
        want = ge.code;
        text = ge.msg;
        break;
      }
      ip = next;
    }
    CHECK(o.code == want && o.msg == text);
    if (!want) CHECK(o.finished);
  }
  // the carry buffer's bound
  {
    Bytes big = gz_header(0x08, 0, "", false, "", false);
    big.resize(kCsHeaderMax + 1, 'x');
    CsFrame f = f0;
    const CsStep st = cs_step(&f, big.data(), big.size() - 1, 0, 0);
    CHECK(st.action == CS_ACT_WAIT);
    const CsStep st2 = cs_step(&f, big.data(), big.size(), 0, 0);
    CHECK(st2.action == CS_ACT_ERROR && f.code == ZT_E_ARG && f.msg == "gzip header fields exceed 1 MiB");
  }
}

static void check_zlib() {
  Bytes dict(40000);
  for (size_t k = 0; k < dict.size(); ++k) dict[k] = (uint8_t)(k % 251);
  const uint32_t id = adler32_small(dict.data(), dict.size());
  for (int fdict = 0; fdict < 2; ++fdict) {
    Bytes file = {0x78, (uint8_t)(fdict ? 0xBB : 0x9C)};
    CHECK((file[0] * 256 + file[1]) % 31 == 0);
    if (fdict)
      for (int k = 3; k >= 0; --k) file.push_back((uint8_t)(id >> (8 * k)));
    const ModelMember mm{file.size(), 17, 0, 0x11223344u, 555};
    file.insert(file.end(), 17, 0x55);
    for (int k = 3; k >= 0; --k) file.push_back((uint8_t)(mm.adler >> (8 * k)));
    file.insert(file.end(), 5, 0xEE);  // trailing bytes
    for (const int fmt : {CS_ZLIB, CS_AUTO})
      for (size_t cut = 0; cut <= file.size(); ++cut) {
        CsFrame f;
        f.init(fmt, 1);
        f.has_dict = true;
        f.dict_id = id;
        f.dict_len = dict_window_len(dict.size());
        const Outcome o = drive(f, file, {mm}, {cut, std::min(file.size(), cut + 3)});
        CHECK(o.code == ZT_OK && o.finished && o.members_done == 1 && o.unused == 5);
        CHECK(o.turns == (size_t)fdict && o.members[0].data_len == 555 && o.members[0].m.crc32 == mm.adler);
        // FDICT without a dictionary, and with another one: decided when the field is complete
        CsFrame none;
        none.init(fmt, 1);
        const Outcome o2 = drive(none, file, {mm}, {cut});
        CHECK(o2.code == (fdict ? ZT_E_ZLIB_FDICT : ZT_OK));
        if (fdict) CHECK(o2.msg == "fdict flag is not supported" && o2.decided_at == (cut >= 2 ? cut : file.size()));
        CsFrame other = f;
        other.dict_id = id ^ 0x100;
        const Outcome o3 = drive(other, file, {mm}, {cut});
        CHECK(o3.code == (fdict ? ZT_E_ZLIB_DICTID : ZT_OK));
        if (fdict) {
          char text[96];
          snprintf(text, sizeof text, "invalid dictionary id: 0x%x / 0x%x", id, id ^ 0x100);
          CHECK(o3.msg == text && o3.decided_at == (cut >= 6 ? cut : file.size()));
        }
        // a flipped Adler-32: with verify only
        Bytes bad = file;
        bad[mm.body_at + mm.body_len + 2] ^= 1;
        const Outcome o4 = drive(f, bad, {mm}, {cut});
        CHECK(o4.code == ZT_E_ZLIB_ADLER && o4.msg == "invalid adler-32 checksum");
        CHECK(o4.decided_at == (cut >= mm.body_at + mm.body_len + 4 ? cut : bad.size()));
        CsFrame loose = f;
        loose.verify = 0;
        const Outcome o5 = drive(loose, bad, {mm}, {cut});
        CHECK(o5.code == ZT_OK && o5.finished && o5.unused == 5);
      }
    // truncated DICTID
    if (fdict) {
      Bytes part(file.begin(), file.begin() + 4);
      CsFrame f;
      f.init(CS_ZLIB, 1);
      f.has_dict = true;
      f.dict_id = id;
      const Outcome o = drive(f, part, {mm}, {2});
      CHECK(o.code == ZT_E_INPUT_BROKEN && o.msg == "input buffer is broken");
    }
  }
  // header errors, with the one-shot texts
  struct Z {
    Bytes in;
    int code;
    const char *msg;
  };
  const Z zs[] = {{{}, ZT_E_ZLIB_METHOD, "unsupported compression method"},
                  {{0x77, 0x00}, ZT_E_ZLIB_METHOD, "unsupported compression method"},
                  {{0x78}, ZT_E_ZLIB_FCHECK, "invalid fcheck flag:NaN"},
                  {{0x78, 0x9D}, ZT_E_ZLIB_FCHECK, "invalid fcheck flag:1"}};
  for (const Z &z : zs)
    for (size_t cut = 0; cut <= z.in.size(); ++cut) {
      CsFrame f;
      f.init(CS_ZLIB, 1);
      const Outcome o = drive(f, z.in, {}, {cut});
      CHECK(o.code == z.code && o.msg == z.msg);
    }
  // AUTO on bytes that are neither: the gzip signature error
  {
    const Bytes junk = {0x50, 0x4B, 3, 4};
    CsFrame f;
    f.init(CS_AUTO, 1);
    const Outcome o = drive(f, junk, {}, {1});
    CHECK(o.code == ZT_E_GZIP_SIGNATURE && o.msg == "invalid file signature:80,75");
    CsFrame e;
    e.init(CS_AUTO, 1);
    const Outcome o2 = drive(e, {}, {}, {0});
    CHECK(o2.code == ZT_OK && o2.finished && o2.at_member_end);
  }
}

// ---- where a truncated body ends -----------------------------------------------------
struct BitOut {
  Bytes b;
  uint64_t pos = 0;
  void bits(uint32_t v, int k) {  // LSB first
    for (int i = 0; i < k; ++i, ++pos) {
      if ((pos & 7) == 0) b.push_back(0);
      b[pos >> 3] |= (uint8_t)(((v >> i) & 1) << (pos & 7));
    }
  }
  void code(uint32_t v, int k) {  // a Huffman code: MSB first
    for (int i = k - 1; i >= 0; --i) bits((v >> i) & 1, 1);
  }
  void fixed_lit(int c) { c < 144 ? code(0x30 + c, 8) : code(0x190 + c - 144, 9); }
};

static void check_truncation() {
  // a fixed block "ab", then a final stored block of 5 bytes
  BitOut o;
  o.bits(0, 1);
  o.bits(1, 2);
  o.fixed_lit('a');
  const uint64_t after_a = o.pos;
  o.fixed_lit(200);
  o.code(0, 7);  // end of block
  const uint64_t header = o.pos;
  o.bits(1, 1);
  o.bits(0, 2);
  const size_t p = (size_t)((o.pos + 7) >> 3);
  Bytes s = o.b;
  s.resize(p);
  for (const uint8_t v : {5, 0, 0xFA, 0xFF, 1, 2, 3, 4, 5}) s.push_back(v);
  CHECK(after_a == 11 && header == 3 + 8 + 9 + 7 && p == 4 && s.size() == 13);
  const uint8_t none[320] = {0};
  for (size_t n = 0; n <= s.size(); ++n) {
    const CsTruncation want = n < p            ? CS_TRUNC_OTHER
                              : n <= p + 1     ? CS_TRUNC_STORED_LEN
                              : n <= p + 3     ? CS_TRUNC_STORED_NLEN
                                               : CS_TRUNC_OTHER;
    CHECK(cs_truncation(s.data(), n, 0, SP_HEADER, 0, 0, 0, 0, 0, none) == want);
    // from inside the fixed block, and from the stored block's header
    if (n >= 2) CHECK(cs_truncation(s.data(), n, after_a, SP_HUFF, 0, 1, 0, 0, 0, none) == want);
    if (n >= p) CHECK(cs_truncation(s.data() + 3, n - 3, header - 24, SP_HEADER, 0, 1, 0, 0, 0, none) == want);
  }
  // inside a stored payload, and behind a stored block that ended
  CHECK(cs_truncation(s.data() + 8, 3, 0, SP_STORED, 1, 0, 4, 0, 0, none) == CS_TRUNC_OTHER);
  const uint8_t next[] = {9, 9, 0x01};  // two payload bytes, then a stored header and nothing more
  CHECK(cs_truncation(next, 3, 0, SP_STORED, 0, 0, 2, 0, 0, none) == CS_TRUNC_STORED_LEN);
  // a dynamic block: lengths {1, 1} for literals 0 and 256 only, then a stored header
  BitOut d;
  d.bits(0, 1);
  d.bits(2, 2);
  d.bits(0, 5);   // HLIT 257
  d.bits(0, 5);   // HDIST 1
  d.bits(14, 4);  // HCLEN 18: code-length codes 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1
  const int cll[18] = {0, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2};  // 18: 1 bit, 0 and 1: 2 bits
  for (int k = 0; k < 18; ++k) d.bits((uint32_t)cll[k], 3);
  // codes: 18 -> 0, 0 -> 10, 1 -> 11
  d.code(3, 2);               // literal 0: length 1
  d.code(0, 1), d.bits(127, 7);  // 138 zeros
  d.code(0, 1), d.bits(106, 7);  // 117 zeros: 1 + 138 + 117 = 256
  d.code(3, 2);               // 256: length 1
  d.code(2, 2);               // the one distance code: length 0
  d.code(0, 1);               // literal 0
  d.code(1, 1);               // end of block
  d.bits(1, 1), d.bits(0, 2);  // a final stored block
  const size_t dp = (size_t)((d.pos + 7) >> 3);
  Bytes ds = d.b;
  ds.resize(dp);
  for (size_t n = 0; n <= dp + 3; ++n) {
    Bytes part(ds);
    part.resize(n, 0);
    const CsTruncation want = n < dp ? CS_TRUNC_OTHER : n <= dp + 1 ? CS_TRUNC_STORED_LEN : CS_TRUNC_STORED_NLEN;
    CHECK(cs_truncation(part.data(), n, 0, SP_HEADER, 0, 0, 0, 0, 0, none) == want);
  }
}

// ---- the bytes a member record hands out stay where they are --------------------------
// zt_container_session_member returns pointers into a member's name and
// comment; they are promised to live as long as the session, so adding later
// members must not move a member (short strings keep their bytes inside the
// object).  Under ASan a moved member's old bytes are freed memory.
static void check_member_addresses() {
  CsFrame f;
  f.init(CS_GZIP, 1);
  std::vector<const char *> names, comments;
  std::vector<const CsMember *> where;
  uint64_t pos = 0;
  for (int k = 0; k < 200; ++k) {
    char name[16], comment[48];
    snprintf(name, sizeof name, "n%d", k);                                   // short: inside the string object
    snprintf(comment, sizeof comment, "a comment long enough for the heap %d", k);
    Bytes h = gz_header(0x18, 0, name, true, comment, true);
    CsStep st = cs_step(&f, h.data(), h.size(), 0, pos);
    CHECK(st.action == CS_ACT_BODY && st.consumed == h.size() && f.state == CS_BODY);
    pos += h.size();
    f.crc = 7u + k;
    f.member_out = k;
    f.state = CS_TRAILER;
    Bytes t;
    put32(t, 7u + k);
    put32(t, (uint32_t)k);
    st = cs_step(&f, t.data(), t.size(), 0, pos);
    CHECK(st.action == CS_ACT_WAIT && st.consumed == 8 && f.members_done == (uint64_t)k + 1);
    pos += 8;
    const CsMember &m = f.members[k];
    where.push_back(&m);
    names.push_back(m.name.data());
    comments.push_back(m.comment.data());
    // every pointer handed out so far still reads the member's bytes
    for (int q = 0; q <= k; q += (k < 20 ? 1 : 17)) {
      snprintf(name, sizeof name, "n%d", q);
      snprintf(comment, sizeof comment, "a comment long enough for the heap %d", q);
      CHECK(where[q] == &f.members[q] && names[q] == f.members[q].name.data());
      CHECK(!strcmp(names[q], name) && !strcmp(comments[q], comment));
    }
  }
}

int main() {
  static_assert(sizeof(SessTurn) == 16, "turn record");
  check_member_addresses();
  check_truncation();
  check_header_scan();
  check_auto_isize_adler();
  check_gzip_files();
  check_zlib();
  printf("container_stream_check ok\n");
  return 0;
}
