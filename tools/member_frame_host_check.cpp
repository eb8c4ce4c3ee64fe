// tools/member_frame_host_check.cpp -- drives zlib.ts_amd/csrc/member_frame.h
// (the one description of a gzip / zlib / raw member's prefix, trailer and
// stored blocks) and dict_host.h's zlib_header_status without a device, each
// against a slow restatement or the exact bytes.  The stored blocks are also
// compared with what dev_stored_jobs' copy and patch jobs give when the host
// model of the kernels (tools/dev_batch_model.h) runs them.  Meant to be built
// with a sanitizer and run on its own (tests/test_member_frame_host.py):
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o member_frame_host_check tools/member_frame_host_check.cpp
//   ./member_frame_host_check
//
// Every buffer is a heap allocation of exactly its bytes.  Prints
// "member_frame_host_check ok"; exit 1 on a broken invariant.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../zlib.ts_amd/csrc/dict_host.h"
#include "../zlib.ts_amd/csrc/member_frame.h"
#include "dev_batch_model.h"

typedef std::vector<uint8_t> Bytes;

static void check_zlib_header() {
  const uint8_t want[2][4] = {{0x01, 0x5E, 0x9C, 0xDA}, {0x20, 0x7D, 0xBB, 0xF9}};
  for (int fdict = 0; fdict < 2; ++fdict)
    for (uint32_t flevel = 0; flevel < 4; ++flevel) {
      const Bytes h = zlib_cmf_flg(flevel, fdict != 0);
      CHECK(h.size() == 2 && h[0] == 0x78 && h[1] == want[fdict][flevel]);
      CHECK(((h[0] << 8) + h[1]) % 31 == 0);
      // both forms the writers used to spell, each where it was in use: the
      // first never met FDICT, and 0x7820 is the one value with remainder 0,
      // where it would give FCHECK 31
      const uint32_t cmf = 0x78, flg0 = (flevel << 6) | (fdict ? 0x20u : 0u), rem = ((cmf << 8) + flg0) % 31;
      if (!fdict) CHECK(h[1] == (uint8_t)(flg0 | (31 - ((cmf << 8) + flg0) % 31)));
      CHECK(h[1] == (uint8_t)(flg0 | (rem ? 31 - rem : 0)));
      CHECK((rem == 0) == (fdict && flevel == 0));
      // the frames built from it, read back
      const uint32_t id = 0xA1B2C3D4u + flevel;
      const MemberFrame fr = fdict ? frame_zlib_dict(flevel, id) : frame_zlib(flevel);
      CHECK(fr.kind == kFmtZlib && fr.trailer_len() == 4 && fr.prefix_len() == (fdict ? 6u : 2u));
      CHECK(fr.prefix[0] == h[0] && fr.prefix[1] == h[1]);
      Bytes in(3, 0xEE);  // (parsed at an offset)
      in.insert(in.end(), fr.prefix.begin(), fr.prefix.end());
      ZlibHeader zh;
      CHECK(zlib_parse_header(in.data(), in.size(), 3, &zh) == ZH_OK);
      CHECK(zh.fdict == fdict && zh.dictid == (fdict ? id : 0u) && zh.body == 3 + fr.prefix.size());
    }
}

static void check_gzip_header() {
  const uint8_t fixed[10] = {0x1F, 0x8B, 0x08, 0, 0, 0, 0, 0, 0, 0x03};
  const MemberFrame plain = frame_gzip(nullptr);
  CHECK(plain.kind == kFmtGzip && plain.trailer_len() == 8 && plain.prefix.size() == 10);
  CHECK(memcmp(plain.prefix.data(), fixed, 10) == 0);
  CHECK(frame_of(kFmtGzip, 2).prefix == plain.prefix && frame_of(kFmtZlib, 1).prefix == frame_zlib(1).prefix);
  CHECK(frame_of(kFmtRaw, 2).prefix.empty() && frame_raw().trailer_len() == 0 && frame_raw().kind == kFmtRaw);
  zt_gzip_opts zero;
  memset(&zero, 0, sizeof zero);
  CHECK(frame_gzip(&zero).prefix == plain.prefix);

  // every combination of name, comment and FHCRC against the reference's order
  const Bytes name = {'f', 'i', 'l', 'e', '.', 't', 'x', 't'}, comment = {'a', ' ', 0xE9, 'b'};
  for (int mask = 0; mask < 8; ++mask) {
    zt_gzip_opts o;
    memset(&o, 0, sizeof o);
    o.fname = mask & 1;
    o.fcomment = (mask >> 1) & 1;
    o.fhcrc = (mask >> 2) & 1;
    o.mtime = 0x12345678u;
    o.name = name.data();
    o.name_len = name.size();
    o.comment = comment.data();
    o.comment_len = comment.size();
    Bytes w = {0x1F, 0x8B, 8};                                                   // signature, method
    w.push_back((o.fname ? 0x08 : 0) | (o.fcomment ? 0x10 : 0) | (o.fhcrc ? 0x02 : 0));  // flags
    w.insert(w.end(), {0x78, 0x56, 0x34, 0x12});                                 // mtime, little endian
    w.push_back(0);                                                              // extra flags
    w.push_back(3);                                                              // UNIX
    if (o.fname) {
      w.insert(w.end(), name.begin(), name.end());
      w.push_back(0);
    }
    if (o.fcomment) {
      w.insert(w.end(), comment.begin(), comment.end());
      w.push_back(0);
    }
    if (o.fhcrc) {
      const uint32_t c16 = crc32_small(w.data(), w.size()) & 0xFFFF;
      w.push_back(c16 & 0xFF);
      w.push_back(c16 >> 8);
    }
    const MemberFrame fr = frame_gzip(&o);
    CHECK(fr.kind == kFmtGzip && fr.prefix == w);
    // read back by the read side's parser, FHCRC compared (the reference
    // takes that CRC from the start of the input: the member is the first)
    const Bytes &in = fr.prefix;
    zt_gzip_member m;
    GzError ge;
    size_t body = 0;
    CHECK(gzip_parse_header(in.data(), in.size(), 0, &m, &body, &ge) == ZT_OK);
    CHECK(body == in.size() && m.mtime == o.mtime && m.os == 3 && m.xfl == 0 && m.flg == w[3]);
    if (o.fname) CHECK(m.name_len == name.size() && memcmp(in.data() + m.name_off, name.data(), name.size()) == 0);
    if (o.fcomment)
      CHECK(m.comment_len == comment.size() && memcmp(in.data() + m.comment_off, comment.data(), comment.size()) == 0);
    CHECK(m.has_crc16 == (uint32_t)o.fhcrc);
  }
  // BGZF: the end marker's 18 header bytes
  const MemberFrame bg = frame_bgzf();
  CHECK(bg.kind == kFmtGzip && bg.prefix.size() == kBgzfHeaderBytes && bg.trailer_len() == kBgzfTrailerBytes);
  CHECK(memcmp(bg.prefix.data(), bgzf_eof_marker(), kBgzfHeaderBytes) == 0);
}

static void check_trailer() {
  const uint32_t crc = 0xAABBCCDDu, adler = 0x11223344u, isize = 0x01020304u;
  for (int kind = kFmtRaw; kind <= kFmtGzip; ++kind) {
    Bytes slow;
    if (kind == kFmtGzip) {
      for (int k = 0; k < 4; ++k) slow.push_back((crc >> (8 * k)) & 0xFF);
      for (int k = 0; k < 4; ++k) slow.push_back((isize >> (8 * k)) & 0xFF);
    }
    if (kind == kFmtZlib) slow = {(uint8_t)(adler >> 24), (uint8_t)(adler >> 16), (uint8_t)(adler >> 8), (uint8_t)adler};
    CHECK(member_trailer_len((MemberKind)kind) == slow.size());
    Bytes t(slow.size());  // exactly the trailer's room (raw: none, and nothing may be written)
    put_trailer(t.data(), (MemberKind)kind, crc, adler, isize);
    CHECK(t == slow);
  }
  // the checksums of nothing, as every empty member carries them
  Bytes z(8, 0x5A), a(4, 0x5A);
  put_trailer(z.data(), kFmtGzip, 0, 1, 0);
  put_trailer(a.data(), kFmtZlib, 0, 1, 0);
  CHECK(z == Bytes(8, 0) && (a == Bytes{0, 0, 0, 1}));
}

static void check_stored() {
  CHECK(stored_header(0, true) == 0xFFFF000001ull && stored_header(65535, false) == 0x0000FFFF00ull);
  for (const uint64_t n : {0ull, 1ull, 65534ull, 65535ull, 65536ull, 131070ull, 131071ull}) {
    Bytes in(n);
    for (uint64_t i = 0; i < n; ++i) in[i] = (uint8_t)(i * 131 + (i >> 9));
    const uint64_t nblk = n ? (n + 65534) / 65535 : 1;
    CHECK(stored_len(n) == n + 5 * nblk && stored_len(0) == 5);
    Bytes out(stored_len(n), 0x5A);
    stored_write(in.data(), n, out.data());
    // block by block: BFINAL on the last only, LEN / NLEN, the bytes
    uint64_t at = 0, p = 0;
    for (uint64_t b = 0; b < nblk; ++b) {
      const uint32_t l = (uint32_t)(n - p < 65535 ? n - p : 65535);
      CHECK(at + 5 + l <= out.size());
      if (at + 5 + l > out.size()) break;
      CHECK(out[at] == (b + 1 == nblk ? 1 : 0));
      CHECK((out[at + 1] | out[at + 2] << 8) == (int)l && (out[at + 3] | out[at + 4] << 8) == (int)(~l & 0xFFFF));
      CHECK(l == 0 || memcmp(out.data() + at + 5, in.data() + p, l) == 0);
      at += 5 + l;
      p += l;
    }
    CHECK(at == out.size() && p == n);
    // the device-resident batch's jobs for the same input, run by the kernels' model
    Bytes dev(stored_len(n), 0xA5);
    DevCopyPlan cp;
    std::vector<DevPatchJob> pj;
    CHECK(dev_stored_jobs(addr(in.data()), n, addr(dev.data()), cp, pj));
    CHECK(pj.size() == nblk && cp.jobs.size() == (n ? nblk : 0));
    model_copy(cp);
    model_patch(pj, nullptr);
    CHECK(dev == out);
  }
}

static void check_header_status() {
  struct Case {
    Bytes in;
    ZlibHdr hs;
    int code;
    std::string msg;
  };
  const Case cases[] = {
      {{}, ZH_METHOD, ZT_E_ZLIB_METHOD, "unsupported compression method"},            // CMF missing
      {{0x77, 0x9C}, ZH_METHOD, ZT_E_ZLIB_METHOD, "unsupported compression method"},  // not deflate
      {{0x78}, ZH_FCHECK_NAN, ZT_E_ZLIB_FCHECK, "invalid fcheck flag:NaN"},           // FLG missing
      {{0x78, 0x9D}, ZH_FCHECK, ZT_E_ZLIB_FCHECK, "invalid fcheck flag:" + std::to_string(0x789D % 31)},
  };
  for (const Case &c : cases) {
    ZlibHeader h;
    const ZlibHdr hs = zlib_parse_header(c.in.data(), c.in.size(), 0, &h);
    int code = 0;
    std::string msg;
    CHECK(hs == c.hs && zlib_header_status(hs, h, &code, &msg) && code == c.code && msg == c.msg);
  }
  CHECK(std::string("invalid fcheck flag:") + std::to_string(0x789D % 31) == "invalid fcheck flag:1");
  // accepted headers and a short DICTID are the callers' to judge: nothing is set
  const Bytes ok = {0x78, 0x9C}, broken = {0x78, 0xBB, 1, 2};
  for (const Bytes &in : {ok, broken}) {
    ZlibHeader h;
    const ZlibHdr hs = zlib_parse_header(in.data(), in.size(), 0, &h);
    int code = 12345;
    std::string msg = "untouched";
    CHECK(hs == (in.size() == 2 ? ZH_OK : ZH_BROKEN) && !zlib_header_status(hs, h, &code, &msg));
    CHECK(code == 12345 && msg == "untouched");
  }
}

int main() {
  check_zlib_header();
  check_gzip_header();
  check_trailer();
  check_stored();
  check_header_status();
  if (fails) {
    fprintf(stderr, "member_frame_host_check: %d failures\n", fails);
    return 1;
  }
  printf("member_frame_host_check ok\n");
  return 0;
}
