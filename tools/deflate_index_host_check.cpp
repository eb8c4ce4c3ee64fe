// tools/deflate_index_host_check.cpp -- drives the host-only arithmetic of the
// deflate-time index (zlib.ts_amd/csrc/deflate_index_host.h) without a device:
// the entry count of a deflate call, the unit an entry stands for, the entry
// offsets of a pieced stream and the header fill, each against a plain serial
// restatement -- walk the blocks, ask restart_after -- and the finished blob
// through index_validate.  Meant to be built with a sanitizer and run on its
// own (tests/test_deflate_index_host.py):
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o deflate_index_host_check tools/deflate_index_host_check.cpp
//   ./deflate_index_host_check
//
// Every blob is a heap allocation of exactly its bytes.  Prints
// "deflate_index_host_check ok"; exit 1 on a broken invariant.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../zlib.ts_amd/csrc/deflate_index_host.h"

using namespace zt;

static int fails = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      if (fails < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
      ++fails;                                                   \
    }                                                            \
  } while (0)

constexpr uint64_t kBlock = ZT_DF_BLOCK;
constexpr uint64_t kSeg = 1u << 20;

// the serial restatement: the units of one call, block by block
static std::vector<DixUnit> serial_units(uint32_t nblocks, uint32_t restart, bool final_) {
  std::vector<DixUnit> u;
  for (uint32_t b = 0; b < nblocks; ++b) {
    u.push_back(DixUnit{b, 0});
    if (restart_after(b, nblocks, restart, final_ ? 1 : 0, nullptr)) {
      u.push_back(DixUnit{b, 1});
      u.push_back(DixUnit{b, 2});
    }
  }
  return u;
}

static void check_call(uint32_t nblocks, uint32_t restart, bool final_) {
  const std::vector<DixUnit> want = serial_units(nblocks, restart, final_);
  CHECK(dix_call_units(nblocks, restart, final_) == want.size());
  for (uint32_t e = 0; e < want.size(); ++e) {
    const DixUnit got = dix_unit_at(e, nblocks, restart);
    CHECK(got.block == want[e].block && got.kind == want[e].kind);
  }
}

// A synthetic stream written as pieces of `sizes` input bytes at stream_start:
// every block 100 + (block % 7) stream bytes, a marker 10.  The entries are
// written the way the kernel writes them -- per piece, from the piece's entry
// offset, the stream bytes so far as the base -- and compared with one serial
// walk over the whole input.
static void check_stream(const std::vector<size_t> &sizes, uint64_t stream_start) {
  const uint32_t restart = (uint32_t)(kSeg / kBlock);
  const size_t np = sizes.size();
  uint64_t n = 0;
  for (size_t s : sizes) n += s;
  const DixLayout L = dix_layout(sizes, restart);
  CHECK(L.first.size() == np + 1 && L.first[0] == 0 && L.nunits == L.first[np]);

  // serial: the whole input as one final call (pieces are whole segments, so
  // a non-final piece's closing marker is the marker of that segment boundary)
  const uint32_t nb_all = (uint32_t)((n + kBlock - 1) / kBlock);
  std::vector<IdxEntry> want;
  {
    uint64_t in = stream_start;
    bool after_marker = true;  // (unit 0)
    for (uint32_t b = 0; b < nb_all; ++b) {
      want.push_back(IdxEntry{in, (uint64_t)b * kBlock, 50 + b % 7, after_marker ? 1u : 0u});
      after_marker = false;
      in += 100 + b % 7;
      if (restart_after(b, nb_all, restart, 1, nullptr)) {
        const uint64_t nx = std::min<uint64_t>((uint64_t)(b + 1) * kBlock, n);
        want.push_back(IdxEntry{in, nx, 0, 0});
        want.push_back(IdxEntry{in + 5, nx, 0, 0});
        in += 10;
        after_marker = true;
      }
    }
    want.push_back(IdxEntry{in, n, 0, 0});
  }
  CHECK(L.nunits + 1 == want.size());
  if (L.nunits + 1 != want.size()) return;

  // per piece, as the device does
  uint8_t *blob = (uint8_t *)malloc(index_blob_bytes((size_t)L.nunits));
  uint64_t written = 0, in_pos = 0, block0 = 0;
  for (size_t i = 0; i < np; ++i) {
    const bool final_ = i + 1 == np;
    const uint32_t nb = (uint32_t)((sizes[i] + kBlock - 1) / kBlock);
    const uint64_t nent = dix_call_units(nb, restart, final_);
    CHECK(L.first[i + 1] - L.first[i] == nent);
    // the piece's block offsets (scan_sizes)
    std::vector<uint64_t> boff(nb + 1, 0);
    for (uint32_t b = 0; b < nb; ++b)
      boff[b + 1] = boff[b] + 100 + (block0 + b) % 7 + (restart_after(b, nb, restart, final_ ? 1 : 0, nullptr) ? 10 : 0);
    for (uint32_t e = 0; e < nent; ++e) {
      const DixUnit u = dix_unit_at(e, nb, restart);
      CHECK(u.block < nb);
      if (u.block >= nb) continue;
      IdxEntry x;
      if (u.kind == 0) {
        x = IdxEntry{stream_start + written + boff[u.block], in_pos + (uint64_t)u.block * kBlock,
                     50 + (uint32_t)((block0 + u.block) % 7), e == 0 ? 1u : 0u};
        if (e && dix_unit_at(e - 1, nb, restart).kind == 2) x.flags = 1;
      } else {
        const uint64_t nx = std::min<uint64_t>((uint64_t)(u.block + 1) * kBlock, sizes[i]);
        x = IdxEntry{stream_start + written + boff[u.block + 1] - (u.kind == 1 ? 10 : 5), in_pos + nx, 0, 0};
      }
      index_write_entry(blob, (size_t)(L.first[i] + e), x);
    }
    written += boff[nb];
    in_pos += sizes[i];
    block0 += nb;
    if (final_) index_write_entry(blob, (size_t)L.nunits, IdxEntry{stream_start + written, in_pos, 0, 0});
  }
  for (size_t k = 0; k < want.size(); ++k) {
    const uint8_t *p = blob + kIdxHeader + k * kIdxEntry;
    CHECK(idx_get64(p) == want[k].in_off && idx_get64(p + 8) == want[k].out_off);
    CHECK(idx_get32(p + 16) == want[k].ntok && idx_get32(p + 20) == want[k].flags);
  }
  const char *why = dix_finish(blob, (size_t)L.nunits, stream_start, written, n);
  if (why) fprintf(stderr, "dix_finish: %s\n", why);
  CHECK(why == nullptr);
  IndexView v;
  CHECK(index_validate(blob, index_blob_bytes((size_t)L.nunits), (size_t)(stream_start + written), &v) == nullptr);
  CHECK(v.nunits == L.nunits && v.stream_start == stream_start && v.end_ip == stream_start + written);
  CHECK(v.total_out == n);
  uint32_t nseg = 0;
  for (const IdxEntry &e : want) nseg += e.flags & 1;
  CHECK(v.nseg == nseg && nseg == (n + kSeg - 1) / kSeg);
  // one byte short of the stream: refused
  CHECK(index_validate(blob, index_blob_bytes((size_t)L.nunits), (size_t)(stream_start + written - 1), &v) != nullptr);
  free(blob);
}

int main() {
  for (uint32_t restart : {1u, 2u, 4u, 32u})
    for (uint32_t nb = 1; nb <= 200; ++nb) {
      check_call(nb, restart, true);
      check_call(nb, restart, false);
    }
  check_call(8192, 32, true);
  CHECK(dix_call_units(8192, 32, true) + 1 == 8192 + 2 * 255 + 1);  // 256 MiB: 8702 units, and the sentinel
  CHECK(dix_call_units(8192, 32, true) == 8702);

  CHECK(dix_stored_tokens(0) == 0 && dix_stored_tokens(1023) == 1023 && dix_stored_tokens(1024) == 3);
  CHECK(dix_stored_tokens(32768) == 3);

  for (uint64_t start : {(uint64_t)0, (uint64_t)37, (uint64_t)1 << 33}) {
    check_stream({1}, start);
    check_stream({5}, start);
    check_stream({kBlock}, start);
    check_stream({kBlock + 1}, start);
    check_stream({kSeg}, start);          // ends exactly on a segment boundary: no marker
    check_stream({kSeg + 1}, start);
    check_stream({3 * kSeg}, start);
    check_stream({32 * kSeg, 32 * kSeg, 1}, start);   // a one-byte last piece
    check_stream({32 * kSeg, 32 * kSeg}, start);      // the last piece ends on a segment boundary
    check_stream({kSeg, 2 * kSeg, 4 * kSeg, kSeg + 777}, start);
    check_stream({2 * kSeg, 1}, start);
  }
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  puts("deflate_index_host_check ok");
  return 0;
}
