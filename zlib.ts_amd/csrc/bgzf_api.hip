// bgzf_api.hip -- BGZF (include/zt_bgzf.h): the entry points and their kernel.
//
// Write: the input is cut into slices of block_size bytes, the slices are the
// items of the batch deflate pipeline (packed at the 32 KiB grid, deflated by
// deflate_batch_dev_run while checksums_batch_dev takes their CRC-32 on the
// second stream), and frame_members_kernel (synth.hip) writes header | CDATA |
// CRC-32 | ISIZE of every block at its dense file offset, BSIZE patched into
// the shared header; the end marker is one more item behind the last block.
// Groups of kBgzfGroupBlocks slices run through the batch layer's stage
// pipeline (StagePipe): group g + 1 is packed and uploaded while group g is
// deflated and framed and group g - 1 comes back, straight into the output.
//
// Read (whole file and ranges share it): the host walk (bgzf_host.h) gives
// the needed blocks with bounds-checked offsets and sizes; only those blocks
// are uploaded; every block is decoded once by the two-phase batch decoder
// with placed outputs (tokenize_kernel, expand_kernel and copy_kernel of
// inflate_tok.hip, unchanged): its input is bounded to its own CDATA, its
// token slot and its place in the decode buffer come from its ISIZE;
// checksums_batch_dev takes the CRC-32 of the decoded bytes on the device;
// bgzf_verify_kernel holds status, length, end position and CRC against the
// trailer and returns the count and the first failing block before any data
// comes back.  (One wave per block with a history ring, inflate_jobs_dev, was
// built and measured first: 70.9 ms for 256 MiB against 25.5 ms of
// zt_gunzip_batch on the same file; it is not kept.)  Range calls gather their
// pieces with range_gather_kernel (range_call.hip) into one packed buffer: one
// download, into the slab the other range calls use (range_call.h).  A failing
// block is decoded again alone by zt_gunzip for the reference's code and
// message.
#include <atomic>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/zt_bgzf.h"
#include "bgzf_host.h"
#include "range_call.h"

namespace zt {

namespace {

// slices per group of the writer's pipeline (64 MiB of padded input); a call's
// device memory is a few groups' worth for any n.
// tuning hook: ZT_BGZF_GROUP_BLOCKS = slices per group
constexpr size_t kBgzfGroupBlocks = 1024;
// blocks per decode of zt_bgzf_decompress (256 MiB of output)
constexpr size_t kBgzfReadGroupBlocks = 4096;
// inputs up to this size are staged with one copy; larger runs are uploaded
// from the caller's buffer (chunked, upload())
constexpr size_t kBgzfStageMax = 32u << 20;

size_t write_group_blocks() {
  static const int v = getenv("ZT_BGZF_GROUP_BLOCKS") ? atoi(getenv("ZT_BGZF_GROUP_BLOCKS")) : 0;
  return v > 0 ? (size_t)v : kBgzfGroupBlocks;
}

// ---- the read side's kernel ------------------------------------------------------
struct BgzfDevBlock {
  uint64_t cdata_end;  // where its CDATA ends in the uploaded input
  uint32_t isize, crc;
  int32_t sum;  // its (crc, adler) pair in the sums, -1: an empty block (CRC 0)
  uint32_t pad;
};
struct BgzfVerdict {
  uint32_t first_fail;  // the first failing block of the decode (0xFFFFFFFF: none)
  uint32_t nfail;
};
struct BgzfVerify {
  const BgzfDevBlock *blk;
  const TokResult *res;
  ChainUnit *cu;               // one chain unit per block, planned on the host
  int32_t *unit_status;        // expand
  int32_t *seg_status;         // copy (one segment per block)
  const uint32_t *sums;
  int32_t *codes;
  BgzfVerdict *verdict;
  uint32_t count;
  // 0, behind the tokenizer: the decode status, out_len == ISIZE and the
  // stream's end == the CDATA's end; a block that holds gets its token count
  // into the chain (bit 31: run tokens; never bit 30: every segment is
  // copied), one that does not becomes an empty unit, so that expand and copy
  // leave it alone.  1, behind copy and the checksums: expand's and copy's
  // statuses and the CRC-32 of the decoded bytes == the trailer's; counts the
  // failures and keeps the first failing block.
  int phase;
};

// One thread per block.  The code says which check failed first (the caller's
// message comes from a second decode of that block alone).
__global__ __launch_bounds__(256) void bgzf_verify_kernel(BgzfVerify P) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= P.count) return;
  const BgzfDevBlock b = P.blk[k];
  int32_t code = ZT_OK;
  if (P.phase == 0) {
    const TokResult r = P.res[k];
    if (r.status != ZT_OK)
      code = r.status == ZT_E_NOMEM ? ZT_E_GZIP_ISIZE : r.status;  // (a full token slot: more output than ISIZE)
    else if (r.out_len != b.isize)
      code = ZT_E_GZIP_ISIZE;
    else if (r.stop_idx >= 0 || ((r.end_bits + 7) >> 3) != b.cdata_end)
      code = ZT_E_BGZF_FORMAT;
    P.codes[k] = code;
    P.unit_status[k] = kNotRun;
    P.seg_status[k] = kNotRun;
    if (code == ZT_OK) {
      P.cu[k].ntok = r.ntok & ~0x40000000u;
    } else {
      P.cu[k].ntok = 0;
      P.cu[k].out_len = 0;
    }
    return;
  }
  code = P.codes[k];
  if (code == ZT_OK) {
    if (P.unit_status[k] != ZT_OK)
      code = P.unit_status[k] < 0 ? P.unit_status[k] : ZT_E_INTERNAL;
    else if (P.seg_status[k] != ZT_OK)
      code = P.seg_status[k] < 0 ? P.seg_status[k] : ZT_E_INTERNAL;
    else if ((b.sum < 0 ? 0u : P.sums[2 * b.sum]) != b.crc)
      code = ZT_E_GZIP_CRC32;
    P.codes[k] = code;
  }
  if (code != ZT_OK) {
    atomicMin(&P.verdict->first_fail, k);
    atomicAdd(&P.verdict->nfail, 1u);
  }
}

struct BgzfCounters {
  std::atomic<uint64_t> range_calls{0}, ranges{0}, blocks_decoded{0}, in_bytes_uploaded{0}, out_bytes_decoded{0},
      out_bytes_returned{0};
};
BgzfCounters g_bz;

int format_error(uint64_t off, const char *why) { return set_error(ZT_E_BGZF_FORMAT, bgzf_format_message(off, why)); }

// ---- one decode: `blocks` (file order, distinct) on the device ---------------------
struct Decoded {
  uint8_t *d_dec = nullptr;
  std::vector<uint64_t> dec_off;  // blocks.size() + 1: 16-byte aligned places in d_dec
  bool dense = false;             // no padding between the blocks: d_dec is their output as it stands
  uint32_t first_fail = 0xFFFFFFFFu, nfail = 0;
  std::vector<int32_t> codes;     // per block, when nfail
  uint64_t in_bytes = 0, out_bytes = 0;
};

// the one upload's layout, then the device-only results
struct ReadTables {
  BgzfDevBlock *blk;
  TokJob *jobs;
  ChainUnit *chain;
  SegJob *segs;
  BgzfVerdict *verdict;
  size_t upload_bytes;
  TokResult *res;
  int32_t *unit_status, *seg_status, *codes;
  size_t bytes;
};
ReadTables read_tables(void *base, size_t nb) {
  Carve cv(base);
  ReadTables t;
  t.blk = cv.take<BgzfDevBlock>(nb);
  t.jobs = cv.take<TokJob>(nb);
  t.chain = cv.take<ChainUnit>(nb);
  t.segs = cv.take<SegJob>(nb);
  t.verdict = cv.take<BgzfVerdict>(1);
  t.upload_bytes = cv.bytes();
  t.res = cv.take<TokResult>(nb);
  t.unit_status = cv.take<int32_t>(nb);
  t.seg_status = cv.take<int32_t>(nb);
  t.codes = cv.take<int32_t>(nb);
  t.bytes = cv.bytes();
  return t;
}

// Everything is planned on the host: a block's ISIZE is known, so its token
// slot, its place in the decode buffer, its chain unit and its one-unit
// segment are laid out before anything runs.  One upload; then, without the
// host waiting in between, tokenize_kernel (inflate_tok.hip, unchanged: one
// wave per block, no history ring), bgzf_verify_kernel phase 0, expand_kernel
// + copy_kernel (unchanged), the checksums, bgzf_verify_kernel phase 1.
int decode_blocks_dev(DeviceCtx *c, const uint8_t *in, const BgzfNeed *blocks, size_t nb, Decoded *D) {
  hipStream_t s = c->stream;
  if (nb > 0x7FFFFFFFull) return set_error(ZT_E_ARG, "too many blocks for one call");
  // upload runs: blocks adjacent in the file go up with one copy
  struct Run {
    uint64_t file, len, dev;
  };
  std::vector<Run> runs;
  std::vector<uint64_t> in_dev(nb);
  uint64_t in_total = 0;
  for (size_t k = 0; k < nb; ++k) {
    const BgzfBlock &b = blocks[k].b;
    if (runs.empty() || runs.back().file + runs.back().len != b.off) {
      in_total = align_up(in_total, 16);
      runs.push_back(Run{b.off, 0, in_total});
    }
    in_dev[k] = runs.back().dev + (b.off - runs.back().file);
    runs.back().len += b.size;
    in_total = runs.back().dev + runs.back().len;
    D->in_bytes += b.size;
  }
  D->dec_off.assign(nb + 1, 0);
  D->dense = true;
  uint64_t dec_total = 0, dense_total = 0, tok_total = 0, desc_total = 0;
  size_t ndata = 0;
  void *d_tab;
  ZT_TRY(scratch(c, kRangeIn, read_tables(nullptr, nb).bytes, &d_tab));
  const ReadTables T = read_tables(d_tab, nb);
  std::vector<uint8_t> tab(T.upload_bytes, 0);
  const ReadTables H = read_tables(tab.data(), nb);
  std::vector<uint64_t> co, cl;
  for (size_t k = 0; k < nb; ++k) {
    const BgzfBlock &b = blocks[k].b;
    dec_total = align_up(dec_total, 16);  // (checksums_batch_dev reads from 16-byte aligned offsets)
    D->dec_off[k] = dec_total;
    if (b.isize && dec_total != dense_total) D->dense = false;
    desc_total = align_up(desc_total, 512);
    const uint64_t cdata = in_dev[k] + b.cdata_off;
    H.blk[k] = BgzfDevBlock{cdata + b.cdata_len, b.isize, b.crc, b.isize ? (int32_t)co.size() : -1, 0};
    // tokens <= output bytes (a stored payload is admitted against the slot
    // before it becomes run tokens: the slot has room for ISIZE literals)
    const uint32_t cap = b.isize + 64;
    H.jobs[k] = TokJob{cdata, tok_total, cap, 0, cdata + b.cdata_len};
    H.chain[k] = ChainUnit{tok_total, dec_total, dec_total, desc_total, 0, b.isize};
    H.segs[k] = SegJob{(uint32_t)k, 1};
    if (b.isize) {
      co.push_back(dec_total);
      cl.push_back(b.isize);
      ++ndata;
    }
    tok_total += align_up(cap, 64);
    desc_total += b.isize;
    dec_total += b.isize;
    dense_total += b.isize;
  }
  D->dec_off[nb] = dec_total;
  D->out_bytes = dense_total;
  *H.verdict = BgzfVerdict{0xFFFFFFFFu, 0};
  void *d_in, *d_dec, *d_tok, *d_desc, *d_sums = nullptr;
  ZT_TRY(scratch(c, kIn, in_total + 256, &d_in));  // + slack: the reader's aligned loads
  ZT_TRY(scratch(c, kOut, dec_total + 256, &d_dec));  // + slack: the gather's aligned loads
  ZT_TRY(scratch(c, kTokens, (tok_total + 256) * 4, &d_tok));  // + slack: chunked token reads
  ZT_TRY(scratch(c, kDeflateOrDesc, (desc_total + 1024) * 2, &d_desc));  // + slack: chunked descriptor reads
  if (ndata) ZT_TRY(scratch(c, kSums, 8 * ndata, &d_sums));
  D->d_dec = static_cast<uint8_t *>(d_dec);
  if (in_total <= kBgzfStageMax) {
    void *h;
    ZT_TRY(pinned(c, in_total, &h, kPinBatch));
    for (const Run &r : runs) copy_to_staging(static_cast<uint8_t *>(h) + r.dev, in + r.file, r.len);
    ZT_HIP(hipMemcpyAsync(d_in, h, in_total, hipMemcpyHostToDevice, s));
  } else {
    for (const Run &r : runs) ZT_TRY(upload(c, static_cast<uint8_t *>(d_in) + r.dev, in + r.file, r.len, s));
  }
  ZT_HIP(hipMemcpyAsync(d_tab, tab.data(), T.upload_bytes, hipMemcpyHostToDevice, s));
  // (stops: never read, nstops = 0)
  ZT_TRY(tokenize_units_dev(tok_params_planned(static_cast<const uint8_t *>(d_in), in_total,
                                               reinterpret_cast<const uint64_t *>(T.jobs), 0, T.jobs, T.res,
                                               static_cast<uint32_t *>(d_tok), (uint32_t)nb),
                            s));
  BgzfVerify bv;
  bv.blk = T.blk;
  bv.res = T.res;
  bv.cu = T.chain;
  bv.unit_status = T.unit_status;
  bv.seg_status = T.seg_status;
  bv.sums = static_cast<const uint32_t *>(d_sums);
  bv.codes = T.codes;
  bv.verdict = T.verdict;
  bv.count = (uint32_t)nb;
  bv.phase = 0;
  const uint32_t grid = (uint32_t)((nb + 255) / 256);
  bgzf_verify_kernel<<<grid, 256, 0, s>>>(bv);
  ZT_HIP(hipGetLastError());
  ResolveParams rp;
  rp.tokens = static_cast<const uint32_t *>(d_tok);
  rp.units = T.chain;
  rp.segs = T.segs;
  rp.out = D->d_dec;
  rp.desc = static_cast<uint16_t *>(d_desc);
  rp.unit_status = T.unit_status;
  rp.seg_status = T.seg_status;
  rp.nunits = (uint32_t)nb;
  rp.nseg = (uint32_t)nb;
  rp.marker = 0;
  rp.in = static_cast<const uint8_t *>(d_in);
  ZT_TRY(resolve_segments_dev(rp, s));
  if (ndata)
    ZT_TRY(checksums_batch_dev(c, D->d_dec, ndata, co.data(), cl.data(), static_cast<uint32_t *>(d_sums), s));
  bv.phase = 1;
  bgzf_verify_kernel<<<grid, 256, 0, s>>>(bv);
  ZT_HIP(hipGetLastError());
  BgzfVerdict v;
  ZT_TRY(readback(c, &v, T.verdict, sizeof v, s));
  D->first_fail = v.first_fail;
  D->nfail = v.nfail;
  if (v.nfail) {
    D->codes.resize(nb);
    ZT_TRY(readback(c, D->codes.data(), T.codes, nb * sizeof(int32_t), s));
  }
  return ZT_OK;
}

// `jobs` (tile0 ascending, `tiles` in all) gathered from the decode buffer into
// one packed buffer of `total` bytes (range_gather_kernel), then its one
// download to h_dst.  Every job ends inside `total`.
int gather_download(DeviceCtx *c, const std::vector<RangeJob> &jobs, uint64_t tiles, const uint8_t *d_dec,
                    uint64_t total, uint8_t *h_dst) {
  hipStream_t s = c->stream;
  if (tiles > 0x7FFFFFFFull) return set_error(ZT_E_ARG, "too many ranges for one call");
  uint8_t *d_bytes = nullptr;
  RangeJob *d_jobs = nullptr;
  ChainInfo *d_info = nullptr;
  ZT_TRY(scratch_carved(c, kRangeOut, [&](void *base) {
    Carve cv(base);
    d_bytes = cv.take<uint8_t>(total);
    d_jobs = cv.take<RangeJob>(jobs.size());
    d_info = cv.take<ChainInfo>(1);
    return cv.bytes();
  }));
  const ChainInfo info{1, 0, 0, 0, 0};  // (the gather's switch: blocks fail one by one here, the gather always runs)
  if (!jobs.empty())
    ZT_HIP(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(RangeJob), hipMemcpyHostToDevice, s));
  ZT_HIP(hipMemcpyAsync(d_info, &info, sizeof info, hipMemcpyHostToDevice, s));
  ZT_TRY(range_gather_dev(d_jobs, (uint32_t)jobs.size(), (uint32_t)tiles, d_dec, d_bytes, d_info, s));
  return download(c, h_dst, d_bytes, total, s);
}

// the failure path: the block alone through the single-member path, for the
// reference's code and message
int rerun_block(const uint8_t *in, const BgzfBlock &b) {
  uint8_t *o = nullptr;
  size_t ol = 0;
  const int rc = zt_gunzip(in + b.off, b.size, &o, &ol, nullptr, nullptr);
  if (rc != ZT_OK) return rc;
  zt_free(o);
  return format_error(b.off, "CDATA does not end with its DEFLATE stream");
}

// ---- range and chunk reads ------------------------------------------------------------
// One requested range after the host lookup.
struct ReadReq {
  int status = ZT_OK;
  std::string msg;  // of a status set on the host
  uint64_t len = 0;
  uint64_t dst = 0;  // 256-aligned place in the packed output
  std::vector<BgzfPiece> pieces;
};

int read_requests(const uint8_t *in, std::vector<ReadReq> &req, std::vector<BgzfNeed> need, uint8_t **out,
                  size_t *out_len, int *status) {
  const size_t count = req.size();
  g_bz.ranges += count;
  const std::vector<BgzfNeed> uniq = bgzf_dedup(std::move(need));
  const size_t nb = uniq.size();
  uint64_t dst_total = 0;
  for (ReadReq &r : req) {
    r.dst = dst_total;
    if (r.status == ZT_OK) dst_total += align_up(r.len ? r.len : 1, 256);  // (>= 1 byte: every pointer distinct)
  }
  const RangeSlab slab{slab_out(dst_total, count, true), count, out, out_len};
  if (!slab.base) return set_error(ZT_E_NOMEM, "host allocation failed");
  std::map<size_t, std::pair<int, std::string>> failed;  // block slot -> its own code and message
  if (nb) {  // (nothing to decode: no GPU touched)
    DeviceCtx *c;
    if (const int rc = get_ctx(&c)) return slab.give_up(rc);
    std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
    Decoded D;
    if (const int rc = decode_blocks_dev(c, in, uniq.data(), nb, &D)) return slab.give_up(rc);
    std::vector<RangeJob> jobs;
    uint64_t tiles = 0;
    for (const ReadReq &r : req) {
      if (r.status != ZT_OK) continue;
      for (const BgzfPiece &p : r.pieces) {
        const size_t slot = bgzf_slot_of(uniq, p.boff);
        range_job_add(jobs, &tiles, D.dec_off[slot] + p.lo, r.dst + p.dst, p.len);
      }
    }
    if (const int rc = gather_download(c, jobs, tiles, D.d_dec, dst_total, slab.base)) return slab.give_up(rc);
    g_bz.range_calls++;
    g_bz.blocks_decoded += nb;
    g_bz.in_bytes_uploaded += D.in_bytes;
    g_bz.out_bytes_decoded += D.out_bytes;
    if (D.nfail) {
      // a range fails with the first failing block it touches, in file order
      for (ReadReq &r : req) {
        if (r.status != ZT_OK) continue;
        for (const BgzfPiece &p : r.pieces) {
          const size_t slot = bgzf_slot_of(uniq, p.boff);
          if (D.codes[slot] == ZT_OK) continue;
          auto it = failed.find(slot);
          if (it == failed.end()) {
            const int rc = rerun_block(in, uniq[slot].b);
            it = failed.emplace(slot, std::make_pair(rc, std::string(zt_last_error_message()))).first;
          }
          r.status = it->second.first;
          r.msg = it->second.second;
          break;
        }
      }
    }
  }
  for (size_t i = 0; i < count; ++i) status[i] = req[i].status;
  return slab.hand_out(
      status, [&](size_t i) { return req[i].dst; }, [&](size_t i) { return req[i].len; }, g_bz.out_bytes_returned,
      [&](size_t i) { return set_error(req[i].status, req[i].msg); });
}

// ---- the write side ---------------------------------------------------------------------
struct WritePlan {
  const uint8_t *in;
  size_t n;
  uint32_t bs;      // slice bytes
  uint64_t cell;    // a slice's room at the 32 KiB grid
  size_t nblk, G, ng;
  int ct, lv;
  uint64_t block_bound;  // the largest block a slice can give (<= 65536)
  size_t blocks_of(size_t g) const { return std::min(G, nblk - g * G); }
  uint32_t slice_len(size_t k) const { return (uint32_t)std::min<uint64_t>(bs, n - (uint64_t)k * bs); }
};

// compression type NONE (or level 0): stored blocks, written on the host as the
// batch calls do; the CRCs alone come from the device
int write_stored(const WritePlan &W, uint8_t *out, uint64_t *total, std::vector<GziPair> *pairs) {
  const MemberFrame fr = frame_bgzf();
  uint64_t at = 0;
  for (size_t g = 0; g < W.ng; ++g) {
    const size_t k0 = g * W.G, nb = W.blocks_of(g);
    std::vector<const uint8_t *> ptr(nb);
    std::vector<size_t> len(nb);
    std::vector<uint32_t> crc(nb);
    for (size_t j = 0; j < nb; ++j) {
      ptr[j] = W.in + (uint64_t)(k0 + j) * W.bs;
      len[j] = W.slice_len(k0 + j);
    }
    ZT_TRY(zt_crc32_batch(ptr.data(), len.data(), nb, crc.data()));
    for (size_t j = 0; j < nb; ++j) {
      const uint32_t l = (uint32_t)len[j], size = kBgzfHeaderBytes + 5 + l + kBgzfTrailerBytes;
      if (k0 + j) pairs->push_back(GziPair{at, (uint64_t)(k0 + j) * W.bs});
      uint8_t *o = out + at;
      memcpy(o, fr.prefix.data(), kBgzfHeaderBytes);
      o[16] = (uint8_t)((size - 1) & 0xFF);
      o[17] = (uint8_t)((size - 1) >> 8);
      stored_write(ptr[j], l, o + kBgzfHeaderBytes);
      put_trailer(o + kBgzfHeaderBytes + 5 + l, fr.kind, crc[j], 1, l);
      at += size;
    }
  }
  memcpy(out + at, bgzf_eof_marker(), kBgzfEofBytes);
  *total = at + kBgzfEofBytes;
  return ZT_OK;
}

int write_pipeline(DeviceCtx *c, const WritePlan &W, uint8_t *out, uint64_t *total, std::vector<GziPair> *pairs) {
  const size_t G = W.G, ng = W.ng;
  const uint64_t gpad = G * W.cell;
  // device: two input groups, one deflate output and scratch, two framed groups
  const uint64_t fr_cap = align_up(G * W.block_bound + kBgzfEofBytes, 256);
  const size_t ss = deflate_batch_scratch_bytes(c, gpad);
  void *p;
  uint8_t *d_in[2], *d_framed[2], *stage_in[2], *stage_out;
  FrameItem *d_items[2];
  uint8_t *d_prefix;
  void *d_body, *d_scr, *d_sums;
  ZT_TRY(scratch(c, kIn, 2 * (gpad + 256), &p));
  d_in[0] = static_cast<uint8_t *>(p);
  d_in[1] = d_in[0] + gpad + 256;
  ZT_TRY(scratch(c, kOut, batch_out_bound(gpad, 256), &d_body));
  ZT_TRY(scratch(c, kDeflateOrDesc, ss, &d_scr));
  ZT_TRY(scratch(c, kSums, 8 * (G + 1), &d_sums));
  ZT_TRY(scratch_carved(c, kFramed, [&](void *base) {
    Carve cv(base);
    for (int k = 0; k < 2; ++k) {
      d_framed[k] = cv.take<uint8_t>(fr_cap);
      d_items[k] = cv.take<FrameItem>(G + 1);
    }
    d_prefix = cv.take<uint8_t>(kBgzfHeaderBytes);
    return cv.bytes();
  }));
  ZT_TRY(pinned(c, gpad, &p, kPinBatch));
  stage_in[0] = static_cast<uint8_t *>(p);
  ZT_TRY(pinned(c, gpad, &p, kPinGroupIn));
  stage_in[1] = static_cast<uint8_t *>(p);
  ZT_TRY(pinned(c, fr_cap, &p, kPinGroupOut));
  stage_out = static_cast<uint8_t *>(p);
  const MemberFrame fr = frame_bgzf();
  ZT_HIP(hipMemcpyAsync(d_prefix, fr.prefix.data(), kBgzfHeaderBytes, hipMemcpyHostToDevice, c->stream));
  ZT_HIP(hipStreamSynchronize(c->stream));

  std::vector<uint64_t> goff(ng + 1, 0);  // group g's bytes in the file
  std::vector<FrameItem> fi(G + 1);
  std::vector<uint64_t> oo(G + 1), ro(G), rl(G);
  StagePipe pipe(c, ng);
  auto stopped = [] { return set_error(ZT_E_INTERNAL, "pipeline stopped"); };
  auto up_stage = [&](size_t g) -> int {
    // group g - 2 has left the device: its input, its staging and its framed
    // buffer are free
    if (g >= 2 && !pipe.wait_downloaded(g - 2)) return stopped();
    const size_t k0 = g * G, nb = W.blocks_of(g);
    uint8_t *st = stage_in[g & 1];
    parallel_copy(nb, [&](size_t j) {
      const uint32_t l = W.slice_len(k0 + j);
      copy_to_staging(st + j * W.cell, W.in + (uint64_t)(k0 + j) * W.bs, l);
      memset(st + j * W.cell + l, 0, W.cell - l);
    }, nb * W.cell);
    ZT_HIP(hipMemcpyAsync(d_in[g & 1], st, nb * W.cell, hipMemcpyHostToDevice, c->up));
    return ZT_OK;
  };
  auto compute = [&](size_t g) -> int {
    const size_t k0 = g * G, nb = W.blocks_of(g);
    const bool last = g + 1 == ng;
    for (size_t j = 0; j < nb; ++j) {
      ro[j] = j * W.cell;
      rl[j] = W.slice_len(k0 + j);
    }
    ZT_TRY(deflate_members_dev(c, d_in[g & 1], nb, ro.data(), rl.data(), W.ct, W.lv, static_cast<uint8_t *>(d_body),
                               oo.data(), d_scr, ss, nullptr, static_cast<uint32_t *>(d_sums), pipe.landed(g)));
    // the blocks' sizes and dense places
    uint64_t at = 0;
    for (size_t j = 0; j < nb; ++j) {
      const uint64_t body = oo[j + 1] - oo[j], size = kBgzfHeaderBytes + body + kBgzfTrailerBytes;
      if (size > kBgzfBlockBytes || size > W.block_bound)
        return set_error(ZT_E_INTERNAL, "BGZF block of " + std::to_string(size) + " bytes: the slice does not compress");
      fi[j] = FrameItem{oo[j], at, (uint32_t)body, (uint32_t)rl[j]};
      if (k0 + j) pairs->push_back(GziPair{goff[g] + at, (uint64_t)(k0 + j) * W.bs});
      at += size;
    }
    size_t items = nb;
    if (last) {
      // the end marker: one more item, its CDATA the empty fixed block 03 00, CRC 0
      ZT_TRY(q_bytes(static_cast<uint8_t *>(d_body) + oo[nb], 0x0003, 2, c->stream));
      ZT_TRY(q_bytes(static_cast<uint32_t *>(d_sums) + 2 * nb, 0, 8, c->stream));
      fi[nb] = FrameItem{oo[nb], at, 2, 0};
      at += kBgzfEofBytes;
      ++items;
    }
    goff[g + 1] = goff[g] + at;
    ZT_HIP(hipMemcpyAsync(d_items[g & 1], fi.data(), items * sizeof(FrameItem), hipMemcpyHostToDevice, c->stream));
    ZT_TRY(join_sums(c));  // (the trailers need the checksums)
    ZT_TRY(frame_members_dev(d_items[g & 1], (uint32_t)items, d_prefix, kBgzfHeaderBytes, fr.kind,
                             static_cast<const uint8_t *>(d_body), static_cast<const uint32_t *>(d_sums),
                             d_framed[g & 1], c->stream, 16));
    // (the download stage copies on its own stream; fi, d_body and d_sums are the next group's)
    ZT_HIP(hipStreamSynchronize(c->stream));
    ZT_HIP(hipStreamSynchronize(c->aux));
    return ZT_OK;
  };
  auto dn_stage = [&](size_t g) -> int {
    const uint64_t len = goff[g + 1] - goff[g];
    uint8_t *dst = out + goff[g];
    if (host_direct(dst, len)) {
      ZT_HIP(hipMemcpyAsync(dst, d_framed[g & 1], len, hipMemcpyDeviceToHost, c->dn));
      ZT_HIP(hipStreamSynchronize(c->dn));
    } else {
      ZT_HIP(hipMemcpyAsync(stage_out, d_framed[g & 1], len, hipMemcpyDeviceToHost, c->dn));
      ZT_HIP(hipStreamSynchronize(c->dn));
      memcpy(dst, stage_out, len);
    }
    return ZT_OK;
  };
  ZT_TRY(pipe.run(up_stage, compute, dn_stage));
  *total = goff[ng];
  return ZT_OK;
}

uint8_t *blob_out(const std::vector<uint8_t> &v) {
  uint8_t *h = host_out(v.size());
  if (h && !v.empty()) memcpy(h, v.data(), v.size());
  return h;
}

void fill_info(zt_bgzf_info *info, const BgzfWalk &w) {
  if (!info) return;
  info->blocks = w.blocks.size();
  info->data_blocks = w.data_blocks;
  info->total_out = w.uoff.back();
  info->error_offset = w.error_offset;
  info->has_eof = w.has_eof ? 1 : 0;
}

}  // namespace

}  // namespace zt

using namespace zt;

extern "C" {

int zt_bgzf_compress(const uint8_t *in, size_t n, const zt_bgzf_opts *opts, uint8_t **out, size_t *out_len,
                     uint8_t **gzi, size_t *gzi_len) {
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if (n && !in) return set_error(ZT_E_ARG, "null input");
  *out = nullptr;
  *out_len = 0;
  if (gzi) *gzi = nullptr;
  if (gzi_len) *gzi_len = 0;
  WritePlan W;
  ZT_TRY(resolve_opts(opts ? &opts->deflate : nullptr, &W.ct, &W.lv));
  W.bs = opts && opts->block_size ? opts->block_size : kBgzfBlockMax;
  if (W.bs < kBgzfBlockMin || W.bs > kBgzfBlockMax) return set_error(ZT_E_ARG, "block_size must be 0 or 4096..65280");
  W.in = in;
  W.n = n;
  W.cell = align_up(W.bs, 32768);
  W.nblk = (n + W.bs - 1) / W.bs;
  W.G = std::min(write_group_blocks(), std::max<size_t>(W.nblk, 1));
  W.ng = (W.nblk + W.G - 1) / W.G;
  W.block_bound = std::min<uint64_t>(kBgzfBlockBytes, kBgzfHeaderBytes + bgzf_cdata_bound(W.ct, W.bs) + kBgzfTrailerBytes);
  const uint64_t bound = W.nblk * W.block_bound + kBgzfEofBytes;
  uint8_t *h = host_out(bound, true);
  if (!h) return set_error(ZT_E_NOMEM, "host allocation failed");
  uint64_t total = 0;
  std::vector<GziPair> pairs;
  int rc = ZT_OK;
  if (W.nblk == 0) {
    memcpy(h, bgzf_eof_marker(), kBgzfEofBytes);
    total = kBgzfEofBytes;
  } else if (W.ct == 0) {
    rc = write_stored(W, h, &total, &pairs);
  } else {
    DeviceCtx *c;
    rc = get_ctx(&c);
    if (rc == ZT_OK) {
      std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
      rc = write_pipeline(c, W, h, &total, &pairs);
    }
  }
  uint8_t *g = nullptr;
  std::vector<uint8_t> blob;
  if (rc == ZT_OK && gzi) {
    blob = bgzf_gzi_encode(pairs);
    g = blob_out(blob);
    if (!g) rc = set_error(ZT_E_NOMEM, "host allocation failed");
  }
  if (rc != ZT_OK) {
    host_discard(h);
    return rc;
  }
  host_out_used(h, total);
  *out = h;
  *out_len = total;
  if (gzi) *gzi = g;
  if (gzi_len) *gzi_len = 8 + 16 * pairs.size();
  return ZT_OK;
}

int zt_bgzf_index(const uint8_t *in, size_t n, uint8_t **gzi, size_t *gzi_len, zt_bgzf_info *info) {
  if (n && !in) return set_error(ZT_E_ARG, "null input");
  if (gzi) *gzi = nullptr;
  if (gzi_len) *gzi_len = 0;
  const BgzfWalk w = bgzf_walk(in, n);
  fill_info(info, w);
  if (w.why) return format_error(w.error_offset, w.why);
  const std::vector<uint8_t> blob = bgzf_gzi_encode(bgzf_gzi_pairs(w));
  if (gzi) {
    *gzi = blob_out(blob);
    if (!*gzi) return set_error(ZT_E_NOMEM, "host allocation failed");
  }
  if (gzi_len) *gzi_len = blob.size();
  return ZT_OK;
}

int zt_bgzf_decompress(const uint8_t *in, size_t n, uint8_t **out, size_t *out_len, zt_bgzf_info *info) {
  if (!out || !out_len) return set_error(ZT_E_ARG, "null output");
  if (n && !in) return set_error(ZT_E_ARG, "null input");
  *out = nullptr;
  *out_len = 0;
  const BgzfWalk w = bgzf_walk(in, n);
  fill_info(info, w);
  if (w.why) return format_error(w.error_offset, w.why);
  const uint64_t total = w.uoff.back();
  uint8_t *h = host_out(total, true);
  if (!h) return set_error(ZT_E_NOMEM, "host allocation failed");
  const size_t nblk = w.blocks.size();
  if (nblk) {
    DeviceCtx *c;
    int rc = get_ctx(&c);
    if (rc == ZT_OK) {
      std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
      std::vector<BgzfNeed> need;
      for (size_t k0 = 0; k0 < nblk && rc == ZT_OK; k0 += kBgzfReadGroupBlocks) {
        const size_t nb = std::min(kBgzfReadGroupBlocks, nblk - k0);
        need.clear();
        for (size_t k = k0; k < k0 + nb; ++k) need.push_back(BgzfNeed{w.blocks[k], w.uoff[k]});
        Decoded D;
        rc = decode_blocks_dev(c, in, need.data(), nb, &D);
        if (rc != ZT_OK) break;
        if (D.nfail) {  // the first failing block in file order (earlier groups held)
          const BgzfBlock &b = w.blocks[k0 + D.first_fail];
          if (info) info->error_offset = b.off;
          rc = rerun_block(in, b);
          break;
        }
        const uint64_t glen = w.uoff[k0 + nb] - w.uoff[k0];
        if (!glen) continue;
        if (D.dense) {
          rc = download(c, h + w.uoff[k0], D.d_dec, glen, c->stream);
        } else {
          // blocks whose sizes are no multiples of 16 sit apart in the decode
          // buffer: packed by the gather, then one download
          std::vector<RangeJob> jobs;
          uint64_t tiles = 0;
          for (size_t k = 0; k < nb; ++k) {
            if (!need[k].b.isize) continue;
            range_job_add(jobs, &tiles, D.dec_off[k], w.uoff[k0 + k] - w.uoff[k0], need[k].b.isize);
          }
          rc = gather_download(c, jobs, tiles, D.d_dec, glen, h + w.uoff[k0]);
        }
      }
    }
    if (rc != ZT_OK) {
      host_discard(h);
      return rc;
    }
  }
  *out = h;
  *out_len = total;
  return ZT_OK;
}

int zt_bgzf_read_ranges(const uint8_t *in, size_t n, const uint8_t *gzi, size_t gzi_len, const uint64_t *off,
                        const uint64_t *len, size_t count, uint8_t **out, size_t *out_len, int *status) {
  if (count == 0) return ZT_OK;
  if (!off || !len || !out || !out_len || !status) return set_error(ZT_E_ARG, "null argument");
  if (!in && n) return set_error(ZT_E_ARG, "null input");
  for (size_t i = 0; i < count; ++i) out[i] = nullptr, out_len[i] = 0, status[i] = ZT_OK;
  BgzfLookup look;
  std::vector<GziPair> pairs;
  if (gzi) {
    if (const char *why = bgzf_gzi_decode(gzi, gzi_len, n, &pairs))
      return set_error(ZT_E_BGZF_INDEX, std::string("invalid .gzi: ") + why);
  }
  const BgzfLocator loc = gzi ? BgzfLocator(in, n, pairs, &look) : BgzfLocator(in, n, &look);
  auto lookup_error = [](const BgzfLookup &l) {
    if (l.err == kBgzfLookIndex)
      return set_error(ZT_E_BGZF_INDEX, ".gzi does not fit the file at offset " + std::to_string(l.error_offset) + ": " + l.why);
    return format_error(l.error_offset, l.why);
  };
  if (look.err) return lookup_error(look);
  std::vector<ReadReq> req(count);
  std::vector<BgzfNeed> need;
  for (size_t i = 0; i < count; ++i) {
    uint64_t l = len[i];
    if (!bgzf_clamp(loc.total(), off[i], &l)) {
      req[i].status = ZT_E_ARG;
      req[i].msg = "range starts past the end of the output";
      continue;
    }
    req[i].len = l;
    if (!l) continue;
    const BgzfLookup r = loc.locate(off[i], l, &need, &req[i].pieces);
    if (r.err) return lookup_error(r);
  }
  return read_requests(in, req, std::move(need), out, out_len, status);
}

int zt_bgzf_read_virtual(const uint8_t *in, size_t n, const uint64_t *vbeg, const uint64_t *vend, size_t count,
                         uint8_t **out, size_t *out_len, int *status) {
  if (count == 0) return ZT_OK;
  if (!vbeg || !vend || !out || !out_len || !status) return set_error(ZT_E_ARG, "null argument");
  if (!in && n) return set_error(ZT_E_ARG, "null input");
  std::vector<ReadReq> req(count);
  std::vector<BgzfNeed> need;
  for (size_t i = 0; i < count; ++i) {
    out[i] = nullptr, out_len[i] = 0, status[i] = ZT_OK;
    std::vector<BgzfNeed> mine;
    const BgzfChunk ch = bgzf_locate_virtual(in, n, vbeg[i], vend[i], &mine, &req[i].pieces);
    if (ch.look.err) {
      req[i].status = ZT_E_BGZF_FORMAT;
      req[i].msg = bgzf_format_message(ch.look.error_offset, ch.look.why);
    } else if (ch.arg) {
      req[i].status = ZT_E_ARG;
      req[i].msg = vend[i] < vbeg[i] ? "chunk ends before it begins" : "uoffset past the end of its block";
    } else {
      req[i].len = ch.len;
      need.insert(need.end(), mine.begin(), mine.end());
      continue;
    }
    req[i].pieces.clear();
  }
  return read_requests(in, req, std::move(need), out, out_len, status);
}

int zt_bgzf_stats_read(zt_bgzf_stats *out, int reset) {
  if (!out) return set_error(ZT_E_ARG, "null output");
  out->range_calls = stat_take(g_bz.range_calls, reset);
  out->ranges = stat_take(g_bz.ranges, reset);
  out->blocks_decoded = stat_take(g_bz.blocks_decoded, reset);
  out->in_bytes_uploaded = stat_take(g_bz.in_bytes_uploaded, reset);
  out->out_bytes_decoded = stat_take(g_bz.out_bytes_decoded, reset);
  out->out_bytes_returned = stat_take(g_bz.out_bytes_returned, reset);
  return ZT_OK;
}

}  // extern "C"
