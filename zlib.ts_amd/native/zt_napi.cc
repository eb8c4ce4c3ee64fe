// zt_napi.cc -- N-API addon: the thin binding between the JS facade
// (zlib.ts_amd/lib/*.js, the reference's RawDeflate / RawInflate / CRC32 /
// Adler32 surface) and libzt.so's C-ABI (include/zt.h).  Uint8Array memory is
// passed zero-copy; results come back as Uint8Arrays over the library's own
// output buffers (no copy, released by zt_free on collection).  Every call runs on
// the GPU; errors carry libzt's status code and message (the JS facade maps
// them onto the reference's thrown values).
#include <node_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/zt.h"
#include "../../include/zt_zipcrypto.h"
#include "../../include/zt_dict.h"
#include "../../include/zt_container_batch.h"
#include "../../include/zt_index.h"
#include "../../include/zt_checkpoint.h"
#include "../../include/zt_bgzf.h"
#include "../../include/zt_stream.h"
#include "../../include/zt_stream_container.h"
#include "../../include/zt_strategy.h"

namespace {

napi_value throw_zt(napi_env env, int code) {
  const char *msg = zt_last_error_message();
  char codebuf[16];
  snprintf(codebuf, sizeof codebuf, "%d", code);
  napi_value err, m, c;
  napi_create_string_utf8(env, msg ? msg : "libzt error", NAPI_AUTO_LENGTH, &m);
  napi_create_string_utf8(env, codebuf, NAPI_AUTO_LENGTH, &c);
  napi_create_error(env, c, m, &err);
  napi_value num;
  napi_create_int32(env, code, &num);
  napi_set_named_property(env, err, "ztStatus", num);
  napi_throw(env, err);
  return nullptr;
}

bool get_u8(napi_env env, napi_value v, const uint8_t **p, size_t *n) {
  bool is_ta = false;
  napi_is_typedarray(env, v, &is_ta);
  if (!is_ta) {
    napi_throw_type_error(env, nullptr, "expected a Uint8Array");
    return false;
  }
  napi_typedarray_type t;
  size_t len = 0, off = 0;
  void *data = nullptr;
  napi_value ab;
  napi_get_typedarray_info(env, v, &t, &len, &data, &ab, &off);
  if (t != napi_uint8_array) {
    napi_throw_type_error(env, nullptr, "expected a Uint8Array");
    return false;
  }
  *p = static_cast<const uint8_t *>(data);
  *n = len;
  return true;
}

int64_t get_i64(napi_env env, napi_value v, int64_t dflt) {
  napi_valuetype t;
  napi_typeof(env, v, &t);
  if (t != napi_number) return dflt;
  int64_t x = dflt;
  napi_get_value_int64(env, v, &x);
  return x;
}

uint32_t get_u32(napi_env env, napi_value v, uint32_t dflt) {
  napi_valuetype t;
  napi_typeof(env, v, &t);
  if (t != napi_number) return dflt;
  uint32_t x = dflt;
  napi_get_value_uint32(env, v, &x);
  return x;
}

// A libzt-allocated result handed to JS without a copy: an external
// ArrayBuffer over the library's buffer, released by zt_free when the GC
// collects it (large outputs then go back to libzt's host output pool,
// registered for DMA, and the next call of a similar size reuses them).  The
// bytes are reported to V8 as external memory so that a loop of large calls
// triggers collections.
void release_result(napi_env env, void *data, void *hint) {
  zt_free(data);
  int64_t adj = 0;
  napi_adjust_external_memory(env, -(int64_t)(uintptr_t)hint, &adj);
}

napi_value new_u8(napi_env env, uint8_t *buf, size_t n) {
  napi_value ab, ta;
  if (n == 0 || !buf) {
    void *data = nullptr;
    napi_create_arraybuffer(env, 0, &data, &ab);
    zt_free(buf);
  } else if (napi_create_external_arraybuffer(env, buf, n, release_result, (void *)(uintptr_t)n, &ab) == napi_ok) {
    int64_t adj = 0;
    napi_adjust_external_memory(env, (int64_t)n, &adj);
  } else {  // (a runtime without external buffers: copy)
    void *data = nullptr;
    napi_create_arraybuffer(env, n, &data, &ab);
    memcpy(data, buf, n);
    zt_free(buf);
  }
  napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &ta);
  return ta;
}

napi_value args(napi_env env, napi_callback_info info, napi_value *argv, size_t want) {
  size_t argc = want;
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  napi_value undef;
  napi_get_undefined(env, &undef);
  for (size_t i = argc; i < want; ++i) argv[i] = undef;
  return undef;
}

// optional trailing `dictionary` argument (include/zt_dict.h): undefined /
// null = none (*given stays false)
bool get_dict(napi_env env, napi_value v, const uint8_t **p, size_t *n, bool *given) {
  napi_valuetype t;
  napi_typeof(env, v, &t);
  *given = false;
  *p = nullptr;
  *n = 0;
  if (t == napi_undefined || t == napi_null) return true;
  if (!get_u8(env, v, p, n)) return false;
  *given = true;
  return true;
}

// optional trailing `strategy` argument (include/zt_strategy.h): undefined /
// null = none, the plain entry point
bool get_strategy(napi_env env, napi_value v, int *strategy) {
  napi_valuetype t;
  napi_typeof(env, v, &t);
  *strategy = 0;
  if (t == napi_undefined || t == napi_null) return false;
  *strategy = (int)get_i64(env, v, 0);
  return true;
}

// crc32Update(data: Uint8Array, crc: number) -> number
napi_value crc32_update(napi_env env, napi_callback_info info) {
  napi_value a[2];
  args(env, info, a, 2);
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  uint32_t out = 0;
  int rc = zt_crc32_update(get_u32(env, a[1], 0), p, n, &out);
  if (rc) return throw_zt(env, rc);
  napi_value r;
  napi_create_uint32(env, out, &r);
  return r;
}

// adler32Update(adler: number, data: Uint8Array) -> number
napi_value adler32_update(napi_env env, napi_callback_info info) {
  napi_value a[2];
  args(env, info, a, 2);
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[1], &p, &n)) return nullptr;
  uint32_t out = 0;
  int rc = zt_adler32_update(get_u32(env, a[0], 1), p, n, &out);
  if (rc) return throw_zt(env, rc);
  napi_value r;
  napi_create_uint32(env, out, &r);
  return r;
}

// deflateRaw(input: Uint8Array, compressionType, lazy, level[, dictionary[, strategy]]) -> Uint8Array
// (a strategy goes without a dictionary: the facade refuses the pair)
napi_value deflate_raw(napi_env env, napi_callback_info info) {
  napi_value a[6];
  args(env, info, a, 6);
  int strategy;
  const bool has_s = get_strategy(env, a[5], &strategy);
  const uint8_t *d;
  size_t dn;
  bool has_d;
  if (!get_dict(env, a[4], &d, &dn, &has_d)) return nullptr;
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  zt_deflate_opts o;
  o.compression_type = (int)get_i64(env, a[1], 2);
  o.lazy = (int)get_i64(env, a[2], 0);
  o.level = (int)get_i64(env, a[3], -1);
  uint8_t *out = nullptr;
  size_t olen = 0;
  int rc = has_s   ? zt_deflate_raw_strategy(p, n, &o, strategy, &out, &olen)
           : has_d ? zt_deflate_raw_dict(p, n, &o, d, dn, &out, &olen)
                   : zt_deflate_raw(p, n, &o, &out, &olen);
  if (rc) return throw_zt(env, rc);
  return new_u8(env, out, olen);
}

// inflateRaw(input: Uint8Array, index, bufferType, bufferSize, refStrict[, dictionary]) -> {output, ip}
napi_value inflate_raw(napi_env env, napi_callback_info info) {
  napi_value a[6];
  args(env, info, a, 6);
  const uint8_t *d;
  size_t dn;
  bool has_d;
  if (!get_dict(env, a[5], &d, &dn, &has_d)) return nullptr;
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  const int64_t index = get_i64(env, a[1], 0);
  zt_inflate_opts o;
  o.buffer_type = (int)get_i64(env, a[2], 1);
  o.buffer_size = (size_t)get_i64(env, a[3], 0x8000);
  bool strict = false;
  napi_valuetype t;
  napi_typeof(env, a[4], &t);
  if (t == napi_boolean) napi_get_value_bool(env, a[4], &strict);
  o.ref_strict = strict ? 1 : 0;
  uint8_t *out = nullptr;
  size_t olen = 0, ip = 0;
  const size_t idx = index < 0 ? 0 : (size_t)index;
  int rc = has_d ? zt_inflate_raw_dict(p, n, idx, &o, d, dn, &out, &olen, &ip)
                 : zt_inflate_raw(p, n, idx, &o, &out, &olen, &ip);
  if (rc) return throw_zt(env, rc);
  napi_value obj, ipv;
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "output", new_u8(env, out, olen));
  napi_create_double(env, (double)ip, &ipv);
  napi_set_named_property(env, obj, "ip", ipv);
  return obj;
}

void set_num(napi_env env, napi_value obj, const char *k, double v) {
  napi_value x;
  napi_create_double(env, v, &x);
  napi_set_named_property(env, obj, k, x);
}

// inflateResume(input: Uint8Array, bitPos, window: Uint8Array[, final]) -> {output, endBits, finished}
// (final: no more input will come -- zt_inflate_raw_resume_final)
napi_value inflate_resume(napi_env env, napi_callback_info info) {
  napi_value a[4];
  args(env, info, a, 4);
  const uint8_t *p, *w;
  size_t n, wn;
  if (!get_u8(env, a[0], &p, &n) || !get_u8(env, a[2], &w, &wn)) return nullptr;
  const int64_t bit = get_i64(env, a[1], 0);
  uint8_t *out = nullptr;
  size_t olen = 0;
  uint64_t end = 0;
  int fin = 0;
  const bool final_input = get_i64(env, a[3], 0) != 0;
  int rc = (final_input ? zt_inflate_raw_resume_final : zt_inflate_raw_resume)(p, n, bit < 0 ? 0 : (uint64_t)bit, w,
                                                                               wn, &out, &olen, &end, &fin);
  if (rc) return throw_zt(env, rc);
  napi_value obj, f;
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "output", new_u8(env, out, olen));
  set_num(env, obj, "endBits", (double)end);
  napi_get_boolean(env, fin != 0, &f);
  napi_set_named_property(env, obj, "finished", f);
  return obj;
}

// optional Uint8Array argument (undefined / null -> absent)
bool opt_u8(napi_env env, napi_value v, const uint8_t **p, size_t *n, bool *present) {
  napi_valuetype t;
  napi_typeof(env, v, &t);
  *present = !(t == napi_undefined || t == napi_null);
  *p = nullptr;
  *n = 0;
  return !*present || get_u8(env, v, p, n);
}

// gzipCompress(input, compressionType, lazy, level, name|null, comment|null, hcrc, mtime[, strategy]) -> {output, crc32}
// (indexed: gzipCompressIndexed, the first eight arguments -> {output, crc32, index})
napi_value gzip_compress_any(napi_env env, napi_callback_info info, bool indexed) {
  napi_value a[9];
  args(env, info, a, 9);
  int strategy;
  const bool has_s = !indexed && get_strategy(env, a[8], &strategy);
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  zt_gzip_opts o;
  memset(&o, 0, sizeof o);
  o.deflate.compression_type = (int)get_i64(env, a[1], 2);
  o.deflate.lazy = (int)get_i64(env, a[2], 0);
  o.deflate.level = (int)get_i64(env, a[3], -1);
  bool has = false;
  if (!opt_u8(env, a[4], &o.name, &o.name_len, &has)) return nullptr;
  o.fname = has;
  if (!opt_u8(env, a[5], &o.comment, &o.comment_len, &has)) return nullptr;
  o.fcomment = has;
  bool hcrc = false;
  napi_valuetype t;
  napi_typeof(env, a[6], &t);
  if (t == napi_boolean) napi_get_value_bool(env, a[6], &hcrc);
  o.fhcrc = hcrc;
  o.mtime = get_u32(env, a[7], 0);
  uint8_t *out = nullptr, *idx = nullptr;
  size_t olen = 0, ilen = 0;
  uint32_t crc = 0;
  int rc = indexed ? zt_gzip_compress_indexed(p, n, &o, &out, &olen, &crc, &idx, &ilen)
           : has_s ? zt_gzip_compress_strategy(p, n, &o, strategy, &out, &olen, &crc)
                   : zt_gzip_compress(p, n, &o, &out, &olen, &crc);
  if (rc) return throw_zt(env, rc);
  napi_value obj;
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "output", new_u8(env, out, olen));
  set_num(env, obj, "crc32", crc);
  if (indexed) napi_set_named_property(env, obj, "index", new_u8(env, idx, ilen));
  return obj;
}
napi_value gzip_compress(napi_env env, napi_callback_info info) { return gzip_compress_any(env, info, false); }
napi_value gzip_compress_indexed(napi_env env, napi_callback_info info) { return gzip_compress_any(env, info, true); }

// [{flg, mtime, xfl, os, xlen, nameOff, nameLen, commentOff, commentLen, crc16 (or -1), crc32, isize,
//   dataOff, dataLen}] of cnt members
napi_value members_array(napi_env env, const zt_gzip_member *mem, size_t cnt) {
  napi_value arr;
  napi_create_array_with_length(env, cnt, &arr);
  for (size_t i = 0; i < cnt; ++i) {
    const zt_gzip_member &m = mem[i];
    napi_value e;
    napi_create_object(env, &e);
    set_num(env, e, "flg", m.flg);
    set_num(env, e, "mtime", m.mtime);
    set_num(env, e, "xfl", m.xfl);
    set_num(env, e, "os", m.os);
    set_num(env, e, "xlen", m.xlen);
    set_num(env, e, "nameOff", (double)m.name_off);
    set_num(env, e, "nameLen", (double)m.name_len);
    set_num(env, e, "commentOff", (double)m.comment_off);
    set_num(env, e, "commentLen", (double)m.comment_len);
    set_num(env, e, "crc16", m.has_crc16 ? (double)m.crc16 : -1.0);
    set_num(env, e, "crc32", m.crc32);
    set_num(env, e, "isize", m.isize);
    set_num(env, e, "dataOff", (double)m.data_off);
    set_num(env, e, "dataLen", (double)m.data_len);
    napi_set_element(env, arr, (uint32_t)i, e);
  }
  return arr;
}

// gunzip(input) -> {output, members: [{flg, mtime, xfl, os, xlen, nameOff, nameLen, commentOff,
//                   commentLen, crc16 (or -1), crc32, isize, dataOff, dataLen}]}
napi_value gunzip(napi_env env, napi_callback_info info) {
  napi_value a[1];
  args(env, info, a, 1);
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  uint8_t *out = nullptr;
  size_t olen = 0, cnt = 0;
  zt_gzip_member *mem = nullptr;
  int rc = zt_gunzip(p, n, &out, &olen, &mem, &cnt);
  if (rc) return throw_zt(env, rc);
  napi_value obj;
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "output", new_u8(env, out, olen));
  napi_set_named_property(env, obj, "members", members_array(env, mem, cnt));
  zt_free(mem);
  return obj;
}

// a failed item of a batch call: {status, message}
napi_value batch_failure(napi_env env, int status, size_t i) {
  napi_value e, m;
  napi_create_object(env, &e);
  set_num(env, e, "status", status);
  napi_create_string_utf8(env, zt_container_batch_message(i), NAPI_AUTO_LENGTH, &m);
  napi_set_named_property(env, e, "message", m);
  return e;
}

bool get_u8_array(napi_env env, napi_value v, std::vector<const uint8_t *> &in, std::vector<size_t> &n) {
  bool is_arr = false;
  napi_is_array(env, v, &is_arr);
  if (!is_arr) {
    napi_throw_type_error(env, nullptr, "expected an array of Uint8Array");
    return false;
  }
  uint32_t cnt = 0;
  napi_get_array_length(env, v, &cnt);
  in.resize(cnt);
  n.resize(cnt);
  for (uint32_t i = 0; i < cnt; ++i) {
    napi_value e;
    napi_get_element(env, v, i, &e);
    if (!get_u8(env, e, &in[i], &n[i])) return false;
  }
  return true;
}

// gunzipBatch(inputs: Uint8Array[]) -> [{output, members} | {status, message}]  (zt_gunzip_batch)
napi_value gunzip_batch(napi_env env, napi_callback_info info) {
  napi_value a[1];
  args(env, info, a, 1);
  std::vector<const uint8_t *> in;
  std::vector<size_t> n;
  if (!get_u8_array(env, a[0], in, n)) return nullptr;
  const size_t cnt = in.size();
  std::vector<uint8_t *> out(cnt, nullptr);
  std::vector<size_t> olen(cnt, 0), nm(cnt, 0);
  std::vector<zt_gzip_member *> mem(cnt, nullptr);
  std::vector<int> st(cnt, 0);
  const int rc = zt_gunzip_batch(in.data(), n.data(), cnt, out.data(), olen.data(), mem.data(), nm.data(), st.data());
  bool any = false;
  for (int s : st) any = any || s != 0;
  if (rc && !any) return throw_zt(env, rc);
  napi_value arr;
  napi_create_array_with_length(env, cnt, &arr);
  for (size_t i = 0; i < cnt; ++i) {
    napi_value e;
    if (st[i]) {
      e = batch_failure(env, st[i], i);
    } else {
      napi_create_object(env, &e);
      napi_set_named_property(env, e, "output", new_u8(env, out[i], olen[i]));
      napi_set_named_property(env, e, "members", members_array(env, mem[i], nm[i]));
    }
    zt_free(mem[i]);
    napi_set_element(env, arr, (uint32_t)i, e);
  }
  return arr;
}

// zlibDecompressBatch(inputs: Uint8Array[], verify[, dictionary]) -> [{output, ip, adler32} | {status, message}]
// (zt_zlib_decompress_batch / _dict; every stream from index 0)
napi_value zlib_decompress_batch(napi_env env, napi_callback_info info) {
  napi_value a[3];
  args(env, info, a, 3);
  const uint8_t *d;
  size_t dn;
  bool has_d;
  if (!get_dict(env, a[2], &d, &dn, &has_d)) return nullptr;
  std::vector<const uint8_t *> in;
  std::vector<size_t> n;
  if (!get_u8_array(env, a[0], in, n)) return nullptr;
  bool verify = false;
  napi_valuetype t;
  napi_typeof(env, a[1], &t);
  if (t == napi_boolean) napi_get_value_bool(env, a[1], &verify);
  const size_t cnt = in.size();
  std::vector<uint8_t *> out(cnt, nullptr);
  std::vector<size_t> olen(cnt, 0), ip(cnt, 0);
  std::vector<uint32_t> adler(cnt, 1);
  std::vector<int> st(cnt, 0);
  const int rc = has_d ? zt_zlib_decompress_batch_dict(in.data(), n.data(), nullptr, cnt, verify, d, dn, out.data(),
                                                       olen.data(), ip.data(), adler.data(), st.data())
                       : zt_zlib_decompress_batch(in.data(), n.data(), nullptr, cnt, verify, out.data(), olen.data(),
                                                  ip.data(), adler.data(), st.data());
  bool any = false;
  for (int s : st) any = any || s != 0;
  if (rc && !any) return throw_zt(env, rc);
  napi_value arr;
  napi_create_array_with_length(env, cnt, &arr);
  for (size_t i = 0; i < cnt; ++i) {
    napi_value e;
    if (st[i]) {
      e = batch_failure(env, st[i], i);
    } else {
      napi_create_object(env, &e);
      napi_set_named_property(env, e, "output", new_u8(env, out[i], olen[i]));
      set_num(env, e, "ip", (double)ip[i]);
      set_num(env, e, "adler32", adler[i]);
    }
    napi_set_element(env, arr, (uint32_t)i, e);
  }
  return arr;
}

// zlibCompress(input, compressionType, lazy, level) -> {output, adler32}
// (a fifth argument: the preset dictionary -- FDICT and DICTID in the header;
// a sixth: the strategy, without a dictionary)
napi_value zlib_compress(napi_env env, napi_callback_info info) {
  napi_value a[6];
  args(env, info, a, 6);
  int strategy;
  const bool has_s = get_strategy(env, a[5], &strategy);
  const uint8_t *d;
  size_t dn;
  bool has_d;
  if (!get_dict(env, a[4], &d, &dn, &has_d)) return nullptr;
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  zt_deflate_opts o;
  o.compression_type = (int)get_i64(env, a[1], 2);
  o.lazy = (int)get_i64(env, a[2], 0);
  o.level = (int)get_i64(env, a[3], -1);
  uint8_t *out = nullptr;
  size_t olen = 0;
  uint32_t adler = 1;
  int rc = has_s   ? zt_zlib_compress_strategy(p, n, &o, strategy, &out, &olen, &adler)
           : has_d ? zt_zlib_compress_dict(p, n, &o, d, dn, &out, &olen, &adler)
                   : zt_zlib_compress(p, n, &o, &out, &olen, &adler);
  if (rc) return throw_zt(env, rc);
  napi_value obj;
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "output", new_u8(env, out, olen));
  set_num(env, obj, "adler32", adler);
  return obj;
}

// zlibDecompress(input, index, verify[, dictionary]) -> {output, ip, adler32}
napi_value zlib_decompress(napi_env env, napi_callback_info info) {
  napi_value a[4];
  args(env, info, a, 4);
  const uint8_t *d;
  size_t dn;
  bool has_d;
  if (!get_dict(env, a[3], &d, &dn, &has_d)) return nullptr;
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  const int64_t index = get_i64(env, a[1], 0);
  bool verify = false;
  napi_valuetype t;
  napi_typeof(env, a[2], &t);
  if (t == napi_boolean) napi_get_value_bool(env, a[2], &verify);
  uint8_t *out = nullptr;
  size_t olen = 0, ip = 0;
  uint32_t adler = 1;
  const size_t idx = index < 0 ? 0 : (size_t)index;
  int rc = has_d ? zt_zlib_decompress_dict(p, n, idx, verify, d, dn, &out, &olen, &ip, &adler)
                 : zt_zlib_decompress(p, n, idx, verify, &out, &olen, &ip, &adler);
  if (rc) return throw_zt(env, rc);
  napi_value obj;
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "output", new_u8(env, out, olen));
  set_num(env, obj, "ip", (double)ip);
  set_num(env, obj, "adler32", adler);
  return obj;
}

napi_value prop(napi_env env, napi_value obj, const char *k) {
  napi_value v;
  napi_get_named_property(env, obj, k, &v);
  return v;
}

// zipCompress(files: [{data, name, comment (or null), method, os, mtime (4 bytes),
//             compressionType, lazy, level, password (Uint8Array or null),
//             cryptHeader (0 reference | 1 PKWARE), cryptLead (10 bytes or null)}],
//             comment: Uint8Array) -> Uint8Array
napi_value zip_compress(napi_env env, napi_callback_info info) {
  napi_value a[2];
  args(env, info, a, 2);
  uint32_t cnt = 0;
  napi_get_array_length(env, a[0], &cnt);
  std::vector<const uint8_t *> in(cnt);
  std::vector<size_t> n(cnt);
  std::vector<zt_zip_file> f(cnt);
  std::vector<zt_zip_crypt> cr(cnt);
  bool any_pw = false;
  for (uint32_t i = 0; i < cnt; ++i) {
    napi_value e;
    napi_get_element(env, a[0], i, &e);
    memset(&f[i], 0, sizeof f[i]);
    if (!get_u8(env, prop(env, e, "data"), &in[i], &n[i])) return nullptr;
    if (!get_u8(env, prop(env, e, "name"), &f[i].name, &f[i].name_len)) return nullptr;
    bool has = false;
    if (!opt_u8(env, prop(env, e, "comment"), &f[i].comment, &f[i].comment_len, &has)) return nullptr;
    f[i].method = (int)get_i64(env, prop(env, e, "method"), 8);
    f[i].os = (int)get_i64(env, prop(env, e, "os"), 0);
    const uint8_t *mt;
    size_t ml;
    if (!get_u8(env, prop(env, e, "mtime"), &mt, &ml)) return nullptr;
    for (size_t k = 0; k < 4 && k < ml; ++k) f[i].mtime[k] = mt[k];
    f[i].deflate.compression_type = (int)get_i64(env, prop(env, e, "compressionType"), 2);
    f[i].deflate.lazy = (int)get_i64(env, prop(env, e, "lazy"), 0);
    f[i].deflate.level = (int)get_i64(env, prop(env, e, "level"), -1);
    memset(&cr[i], 0, sizeof cr[i]);
    bool has_pw = false, has_lead = false;
    static const uint8_t kEmpty = 0;
    if (!opt_u8(env, prop(env, e, "password"), &cr[i].password, &cr[i].password_len, &has_pw)) return nullptr;
    if (has_pw) {
      any_pw = true;
      if (!cr[i].password) cr[i].password = &kEmpty;  // (an empty password is still one)
      cr[i].header_mode = (int)get_i64(env, prop(env, e, "cryptHeader"), 0);
      const uint8_t *ld = nullptr;
      size_t ll = 0;
      if (!opt_u8(env, prop(env, e, "cryptLead"), &ld, &ll, &has_lead)) return nullptr;
      for (size_t k = 0; k < 10 && k < ll; ++k) cr[i].lead[k] = ld[k];
    } else {
      cr[i].password = nullptr;
    }
  }
  const uint8_t *cm = nullptr;
  size_t cl = 0;
  bool has = false;
  if (!opt_u8(env, a[1], &cm, &cl, &has)) return nullptr;
  uint8_t *out = nullptr;
  size_t olen = 0;
  const int rc = any_pw ? zt_zip_compress_pw(in.data(), n.data(), f.data(), cr.data(), cnt, cm, cl, &out, &olen)
                        : zt_zip_compress(in.data(), n.data(), f.data(), cnt, cm, cl, &out, &olen);
  if (rc) return throw_zt(env, rc);
  return new_u8(env, out, olen);
}

// unzip(input, verify, password (Uint8Array or null)) -> {output, entries: [{nameOff, nameLen, ..., status, message}]}
// (archive-level errors throw; an entry's error is in its status / message)
napi_value unzip(napi_env env, napi_callback_info info) {
  napi_value a[3];
  args(env, info, a, 3);
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  bool verify = false;
  napi_valuetype t;
  napi_typeof(env, a[1], &t);
  if (t == napi_boolean) napi_get_value_bool(env, a[1], &verify);
  const uint8_t *pw = nullptr;
  size_t pwn = 0;
  bool has_pw = false;
  static const uint8_t kEmpty = 0;
  if (!opt_u8(env, a[2], &pw, &pwn, &has_pw)) return nullptr;
  if (has_pw && !pw) pw = &kEmpty;
  uint8_t *out = nullptr;
  size_t olen = 0, cnt = 0;
  zt_unzip_entry *ent = nullptr;
  const int rc = has_pw ? zt_unzip_pw(p, n, verify ? 1 : 0, pw, pwn, &out, &olen, &ent, &cnt)
                        : zt_unzip(p, n, verify ? 1 : 0, &out, &olen, &ent, &cnt);
  if (rc && !ent) return throw_zt(env, rc);
  napi_value obj, arr;
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "output", new_u8(env, out, olen));
  napi_create_array_with_length(env, cnt, &arr);
  for (size_t i = 0; i < cnt; ++i) {
    const zt_unzip_entry &m = ent[i];
    napi_value e;
    napi_create_object(env, &e);
    set_num(env, e, "nameOff", (double)m.name_off);
    set_num(env, e, "nameLen", (double)m.name_len);
    set_num(env, e, "commentOff", (double)m.comment_off);
    set_num(env, e, "commentLen", (double)m.comment_len);
    set_num(env, e, "dataOff", (double)m.data_off);
    set_num(env, e, "dataLen", (double)m.data_len);
    set_num(env, e, "relativeOffset", (double)m.local_offset);
    set_num(env, e, "version", m.version);
    set_num(env, e, "os", m.os);
    set_num(env, e, "needVersion", m.need_version);
    set_num(env, e, "flags", m.flags);
    set_num(env, e, "compression", m.method);
    set_num(env, e, "time", m.time);
    set_num(env, e, "date", m.date);
    set_num(env, e, "crc32", m.crc32);
    set_num(env, e, "compressedSize", m.compressed_size);
    set_num(env, e, "plainSize", m.plain_size);
    set_num(env, e, "status", m.status);
    napi_value msg;
    napi_create_string_utf8(env, m.message, NAPI_AUTO_LENGTH, &msg);
    napi_set_named_property(env, e, "message", msg);
    napi_set_element(env, arr, (uint32_t)i, e);
  }
  zt_free(ent);
  napi_set_named_property(env, obj, "entries", arr);
  return obj;
}

// ---- the deflate-time index (include/zt_index.h, the write side) ------------------
// deflateRawIndexed(input, compressionType, lazy, level, streamStart) -> {output, index}
napi_value deflate_raw_indexed(napi_env env, napi_callback_info info) {
  napi_value a[5];
  args(env, info, a, 5);
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  zt_deflate_opts o;
  o.compression_type = (int)get_i64(env, a[1], 2);
  o.lazy = (int)get_i64(env, a[2], 0);
  o.level = (int)get_i64(env, a[3], -1);
  const int64_t start = get_i64(env, a[4], 0);
  uint8_t *out = nullptr, *idx = nullptr;
  size_t olen = 0, ilen = 0;
  const int rc = zt_deflate_raw_indexed(p, n, &o, start < 0 ? 0 : (size_t)start, &out, &olen, &idx, &ilen);
  if (rc) return throw_zt(env, rc);
  napi_value obj;
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "output", new_u8(env, out, olen));
  napi_set_named_property(env, obj, "index", new_u8(env, idx, ilen));
  return obj;
}

// zlibCompressIndexed(input, compressionType, lazy, level) -> {output, adler32, index}
napi_value zlib_compress_indexed(napi_env env, napi_callback_info info) {
  napi_value a[4];
  args(env, info, a, 4);
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  zt_deflate_opts o;
  o.compression_type = (int)get_i64(env, a[1], 2);
  o.lazy = (int)get_i64(env, a[2], 0);
  o.level = (int)get_i64(env, a[3], -1);
  uint8_t *out = nullptr, *idx = nullptr;
  size_t olen = 0, ilen = 0;
  uint32_t adler = 1;
  const int rc = zt_zlib_compress_indexed(p, n, &o, &out, &olen, &adler, &idx, &ilen);
  if (rc) return throw_zt(env, rc);
  napi_value obj;
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "output", new_u8(env, out, olen));
  set_num(env, obj, "adler32", adler);
  napi_set_named_property(env, obj, "index", new_u8(env, idx, ilen));
  return obj;
}

// ---- indexed random access (include/zt_index.h) ----------------------------------
// inflateIndexBuild(input: Uint8Array, index) -> Uint8Array (the index blob)
napi_value inflate_index_build(napi_env env, napi_callback_info info) {
  napi_value a[2];
  args(env, info, a, 2);
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  const int64_t index = get_i64(env, a[1], 0);
  uint8_t *idx = nullptr;
  size_t ilen = 0;
  const int rc = zt_inflate_index_build(p, n, index < 0 ? 0 : (size_t)index, &idx, &ilen, nullptr, nullptr, nullptr);
  if (rc) return throw_zt(env, rc);
  return new_u8(env, idx, ilen);
}

// a Float64Array of non-negative integers (offsets, lengths) as uint64
bool get_offsets(napi_env env, napi_value v, std::vector<uint64_t> *dst) {
  bool is_ta = false;
  napi_is_typedarray(env, v, &is_ta);
  napi_typedarray_type t = napi_uint8_array;
  size_t cnt = 0, boff = 0;
  void *data = nullptr;
  napi_value ab;
  if (is_ta) napi_get_typedarray_info(env, v, &t, &cnt, &data, &ab, &boff);
  if (!is_ta || t != napi_float64_array) {
    napi_throw_type_error(env, nullptr, "expected a Float64Array");
    return false;
  }
  const double *d = static_cast<const double *>(data);
  for (size_t i = 0; i < cnt; ++i) {
    if (!(d[i] >= 0) || d[i] > 9007199254740992.0) {
      napi_throw_range_error(env, nullptr, "offset and length must be non-negative integers");
      return false;
    }
    dst->push_back((uint64_t)d[i]);
  }
  return true;
}

// `count` outputs of a ranges call as Uint8Array[]; a failed call throws
napi_value ranges_result(napi_env env, int rc, std::vector<uint8_t *> &out, const std::vector<size_t> &olen) {
  if (rc) {
    for (uint8_t *o : out) zt_free(o);
    return throw_zt(env, rc);
  }
  napi_value arr;
  napi_create_array_with_length(env, out.size(), &arr);
  for (size_t i = 0; i < out.size(); ++i) napi_set_element(env, arr, (uint32_t)i, new_u8(env, out[i], olen[i]));
  return arr;
}

// inflateRanges(input: Uint8Array, indexBlob: Uint8Array, offsets: Float64Array, lengths: Float64Array)
//   -> Uint8Array[]; the first failing range throws
// (ckpt: inflateCkptRanges, the same arguments with a checkpoint blob, include/zt_checkpoint.h)
napi_value inflate_ranges_any(napi_env env, napi_callback_info info, bool ckpt) {
  napi_value a[4];
  args(env, info, a, 4);
  const uint8_t *p, *ix;
  size_t n, in;
  if (!get_u8(env, a[0], &p, &n) || !get_u8(env, a[1], &ix, &in)) return nullptr;
  std::vector<uint64_t> off, len;
  if (!get_offsets(env, a[2], &off) || !get_offsets(env, a[3], &len)) return nullptr;
  if (off.size() != len.size()) {
    napi_throw_range_error(env, nullptr, "one length per offset");
    return nullptr;
  }
  const size_t count = off.size();
  std::vector<uint8_t *> out(count, nullptr);
  std::vector<size_t> olen(count, 0);
  std::vector<int> st(count, 0);
  const int rc = ckpt ? zt_inflate_ckpt_ranges(p, n, ix, in, off.data(), len.data(), count, out.data(), olen.data(),
                                               st.data())
                      : zt_inflate_ranges(p, n, ix, in, off.data(), len.data(), count, out.data(), olen.data(), st.data());
  return ranges_result(env, rc, out, olen);
}

napi_value inflate_ranges(napi_env env, napi_callback_info info) { return inflate_ranges_any(env, info, false); }
napi_value inflate_ckpt_ranges(napi_env env, napi_callback_info info) { return inflate_ranges_any(env, info, true); }

// ---- checkpoint index (include/zt_checkpoint.h) ------------------------------------
// inflateCkptBuild(input: Uint8Array, index, span) -> Uint8Array (the checkpoint blob)
napi_value inflate_ckpt_build(napi_env env, napi_callback_info info) {
  napi_value a[3];
  args(env, info, a, 3);
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  const int64_t index = get_i64(env, a[1], 0), span = get_i64(env, a[2], 0);
  uint8_t *idx = nullptr;
  size_t ilen = 0;
  const int rc = zt_inflate_ckpt_build(p, n, index < 0 ? 0 : (size_t)index, span < 0 ? 1 : (uint64_t)span, &idx, &ilen,
                                       nullptr, nullptr, nullptr);
  if (rc) return throw_zt(env, rc);
  return new_u8(env, idx, ilen);
}

// ---- BGZF (include/zt_bgzf.h) -----------------------------------------------------
// bgzfCompress(input, compressionType, level, blockSize, wantIndex) -> {output, gzi?}
napi_value bgzf_compress(napi_env env, napi_callback_info info) {
  napi_value a[5];
  args(env, info, a, 5);
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  zt_bgzf_opts o;
  o.deflate.compression_type = (int)get_i64(env, a[1], 2);
  o.deflate.lazy = 0;
  o.deflate.level = (int)get_i64(env, a[2], -1);
  o.block_size = get_u32(env, a[3], 0);
  bool want = false;
  napi_get_value_bool(env, a[4], &want);
  uint8_t *out = nullptr, *gzi = nullptr;
  size_t olen = 0, glen = 0;
  const int rc = zt_bgzf_compress(p, n, &o, &out, &olen, want ? &gzi : nullptr, want ? &glen : nullptr);
  if (rc) return throw_zt(env, rc);
  napi_value obj;
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "output", new_u8(env, out, olen));
  if (want) napi_set_named_property(env, obj, "gzi", new_u8(env, gzi, glen));
  return obj;
}

// bgzfIndex(input) -> Uint8Array (the .gzi); bgzfDecompress(input) -> Uint8Array
napi_value bgzf_index(napi_env env, napi_callback_info info) {
  napi_value a[1];
  args(env, info, a, 1);
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  uint8_t *gzi = nullptr;
  size_t glen = 0;
  const int rc = zt_bgzf_index(p, n, &gzi, &glen, nullptr);
  if (rc) return throw_zt(env, rc);
  return new_u8(env, gzi, glen);
}

napi_value bgzf_decompress(napi_env env, napi_callback_info info) {
  napi_value a[1];
  args(env, info, a, 1);
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  uint8_t *out = nullptr;
  size_t olen = 0;
  const int rc = zt_bgzf_decompress(p, n, &out, &olen, nullptr);
  if (rc) return throw_zt(env, rc);
  return new_u8(env, out, olen);
}

// bgzfReadRanges(input, gzi: Uint8Array | null, offsets: Float64Array, lengths: Float64Array)
//   -> Uint8Array[]; the first failing range throws
napi_value bgzf_read_ranges(napi_env env, napi_callback_info info) {
  napi_value a[4];
  args(env, info, a, 4);
  const uint8_t *p, *g;
  size_t n, gn;
  bool has_gzi;
  if (!get_u8(env, a[0], &p, &n) || !get_dict(env, a[1], &g, &gn, &has_gzi)) return nullptr;
  std::vector<uint64_t> off, len;
  if (!get_offsets(env, a[2], &off) || !get_offsets(env, a[3], &len)) return nullptr;
  if (off.size() != len.size()) {
    napi_throw_range_error(env, nullptr, "one length per offset");
    return nullptr;
  }
  const size_t count = off.size();
  std::vector<uint8_t *> out(count, nullptr);
  std::vector<size_t> olen(count, 0);
  std::vector<int> st(count, 0);
  static const uint8_t none = 0;  // (an empty Uint8Array may carry a null pointer)
  const int rc = zt_bgzf_read_ranges(p, n, has_gzi ? (g ? g : &none) : nullptr, gn, off.data(), len.data(), count,
                                     out.data(), olen.data(), st.data());
  return ranges_result(env, rc, out, olen);
}

// bgzfReadVirtual(input, begs: BigUint64Array, ends: BigUint64Array) -> Uint8Array[]
napi_value bgzf_read_virtual(napi_env env, napi_callback_info info) {
  napi_value a[3];
  args(env, info, a, 3);
  const uint8_t *p;
  size_t n;
  if (!get_u8(env, a[0], &p, &n)) return nullptr;
  std::vector<uint64_t> v[2];
  for (int k = 0; k < 2; ++k) {
    bool is_ta = false;
    napi_is_typedarray(env, a[1 + k], &is_ta);
    napi_typedarray_type t = napi_uint8_array;
    size_t cnt = 0, boff = 0;
    void *data = nullptr;
    napi_value ab;
    if (is_ta) napi_get_typedarray_info(env, a[1 + k], &t, &cnt, &data, &ab, &boff);
    if (!is_ta || t != napi_biguint64_array) {
      napi_throw_type_error(env, nullptr, "expected a BigUint64Array");
      return nullptr;
    }
    v[k].assign(static_cast<const uint64_t *>(data), static_cast<const uint64_t *>(data) + cnt);
  }
  if (v[0].size() != v[1].size()) {
    napi_throw_range_error(env, nullptr, "one end per begin");
    return nullptr;
  }
  const size_t count = v[0].size();
  std::vector<uint8_t *> out(count, nullptr);
  std::vector<size_t> olen(count, 0);
  std::vector<int> st(count, 0);
  const int rc = zt_bgzf_read_virtual(p, n, v[0].data(), v[1].data(), count, out.data(), olen.data(), st.data());
  return ranges_result(env, rc, out, olen);
}

// ---- inflate sessions (include/zt_stream.h) -----------------------------------
// A session travels through JS as an external value; its finalizer destroys
// the session unless sessionDestroy already has.
struct SessionBox {
  zt_inflate_session *s;
};

void session_finalize(napi_env, void *data, void *) {
  SessionBox *b = static_cast<SessionBox *>(data);
  zt_inflate_session_destroy(b->s);
  delete b;
}

SessionBox *get_session(napi_env env, napi_value v) {
  napi_valuetype t;
  napi_typeof(env, v, &t);
  void *data = nullptr;
  if (t == napi_external) napi_get_value_external(env, v, &data);
  SessionBox *b = static_cast<SessionBox *>(data);
  if (!b || !b->s) {
    napi_throw_type_error(env, nullptr, "expected an open inflate session");
    return nullptr;
  }
  return b;
}

// sessionCreate([window: Uint8Array]) -> session
napi_value session_create(napi_env env, napi_callback_info info) {
  napi_value a[1];
  args(env, info, a, 1);
  const uint8_t *w;
  size_t wn;
  bool given;
  if (!opt_u8(env, a[0], &w, &wn, &given)) return nullptr;
  zt_inflate_session *s = nullptr;
  const int rc = zt_inflate_session_create(w, wn, &s);
  if (rc) return throw_zt(env, rc);
  SessionBox *b = new SessionBox{s};
  napi_value ext;
  if (napi_create_external(env, b, session_finalize, nullptr, &ext) != napi_ok) {
    session_finalize(env, b, nullptr);
    return nullptr;
  }
  return ext;
}

// sessionFeed(session, chunk: Uint8Array, last) -> Uint8Array (this call's output)
napi_value session_feed(napi_env env, napi_callback_info info) {
  napi_value a[3];
  args(env, info, a, 3);
  SessionBox *b = get_session(env, a[0]);
  const uint8_t *p;
  size_t n;
  if (!b || !get_u8(env, a[1], &p, &n)) return nullptr;
  uint8_t *out = nullptr;
  size_t olen = 0;
  const int rc = zt_inflate_session_feed(b->s, p, n, get_i64(env, a[2], 0) != 0, &out, &olen);
  if (rc) return throw_zt(env, rc);
  return new_u8(env, out, olen);
}

// sessionsFeed(sessions[], chunks: Uint8Array[], last: boolean | boolean[]) -> [{output} | {status, message}]
napi_value sessions_feed(napi_env env, napi_callback_info info) {
  napi_value a[3];
  args(env, info, a, 3);
  std::vector<const uint8_t *> in;
  std::vector<size_t> n;
  if (!get_u8_array(env, a[1], in, n)) return nullptr;
  const size_t cnt = in.size();
  bool is_arr = false;
  napi_is_array(env, a[0], &is_arr);
  uint32_t ns = 0;
  if (is_arr) napi_get_array_length(env, a[0], &ns);
  if (!is_arr || ns != cnt) {
    napi_throw_type_error(env, nullptr, "expected one session per chunk");
    return nullptr;
  }
  std::vector<zt_inflate_session *> ss(cnt);
  std::vector<int> last(cnt, 0);
  bool last_arr = false;
  napi_is_array(env, a[2], &last_arr);
  for (uint32_t i = 0; i < cnt; ++i) {
    napi_value e;
    napi_get_element(env, a[0], i, &e);
    SessionBox *b = get_session(env, e);
    if (!b) return nullptr;
    ss[i] = b->s;
    napi_value f = a[2];
    if (last_arr) napi_get_element(env, a[2], i, &f);
    bool flag = false;
    napi_coerce_to_bool(env, f, &f);
    napi_get_value_bool(env, f, &flag);
    last[i] = flag;
  }
  std::vector<uint8_t *> out(cnt, nullptr);
  std::vector<size_t> olen(cnt, 0);
  std::vector<int> st(cnt, 0);
  const int rc = zt_inflate_sessions_feed(ss.data(), in.data(), n.data(), last.data(), cnt, out.data(), olen.data(),
                                          st.data());
  bool any = false;
  for (int x : st) any = any || x != 0;
  if (rc && !any) return throw_zt(env, rc);
  napi_value arr;
  napi_create_array_with_length(env, cnt, &arr);
  for (size_t i = 0; i < cnt; ++i) {
    napi_value e, m;
    napi_create_object(env, &e);
    if (st[i]) {
      set_num(env, e, "status", st[i]);
      napi_create_string_utf8(env, zt_inflate_session_message(ss[i]), NAPI_AUTO_LENGTH, &m);
      napi_set_named_property(env, e, "message", m);
      zt_free(out[i]);
    } else {
      napi_set_named_property(env, e, "output", new_u8(env, out[i], olen[i]));
    }
    napi_set_element(env, arr, (uint32_t)i, e);
  }
  return arr;
}

// sessionInfo(session) -> {totalIn, endBits, totalOut, decodedBits, crc32, adler32, pending, finished, status,
// launches, message}
napi_value session_info(napi_env env, napi_callback_info info) {
  napi_value a[1];
  args(env, info, a, 1);
  SessionBox *b = get_session(env, a[0]);
  if (!b) return nullptr;
  zt_inflate_session_info i;
  const int rc = zt_inflate_session_get_info(b->s, &i);
  if (rc) return throw_zt(env, rc);
  napi_value obj, f, m;
  napi_create_object(env, &obj);
  set_num(env, obj, "totalIn", (double)i.total_in);
  set_num(env, obj, "endBits", (double)i.end_bits);
  set_num(env, obj, "totalOut", (double)i.total_out);
  set_num(env, obj, "decodedBits", (double)i.decoded_bits);
  set_num(env, obj, "crc32", (double)i.crc32);
  set_num(env, obj, "adler32", (double)i.adler32);
  set_num(env, obj, "pending", (double)i.pending);
  set_num(env, obj, "status", (double)i.status);
  set_num(env, obj, "launches", (double)i.launches);
  napi_get_boolean(env, i.finished != 0, &f);
  napi_set_named_property(env, obj, "finished", f);
  napi_create_string_utf8(env, zt_inflate_session_message(b->s), NAPI_AUTO_LENGTH, &m);
  napi_set_named_property(env, obj, "message", m);
  return obj;
}

// sessionDestroy(session): releases the session now (the finalizer then finds nothing)
napi_value session_destroy(napi_env env, napi_callback_info info) {
  napi_value a[1];
  const napi_value undef = args(env, info, a, 1);
  napi_valuetype t;
  napi_typeof(env, a[0], &t);
  void *data = nullptr;
  if (t == napi_external) napi_get_value_external(env, a[0], &data);
  if (SessionBox *b = static_cast<SessionBox *>(data)) {
    zt_inflate_session_destroy(b->s);
    b->s = nullptr;
  }
  return undef;
}

// ---- container sessions (include/zt_stream_container.h) ---------------------------
struct ContainerBox {
  zt_container_session *s;
};

void container_finalize(napi_env, void *data, void *) {
  ContainerBox *b = static_cast<ContainerBox *>(data);
  zt_container_session_destroy(b->s);
  delete b;
}

ContainerBox *get_container(napi_env env, napi_value v) {
  napi_valuetype t;
  napi_typeof(env, v, &t);
  void *data = nullptr;
  if (t == napi_external) napi_get_value_external(env, v, &data);
  ContainerBox *b = static_cast<ContainerBox *>(data);
  if (!b || !b->s) {
    napi_throw_type_error(env, nullptr, "expected an open container session");
    return nullptr;
  }
  return b;
}

// containerSessionCreate(format, [dictionary: Uint8Array], verify) -> session
napi_value container_session_create(napi_env env, napi_callback_info info) {
  napi_value a[3];
  args(env, info, a, 3);
  const uint8_t *d;
  size_t dn;
  bool given;
  if (!opt_u8(env, a[1], &d, &dn, &given)) return nullptr;
  zt_container_session *s = nullptr;
  const int rc = zt_container_session_create((int)get_i64(env, a[0], 0), dn ? d : nullptr, dn,
                                             get_i64(env, a[2], 1) != 0, &s);
  if (rc) return throw_zt(env, rc);
  ContainerBox *b = new ContainerBox{s};
  napi_value ext;
  if (napi_create_external(env, b, container_finalize, nullptr, &ext) != napi_ok) {
    container_finalize(env, b, nullptr);
    return nullptr;
  }
  return ext;
}

// containerSessionFeed(session, chunk: Uint8Array, last) -> Uint8Array (this call's output); the error it
// throws carries `output`: the bytes the call decoded before the error
napi_value container_session_feed(napi_env env, napi_callback_info info) {
  napi_value a[3];
  args(env, info, a, 3);
  ContainerBox *b = get_container(env, a[0]);
  const uint8_t *p;
  size_t n;
  if (!b || !get_u8(env, a[1], &p, &n)) return nullptr;
  uint8_t *out = nullptr;
  size_t olen = 0;
  const int rc = zt_container_session_feed(b->s, p, n, get_i64(env, a[2], 0) != 0, &out, &olen);
  if (rc) {
    const char *msg = zt_last_error_message();
    char codebuf[16];
    snprintf(codebuf, sizeof codebuf, "%d", rc);
    napi_value err, m, c, num;
    napi_create_string_utf8(env, msg ? msg : "libzt error", NAPI_AUTO_LENGTH, &m);
    napi_create_string_utf8(env, codebuf, NAPI_AUTO_LENGTH, &c);
    napi_create_error(env, c, m, &err);
    napi_create_int32(env, rc, &num);
    napi_set_named_property(env, err, "ztStatus", num);
    napi_set_named_property(env, err, "output", new_u8(env, out, olen));
    napi_throw(env, err);
    return nullptr;
  }
  return new_u8(env, out, olen);
}

// containerSessionsFeed(sessions[], chunks: Uint8Array[], last: boolean | boolean[])
//   -> [{output} | {status, message, output}]  (a failing item's output: what the call decoded before the error)
napi_value container_sessions_feed(napi_env env, napi_callback_info info) {
  napi_value a[3];
  args(env, info, a, 3);
  std::vector<const uint8_t *> in;
  std::vector<size_t> n;
  if (!get_u8_array(env, a[1], in, n)) return nullptr;
  const size_t cnt = in.size();
  bool is_arr = false;
  napi_is_array(env, a[0], &is_arr);
  uint32_t ns = 0;
  if (is_arr) napi_get_array_length(env, a[0], &ns);
  if (!is_arr || ns != cnt) {
    napi_throw_type_error(env, nullptr, "expected one session per chunk");
    return nullptr;
  }
  std::vector<zt_container_session *> ss(cnt);
  std::vector<int> last(cnt, 0);
  bool last_arr = false;
  napi_is_array(env, a[2], &last_arr);
  for (uint32_t i = 0; i < cnt; ++i) {
    napi_value e;
    napi_get_element(env, a[0], i, &e);
    ContainerBox *b = get_container(env, e);
    if (!b) return nullptr;
    ss[i] = b->s;
    napi_value f = a[2];
    if (last_arr) napi_get_element(env, a[2], i, &f);
    bool flag = false;
    napi_coerce_to_bool(env, f, &f);
    napi_get_value_bool(env, f, &flag);
    last[i] = flag;
  }
  std::vector<uint8_t *> out(cnt, nullptr);
  std::vector<size_t> olen(cnt, 0);
  std::vector<int> st(cnt, 0);
  const int rc = zt_container_sessions_feed(ss.data(), in.data(), n.data(), last.data(), cnt, out.data(), olen.data(),
                                            st.data());
  bool any = false;
  for (int x : st) any = any || x != 0;
  if (rc && !any) return throw_zt(env, rc);
  napi_value arr;
  napi_create_array_with_length(env, cnt, &arr);
  for (size_t i = 0; i < cnt; ++i) {
    napi_value e, m;
    napi_create_object(env, &e);
    if (st[i]) {
      set_num(env, e, "status", st[i]);
      napi_create_string_utf8(env, zt_container_session_message(ss[i]), NAPI_AUTO_LENGTH, &m);
      napi_set_named_property(env, e, "message", m);
    }
    napi_set_named_property(env, e, "output", new_u8(env, out[i], olen[i]));
    napi_set_element(env, arr, (uint32_t)i, e);
  }
  return arr;
}

// containerSessionInfo(session) -> {totalIn, totalOut, membersDone, unused, decodedBits, endBits, crc32, adler32,
// atMemberEnd, finished, status, launches, format, pending, message, members: [...]}
napi_value container_session_info(napi_env env, napi_callback_info info) {
  napi_value a[1];
  args(env, info, a, 1);
  ContainerBox *b = get_container(env, a[0]);
  if (!b) return nullptr;
  zt_container_session_info i;
  const int rc = zt_container_session_get_info(b->s, &i);
  if (rc) return throw_zt(env, rc);
  napi_value obj, f, m, arr;
  napi_create_object(env, &obj);
  set_num(env, obj, "totalIn", (double)i.total_in);
  set_num(env, obj, "totalOut", (double)i.total_out);
  set_num(env, obj, "membersDone", (double)i.members_done);
  set_num(env, obj, "unused", (double)i.unused);
  set_num(env, obj, "decodedBits", (double)i.decoded_bits);
  set_num(env, obj, "endBits", (double)i.end_bits);
  set_num(env, obj, "crc32", (double)i.crc32);
  set_num(env, obj, "adler32", (double)i.adler32);
  set_num(env, obj, "status", (double)i.status);
  set_num(env, obj, "launches", (double)i.launches);
  set_num(env, obj, "format", (double)i.format);
  set_num(env, obj, "pending", (double)i.pending);
  napi_get_boolean(env, i.finished != 0, &f);
  napi_set_named_property(env, obj, "finished", f);
  napi_get_boolean(env, i.at_member_end != 0, &f);
  napi_set_named_property(env, obj, "atMemberEnd", f);
  napi_create_string_utf8(env, zt_container_session_message(b->s), NAPI_AUTO_LENGTH, &m);
  napi_set_named_property(env, obj, "message", m);
  napi_create_array_with_length(env, (size_t)i.members_done, &arr);
  for (size_t k = 0; k < i.members_done; ++k) {
    zt_container_member cm;
    if (zt_container_session_member(b->s, k, &cm)) break;
    napi_value e;
    napi_create_object(env, &e);
    set_num(env, e, "flg", cm.flg);
    set_num(env, e, "mtime", cm.mtime);
    set_num(env, e, "xfl", cm.xfl);
    set_num(env, e, "os", cm.os);
    set_num(env, e, "xlen", cm.xlen);
    set_num(env, e, "hasCrc16", cm.has_crc16);
    set_num(env, e, "crc16", cm.crc16);
    set_num(env, e, "crc32", cm.crc32);
    set_num(env, e, "isize", cm.isize);
    set_num(env, e, "dataOff", (double)cm.data_off);
    set_num(env, e, "dataLen", (double)cm.data_len);
    set_num(env, e, "inOff", (double)cm.in_off);
    for (int which = 0; which < 2; ++which) {
      const bool has = cm.flg & (which ? 0x10u : 0x08u);
      const uint8_t *src = which ? cm.comment : cm.name;
      const size_t len = which ? cm.comment_len : cm.name_len;
      napi_value v;
      if (has) {
        void *dst = nullptr;
        napi_value ab;
        napi_create_arraybuffer(env, len, &dst, &ab);
        if (len) memcpy(dst, src, len);
        napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &v);
      } else {
        napi_get_null(env, &v);
      }
      napi_set_named_property(env, e, which ? "comment" : "name", v);
    }
    napi_set_element(env, arr, (uint32_t)k, e);
  }
  napi_set_named_property(env, obj, "members", arr);
  return obj;
}

// containerSessionDestroy(session): releases the session now (the finalizer then finds nothing)
napi_value container_session_destroy(napi_env env, napi_callback_info info) {
  napi_value a[1];
  const napi_value undef = args(env, info, a, 1);
  napi_valuetype t;
  napi_typeof(env, a[0], &t);
  void *data = nullptr;
  if (t == napi_external) napi_get_value_external(env, a[0], &data);
  if (ContainerBox *b = static_cast<ContainerBox *>(data)) {
    zt_container_session_destroy(b->s);
    b->s = nullptr;
  }
  return undef;
}

napi_value device_count(napi_env env, napi_callback_info) {
  napi_value r;
  napi_create_int32(env, zt_device_count(), &r);
  return r;
}

napi_value version(napi_env env, napi_callback_info) {
  napi_value r;
  napi_create_string_utf8(env, zt_version(), NAPI_AUTO_LENGTH, &r);
  return r;
}

napi_value init(napi_env env, napi_value exports) {
  napi_property_descriptor d[] = {
      {"crc32Update", nullptr, crc32_update, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"adler32Update", nullptr, adler32_update, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"deflateRaw", nullptr, deflate_raw, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"inflateRaw", nullptr, inflate_raw, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"inflateResume", nullptr, inflate_resume, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"gzipCompress", nullptr, gzip_compress, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"gunzip", nullptr, gunzip, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"zlibCompress", nullptr, zlib_compress, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"zlibDecompress", nullptr, zlib_decompress, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"gunzipBatch", nullptr, gunzip_batch, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"zlibDecompressBatch", nullptr, zlib_decompress_batch, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"zipCompress", nullptr, zip_compress, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"unzip", nullptr, unzip, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"inflateIndexBuild", nullptr, inflate_index_build, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"deflateRawIndexed", nullptr, deflate_raw_indexed, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"gzipCompressIndexed", nullptr, gzip_compress_indexed, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"zlibCompressIndexed", nullptr, zlib_compress_indexed, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"inflateRanges", nullptr, inflate_ranges, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"inflateCkptBuild", nullptr, inflate_ckpt_build, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"inflateCkptRanges", nullptr, inflate_ckpt_ranges, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"bgzfCompress", nullptr, bgzf_compress, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"bgzfIndex", nullptr, bgzf_index, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"bgzfDecompress", nullptr, bgzf_decompress, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"bgzfReadRanges", nullptr, bgzf_read_ranges, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"bgzfReadVirtual", nullptr, bgzf_read_virtual, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"sessionCreate", nullptr, session_create, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"sessionFeed", nullptr, session_feed, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"sessionsFeed", nullptr, sessions_feed, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"sessionInfo", nullptr, session_info, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"sessionDestroy", nullptr, session_destroy, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"containerSessionCreate", nullptr, container_session_create, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"containerSessionFeed", nullptr, container_session_feed, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"containerSessionsFeed", nullptr, container_sessions_feed, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"containerSessionInfo", nullptr, container_session_info, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"containerSessionDestroy", nullptr, container_session_destroy, nullptr, nullptr, nullptr, napi_enumerable,
       nullptr},
      {"deviceCount", nullptr, device_count, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"version", nullptr, version, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
  };
  napi_define_properties(env, exports, sizeof d / sizeof d[0], d);
  return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
