// zipcrypto_api.cpp -- host side of the raw ZipCrypto batch calls
// (include/zt_zipcrypto.h) and the batch helper zip_api.cpp encrypts through.
//
// Encrypt: the streams are packed from tile boundaries into one host buffer,
// uploaded once, encrypted in place by the seven launches of zipcrypto.hip and
// downloaded once.  Decrypt: packed at 16-byte boundaries, one lane per stream.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "zipcrypto.h"
#include "zt_internal.h"

namespace zt {
namespace zc {

namespace {
thread_local double g_last_ms = 0;

struct DevBuf {
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t n) {
    if (const hipError_t e = hipMalloc(&p, n ? n : 16)) {
      p = nullptr;
      (void)hipGetLastError();
      return hip_fail(e, "hipMalloc (zipcrypto)");
    }
    return ZT_OK;
  }
};
struct Events {
  hipEvent_t a = nullptr, b = nullptr;
  ~Events() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};
struct HostFree {
  void operator()(uint8_t *p) const { free(p); }
};
}  // namespace

int crypt_items(bool encrypt, const Src *src, const Keys *keys, size_t count, uint8_t *const *dst) {
  g_last_ms = 0;
  DeviceCtx *c;
  ZT_TRY(get_ctx(&c));
  std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);
  if (count == 0) return ZT_OK;
  // layout of the packed buffer
  std::vector<size_t> off(count), len(count);
  std::vector<Tile> tiles;
  std::vector<Item> items;
  std::vector<Stream> streams;
  size_t packed = 0;
  for (size_t i = 0; i < count; ++i) {
    len[i] = src[i].head_len + src[i].body_len;
    off[i] = packed;
    if (encrypt) {
      const size_t nt = (len[i] + kTile - 1) / kTile;
      Item it{};
      it.first_tile = tiles.size();
      it.ntiles = nt;
      memcpy(it.key, keys[i].k, sizeof it.key);
      items.push_back(it);
      for (size_t t = 0; t < nt; ++t)
        tiles.push_back(Tile{(uint32_t)i, (uint32_t)std::min<size_t>(kTile, len[i] - t * kTile)});
      packed += nt * kTile;
    } else {
      Stream st{};
      st.off = packed;
      st.len = len[i];
      memcpy(st.key, keys[i].k, sizeof st.key);
      streams.push_back(st);
      packed += (len[i] + 15) & ~(size_t)15;
    }
  }
  if (packed == 0) return ZT_OK;
  std::unique_ptr<uint8_t, HostFree> h(host_out(packed));
  if (!h) return set_error(ZT_E_NOMEM, "host allocation failed");
  for (size_t i = 0; i < count; ++i) {
    uint8_t *p = h.get() + off[i];
    if (src[i].head_len) memcpy(p, src[i].head, src[i].head_len);
    if (src[i].body_len) memcpy(p + src[i].head_len, src[i].body, src[i].body_len);
  }
  DevBuf d_data, d_tab, d_work;
  ZT_TRY(d_data.alloc(packed));
  ZT_TRY(upload(c, d_data.p, h.get(), packed, c->stream));
  Events ev;
  ZT_HIP(hipEventCreate(&ev.a));
  ZT_HIP(hipEventCreate(&ev.b));
  if (encrypt) {
    const size_t tb = tiles.size() * sizeof(Tile);
    ZT_TRY(d_tab.alloc(tb + items.size() * sizeof(Item)));
    ZT_TRY(d_work.alloc(encrypt_work_bytes(tiles.size())));
    uint8_t *tp = static_cast<uint8_t *>(d_tab.p);
    ZT_HIP(hipMemcpyAsync(tp, tiles.data(), tb, hipMemcpyHostToDevice, c->stream));
    ZT_HIP(hipMemcpyAsync(tp + tb, items.data(), items.size() * sizeof(Item), hipMemcpyHostToDevice, c->stream));
    ZT_HIP(hipEventRecord(ev.a, c->stream));
    ZT_TRY(encrypt_dev(static_cast<uint8_t *>(d_data.p), reinterpret_cast<const Tile *>(tp), tiles.size(),
                       reinterpret_cast<const Item *>(tp + tb), items.size(), d_work.p, c->stream));
  } else {
    ZT_TRY(d_tab.alloc(streams.size() * sizeof(Stream)));
    ZT_HIP(hipMemcpyAsync(d_tab.p, streams.data(), streams.size() * sizeof(Stream), hipMemcpyHostToDevice,
                          c->stream));
    ZT_HIP(hipEventRecord(ev.a, c->stream));
    ZT_TRY(decrypt_dev(static_cast<uint8_t *>(d_data.p), static_cast<const Stream *>(d_tab.p), streams.size(),
                       c->stream));
  }
  ZT_HIP(hipEventRecord(ev.b, c->stream));
  ZT_TRY(download(c, h.get(), d_data.p, packed, c->stream));
  ZT_HIP(hipStreamSynchronize(c->stream));
  float ms = 0;
  ZT_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
  g_last_ms = ms;
  for (size_t i = 0; i < count; ++i)
    if (len[i]) memcpy(dst[i], h.get() + off[i], len[i]);
  return ZT_OK;
}

}  // namespace zc
}  // namespace zt

using namespace zt;

namespace {
int raw_batch(bool encrypt, const uint8_t *const *in, const size_t *n, size_t count, const uint8_t *const *pw,
              const size_t *pw_len, uint8_t **out) {
  if (count == 0) {
    DeviceCtx *c;
    return get_ctx(&c);
  }
  if (!in || !n || !pw || !pw_len || !out) return set_error(ZT_E_ARG, "null argument");
  std::vector<zc::Src> src(count);
  std::vector<zc::Keys> keys(count);
  size_t total = 0;
  for (size_t i = 0; i < count; ++i) {
    if ((n[i] && !in[i]) || (pw_len[i] && !pw[i])) return set_error(ZT_E_ARG, "null argument");
    src[i] = zc::Src{nullptr, 0, in[i], n[i]};
    keys[i] = zc::create_key(pw[i], pw_len[i]);
    total += n[i] ? n[i] : 1;  // (every output pointer distinct)
    out[i] = nullptr;
  }
  {
    DeviceCtx *c;
    ZT_TRY(get_ctx(&c));
  }
  uint8_t *base = slab_out(total, count);
  if (!base) return set_error(ZT_E_NOMEM, "host allocation failed");
  size_t p = 0;
  for (size_t i = 0; i < count; ++i) {
    out[i] = base + p;
    p += n[i] ? n[i] : 1;
  }
  const int rc = zc::crypt_items(encrypt, src.data(), keys.data(), count, out);
  if (rc)
    for (size_t i = 0; i < count; ++i) {
      zt_free(out[i]);
      out[i] = nullptr;
    }
  return rc;
}
}  // namespace

extern "C" {

int zt_zipcrypto_encrypt_batch(const uint8_t *const *in, const size_t *n, size_t count, const uint8_t *const *pw,
                               const size_t *pw_len, uint8_t **out) {
  return raw_batch(true, in, n, count, pw, pw_len, out);
}

int zt_zipcrypto_decrypt_batch(const uint8_t *const *in, const size_t *n, size_t count, const uint8_t *const *pw,
                               const size_t *pw_len, uint8_t **out) {
  return raw_batch(false, in, n, count, pw, pw_len, out);
}

size_t zt_zipcrypto_tile_bytes(void) { return zc::kTile; }
size_t zt_zipcrypto_chunk_bytes(void) { return zc::kChunk; }

int zt_zipcrypto_last_kernel_ms(double *ms) {
  if (!ms) return set_error(ZT_E_ARG, "null output");
  *ms = zc::g_last_ms;
  return ZT_OK;
}

}  // extern "C"
