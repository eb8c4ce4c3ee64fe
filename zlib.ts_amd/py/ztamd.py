"""ztamd -- ctypes binding of libzt.so (include/zt.h) for tests and bench.py.

This is plumbing over the C-ABI, not a second implementation: every call runs
on the GPU through libzt.so.  Importing fails loudly when the library has not
been built (``make -C zlib.ts_amd`` / ``__graft_entry__.build()``).
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.environ.get("ZT_LIB") or os.path.join(os.path.dirname(HERE), "libzt.so")

ZT_OK = 0
ERRORS = {
    -1: "ZT_E_INVALID_COMPRESSION_TYPE", -2: "ZT_E_INVALID_INDEX", -10: "ZT_E_INPUT_BROKEN",
    -11: "ZT_E_INVALID_CODE_LENGTH", -12: "ZT_E_UNKNOWN_BTYPE", -13: "ZT_E_STORED_LEN", -14: "ZT_E_STORED_NLEN",
    -15: "ZT_E_INVALID_DISTANCE", -16: "ZT_E_INVALID_SYMBOL", -17: "ZT_E_BAD_TREE",
    -30: "ZT_E_GZIP_SIGNATURE", -31: "ZT_E_GZIP_METHOD", -32: "ZT_E_GZIP_HCRC", -33: "ZT_E_GZIP_CRC32",
    -34: "ZT_E_GZIP_ISIZE", -40: "ZT_E_ZLIB_METHOD", -41: "ZT_E_ZLIB_FCHECK", -42: "ZT_E_ZLIB_FDICT",
    -43: "ZT_E_ZLIB_ADLER", -44: "ZT_E_ZLIB_DICTID", -50: "ZT_E_ZIP_FORMAT", -51: "ZT_E_ZIP_CRC", -52: "ZT_E_ZIP_ENCRYPTED",
    -60: "ZT_E_NO_INDEX", -61: "ZT_E_INDEX", -62: "ZT_E_INDEX_MISMATCH", -70: "ZT_E_BGZF_FORMAT",
    -71: "ZT_E_BGZF_INDEX", -100: "ZT_E_NO_DEVICE",
    -101: "ZT_E_HIP", -102: "ZT_E_NOMEM", -103: "ZT_E_ARG", -104: "ZT_E_INTERNAL",
}


class ZtError(Exception):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code
        self.msg = msg


class DeflateOpts(ctypes.Structure):
    _fields_ = [("compression_type", ctypes.c_int), ("lazy", ctypes.c_int), ("level", ctypes.c_int)]


class KernelTimes(ctypes.Structure):
    _fields_ = [("deflate_ms", ctypes.c_double), ("deflate_launches", ctypes.c_uint64),
                ("inflate_ms", ctypes.c_double), ("inflate_launches", ctypes.c_uint64),
                ("deflate_pipeline_ms", ctypes.c_double), ("deflate_pipelines", ctypes.c_uint64),
                ("inflate_tok_ms", ctypes.c_double), ("inflate_toks", ctypes.c_uint64),
                ("inflate_paths", ctypes.c_uint64 * 3), ("general_passes", ctypes.c_uint64),
                ("blocks_unsearched", ctypes.c_uint64)]


class ZipFile(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("name_len", ctypes.c_size_t), ("comment", ctypes.c_char_p),
                ("comment_len", ctypes.c_size_t), ("method", ctypes.c_int), ("os", ctypes.c_int),
                ("mtime", ctypes.c_uint8 * 4), ("deflate", DeflateOpts)]


class ZipCrypt(ctypes.Structure):
    _fields_ = [("password", ctypes.c_char_p), ("password_len", ctypes.c_size_t), ("header_mode", ctypes.c_int),
                ("lead", ctypes.c_uint8 * 10)]


class UnzipEntry(ctypes.Structure):
    _fields_ = [("name_off", ctypes.c_size_t), ("name_len", ctypes.c_size_t), ("comment_off", ctypes.c_size_t),
                ("comment_len", ctypes.c_size_t), ("data_off", ctypes.c_size_t), ("data_len", ctypes.c_size_t),
                ("local_offset", ctypes.c_size_t)] + [
                    (f, ctypes.c_uint32) for f in ("version", "os", "need_version", "flags", "method", "time", "date",
                                                   "crc32", "compressed_size", "plain_size", "local_crc32",
                                                   "local_method", "data_crc32")] + [
                    ("status", ctypes.c_int32), ("message", ctypes.c_char * 96)]


class InflateOpts(ctypes.Structure):
    _fields_ = [("buffer_type", ctypes.c_int), ("buffer_size", ctypes.c_size_t), ("ref_strict", ctypes.c_int)]


class GzipOpts(ctypes.Structure):
    _fields_ = [("deflate", DeflateOpts), ("fname", ctypes.c_int), ("fcomment", ctypes.c_int),
                ("fhcrc", ctypes.c_int), ("mtime", ctypes.c_uint32), ("name", ctypes.c_char_p),
                ("name_len", ctypes.c_size_t), ("comment", ctypes.c_char_p), ("comment_len", ctypes.c_size_t)]


class GzipMember(ctypes.Structure):
    _fields_ = [("flg", ctypes.c_uint32), ("mtime", ctypes.c_uint32), ("xfl", ctypes.c_uint32),
                ("os", ctypes.c_uint32), ("xlen", ctypes.c_uint32), ("name_off", ctypes.c_size_t),
                ("name_len", ctypes.c_size_t), ("comment_off", ctypes.c_size_t), ("comment_len", ctypes.c_size_t),
                ("has_crc16", ctypes.c_uint32), ("crc16", ctypes.c_uint32), ("crc32", ctypes.c_uint32),
                ("isize", ctypes.c_uint32), ("data_off", ctypes.c_size_t), ("data_len", ctypes.c_size_t)]


class GunzipBatchStats(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in ("items", "candidates", "members", "decode_passes", "redecoded")]


class IndexStats(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in ("builds", "range_calls", "ranges", "units_tokenized",
                                               "in_bytes_uploaded", "out_bytes_decoded", "out_bytes_returned")]


class CkptStats(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in ("builds", "range_calls", "ranges", "units_tokenized",
                                               "in_bytes_uploaded", "out_bytes_decoded", "out_bytes_returned",
                                               "window_bytes_uploaded")]


class BgzfOpts(ctypes.Structure):
    _fields_ = [("deflate", DeflateOpts), ("block_size", ctypes.c_uint32)]


class BgzfInfo(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in ("blocks", "data_blocks", "total_out", "error_offset")] + [
        ("has_eof", ctypes.c_int)]


class BgzfStats(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in ("range_calls", "ranges", "blocks_decoded", "in_bytes_uploaded",
                                               "out_bytes_decoded", "out_bytes_returned")]


class InflateSessionInfo(ctypes.Structure):
    _fields_ = [("total_in", ctypes.c_uint64), ("end_bits", ctypes.c_uint64), ("total_out", ctypes.c_uint64),
                ("decoded_bits", ctypes.c_uint64), ("crc32", ctypes.c_uint32), ("adler32", ctypes.c_uint32),
                ("pending", ctypes.c_uint32), ("finished", ctypes.c_int32), ("status", ctypes.c_int32),
                ("launches", ctypes.c_uint32)]


class ContainerSessionInfo(ctypes.Structure):
    _fields_ = [("total_in", ctypes.c_uint64), ("total_out", ctypes.c_uint64), ("members_done", ctypes.c_uint64),
                ("unused", ctypes.c_uint64), ("decoded_bits", ctypes.c_uint64), ("end_bits", ctypes.c_uint64),
                ("crc32", ctypes.c_uint32), ("adler32", ctypes.c_uint32), ("at_member_end", ctypes.c_int32),
                ("finished", ctypes.c_int32), ("status", ctypes.c_int32), ("launches", ctypes.c_uint32),
                ("format", ctypes.c_int32), ("pending", ctypes.c_uint32)]


class ContainerMember(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("flg", "mtime", "xfl", "os", "xlen", "has_crc16", "crc16", "crc32",
                                               "isize", "pad")] + [
        ("name", ctypes.c_void_p), ("name_len", ctypes.c_size_t), ("comment", ctypes.c_void_p),
        ("comment_len", ctypes.c_size_t), ("data_off", ctypes.c_uint64), ("data_len", ctypes.c_uint64),
        ("in_off", ctypes.c_uint64)]


def _load():
    # torch (when present) ships its own libamdhip64.so.7; loading it first makes
    # libzt.so bind to that same runtime (same SONAME) instead of starting a
    # second HIP runtime in the process, which would leave torch without a GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIBPATH):
        raise ImportError(f"libzt.so not built at {LIBPATH}; run make -C zlib.ts_amd")
    lib = ctypes.CDLL(LIBPATH)
    sz, vp, u32 = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32
    u8pp = ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))
    P = ctypes.POINTER
    sig = {
        "zt_device_count": ([], ctypes.c_int),
        "zt_set_device": ([ctypes.c_int], ctypes.c_int),
        "zt_set_devices": ([ctypes.c_uint64], ctypes.c_int),
        "zt_last_error_message": ([], ctypes.c_char_p),
        "zt_version": ([], ctypes.c_char_p),
        "zt_free": ([vp], None),
        "zt_crc32_update": ([u32, vp, sz, P(u32)], ctypes.c_int),
        "zt_adler32_update": ([u32, vp, sz, P(u32)], ctypes.c_int),
        "zt_checksums": ([vp, sz, u32, u32, P(u32), P(u32)], ctypes.c_int),
        "zt_deflate_raw": ([vp, sz, P(DeflateOpts), u8pp, P(sz)], ctypes.c_int),
        "zt_inflate_raw": ([vp, sz, sz, P(InflateOpts), u8pp, P(sz), P(sz)], ctypes.c_int),
        "zt_inflate_raw_resume": ([vp, sz, ctypes.c_uint64, vp, sz, u8pp, P(sz), P(ctypes.c_uint64),
                                   P(ctypes.c_int)], ctypes.c_int),
        "zt_inflate_raw_resume_final": ([vp, sz, ctypes.c_uint64, vp, sz, u8pp, P(sz), P(ctypes.c_uint64),
                                         P(ctypes.c_int)], ctypes.c_int),
        "zt_inflate_raw_batch": ([P(vp), P(sz), sz, P(InflateOpts), u8pp, P(sz), P(sz), P(ctypes.c_int)],
                                 ctypes.c_int),
        "zt_deflate_raw_batch": ([P(vp), P(sz), sz, P(DeflateOpts), u8pp, P(sz), P(ctypes.c_int)], ctypes.c_int),
        "zt_gzip_compress": ([vp, sz, P(GzipOpts), u8pp, P(sz), P(u32)], ctypes.c_int),
        "zt_gzip_compress_batch": ([P(vp), P(sz), sz, P(GzipOpts), u8pp, P(sz), P(ctypes.c_int)], ctypes.c_int),
        "zt_zlib_compress_batch": ([P(vp), P(sz), sz, P(DeflateOpts), u8pp, P(sz), P(ctypes.c_int)], ctypes.c_int),
        "zt_crc32_batch": ([P(vp), P(sz), sz, P(u32)], ctypes.c_int),
        "zt_zip_compress": ([P(vp), P(sz), P(ZipFile), sz, vp, sz, u8pp, P(sz)], ctypes.c_int),
        "zt_unzip": ([vp, sz, ctypes.c_int, u8pp, P(sz), P(P(UnzipEntry)), P(sz)], ctypes.c_int),
        "zt_gunzip": ([vp, sz, u8pp, P(sz), P(P(GzipMember)), P(sz)], ctypes.c_int),
        "zt_zlib_compress": ([vp, sz, P(DeflateOpts), u8pp, P(sz), P(u32)], ctypes.c_int),
        "zt_zlib_decompress": ([vp, sz, sz, ctypes.c_int, u8pp, P(sz), P(sz), P(u32)], ctypes.c_int),
        "zt_dev_checksums": ([vp, sz, u32, u32, P(u32), P(u32), vp], ctypes.c_int),
        "zt_deflate_plan_create": ([sz, P(DeflateOpts), P(vp)], ctypes.c_int),
        "zt_deflate_plan_destroy": ([vp], None),
        "zt_deflate_bound": ([sz], sz),
        "zt_deflate_dev": ([vp, vp, sz, sz, ctypes.c_int, vp, P(sz), vp], ctypes.c_int),
        "zt_inflate_plan_create": ([sz, sz, P(vp)], ctypes.c_int),
        "zt_inflate_plan_destroy": ([vp], None),
        "zt_inflate_dev": ([vp, vp, sz, vp, sz, P(sz), P(sz), vp], ctypes.c_int),
        "zt_synth_dev": ([ctypes.c_int, u32, vp, sz, vp], ctypes.c_int),
        "zt_synth_dev_at": ([ctypes.c_int, u32, ctypes.c_uint64, vp, sz, vp], ctypes.c_int),
        "zt_timing_enable": ([ctypes.c_int], ctypes.c_int),
        "zt_timing_read": ([P(KernelTimes)], ctypes.c_int),
        "zt_scratch_bytes": ([P(sz), P(sz)], ctypes.c_int),
        "zt_release_scratch": ([], ctypes.c_int),
        # debug (csrc/zt_internal.h)
        "zt_debug_match_modes": ([P(ctypes.c_uint64)], ctypes.c_int),
        "zt_debug_head_formats": ([P(ctypes.c_uint64)], ctypes.c_int),
        "zt_debug_match": ([vp, sz, sz, ctypes.c_int, vp, vp, vp], ctypes.c_int),
        "zt_debug_huffman": ([vp, u32, u32, u32, vp, vp], ctypes.c_int),
        "zt_debug_chain": ([vp, vp, vp, u32, ctypes.c_uint64, ctypes.c_uint64, u32, vp, vp, vp], ctypes.c_int),
        "zt_debug_chain_host": ([vp, vp, vp, u32, vp, vp, vp, P(u32), P(ctypes.c_int)], ctypes.c_int),
        # include/zt_zipcrypto.h
        "zt_zipcrypto_encrypt_batch": ([P(vp), P(sz), sz, P(vp), P(sz), u8pp], ctypes.c_int),
        "zt_zipcrypto_decrypt_batch": ([P(vp), P(sz), sz, P(vp), P(sz), u8pp], ctypes.c_int),
        "zt_zipcrypto_tile_bytes": ([], sz),
        "zt_zipcrypto_chunk_bytes": ([], sz),
        "zt_zipcrypto_last_kernel_ms": ([P(ctypes.c_double)], ctypes.c_int),
        "zt_zip_compress_pw": ([P(vp), P(sz), P(ZipFile), P(ZipCrypt), sz, vp, sz, u8pp, P(sz)], ctypes.c_int),
        "zt_unzip_pw": ([vp, sz, ctypes.c_int, vp, sz, u8pp, P(sz), P(P(UnzipEntry)), P(sz)], ctypes.c_int),
        # include/zt_dict.h
        "zt_deflate_raw_dict": ([vp, sz, P(DeflateOpts), vp, sz, u8pp, P(sz)], ctypes.c_int),
        "zt_inflate_raw_dict": ([vp, sz, sz, P(InflateOpts), vp, sz, u8pp, P(sz), P(sz)], ctypes.c_int),
        "zt_deflate_raw_batch_dict": ([P(vp), P(sz), sz, P(DeflateOpts), vp, sz, u8pp, P(sz), P(ctypes.c_int)],
                                      ctypes.c_int),
        "zt_inflate_raw_batch_dict": ([P(vp), P(sz), sz, P(InflateOpts), vp, sz, u8pp, P(sz), P(sz),
                                       P(ctypes.c_int)], ctypes.c_int),
        "zt_zlib_compress_dict": ([vp, sz, P(DeflateOpts), vp, sz, u8pp, P(sz), P(u32)], ctypes.c_int),
        "zt_zlib_compress_batch_dict": ([P(vp), P(sz), sz, P(DeflateOpts), vp, sz, u8pp, P(sz), P(ctypes.c_int)],
                                        ctypes.c_int),
        "zt_zlib_decompress_dict": ([vp, sz, sz, ctypes.c_int, vp, sz, u8pp, P(sz), P(sz), P(u32)], ctypes.c_int),
        # include/zt_container_batch.h
        "zt_gunzip_batch": ([P(vp), P(sz), sz, u8pp, P(sz), P(P(GzipMember)), P(sz), P(ctypes.c_int)], ctypes.c_int),
        "zt_zlib_decompress_batch": ([P(vp), P(sz), P(sz), sz, ctypes.c_int, u8pp, P(sz), P(sz), P(u32),
                                      P(ctypes.c_int)], ctypes.c_int),
        "zt_zlib_decompress_batch_dict": ([P(vp), P(sz), P(sz), sz, ctypes.c_int, vp, sz, u8pp, P(sz), P(sz), P(u32),
                                           P(ctypes.c_int)], ctypes.c_int),
        "zt_container_batch_message": ([sz], ctypes.c_char_p),
        "zt_gunzip_batch_last_stats": ([P(GunzipBatchStats)], ctypes.c_int),
        # include/zt_index.h
        "zt_inflate_index_build": ([vp, sz, sz, u8pp, P(sz), u8pp, P(sz), P(sz)], ctypes.c_int),
        "zt_inflate_range": ([vp, sz, vp, sz, ctypes.c_uint64, ctypes.c_uint64, u8pp, P(sz)], ctypes.c_int),
        "zt_inflate_ranges": ([vp, sz, vp, sz, P(ctypes.c_uint64), P(ctypes.c_uint64), sz, u8pp, P(sz),
                               P(ctypes.c_int)], ctypes.c_int),
        "zt_index_stats_read": ([P(IndexStats), ctypes.c_int], ctypes.c_int),
        # include/zt_checkpoint.h
        "zt_inflate_ckpt_build": ([vp, sz, sz, ctypes.c_uint64, u8pp, P(sz), u8pp, P(sz), P(sz)], ctypes.c_int),
        "zt_inflate_ckpt_range": ([vp, sz, vp, sz, ctypes.c_uint64, ctypes.c_uint64, u8pp, P(sz)], ctypes.c_int),
        "zt_inflate_ckpt_ranges": ([vp, sz, vp, sz, P(ctypes.c_uint64), P(ctypes.c_uint64), sz, u8pp, P(sz),
                                    P(ctypes.c_int)], ctypes.c_int),
        "zt_ckpt_stats_read": ([P(CkptStats), ctypes.c_int], ctypes.c_int),
        # include/zt_index.h, the write side
        "zt_deflate_raw_indexed": ([vp, sz, P(DeflateOpts), sz, u8pp, P(sz), u8pp, P(sz)], ctypes.c_int),
        "zt_gzip_compress_indexed": ([vp, sz, P(GzipOpts), u8pp, P(sz), P(u32), u8pp, P(sz)], ctypes.c_int),
        "zt_zlib_compress_indexed": ([vp, sz, P(DeflateOpts), u8pp, P(sz), P(u32), u8pp, P(sz)], ctypes.c_int),
        # include/zt_bgzf.h
        "zt_bgzf_compress": ([vp, sz, P(BgzfOpts), u8pp, P(sz), u8pp, P(sz)], ctypes.c_int),
        "zt_bgzf_index": ([vp, sz, u8pp, P(sz), P(BgzfInfo)], ctypes.c_int),
        "zt_bgzf_decompress": ([vp, sz, u8pp, P(sz), P(BgzfInfo)], ctypes.c_int),
        "zt_bgzf_read_ranges": ([vp, sz, vp, sz, P(ctypes.c_uint64), P(ctypes.c_uint64), sz, u8pp, P(sz),
                                 P(ctypes.c_int)], ctypes.c_int),
        "zt_bgzf_read_virtual": ([vp, sz, P(ctypes.c_uint64), P(ctypes.c_uint64), sz, u8pp, P(sz),
                                  P(ctypes.c_int)], ctypes.c_int),
        "zt_bgzf_stats_read": ([P(BgzfStats), ctypes.c_int], ctypes.c_int),
        # include/zt_dev_batch.h
        "zt_deflate_dev_batch": ([P(vp), P(sz), sz, P(DeflateOpts), ctypes.c_int, P(vp), P(sz), P(sz),
                                  P(ctypes.c_int), vp], ctypes.c_int),
        "zt_deflate_dev_batch_bound": ([sz, ctypes.c_int, ctypes.c_int], sz),
        "zt_inflate_dev_batch": ([P(vp), P(sz), P(sz), sz, P(vp), P(sz), P(sz), P(sz), P(ctypes.c_int), P(u32),
                                  P(u32), vp], ctypes.c_int),
        "zt_debug_dev_batch_times": ([ctypes.c_int, P(ctypes.c_double)], ctypes.c_int),  # debug (dev_batch_api.cpp)
        # include/zt_stream.h
        "zt_inflate_session_create": ([vp, sz, P(vp)], ctypes.c_int),
        "zt_inflate_session_destroy": ([vp], None),
        "zt_inflate_session_feed": ([vp, vp, sz, ctypes.c_int, u8pp, P(sz)], ctypes.c_int),
        "zt_inflate_sessions_feed": ([P(vp), P(vp), P(sz), P(ctypes.c_int), sz, u8pp, P(sz), P(ctypes.c_int)],
                                     ctypes.c_int),
        "zt_inflate_session_get_info": ([vp, P(InflateSessionInfo)], ctypes.c_int),
        "zt_inflate_session_message": ([vp], ctypes.c_char_p),
        # include/zt_stream_container.h
        "zt_container_session_create": ([ctypes.c_int, vp, sz, ctypes.c_int, P(vp)], ctypes.c_int),
        "zt_container_session_destroy": ([vp], None),
        "zt_container_session_feed": ([vp, vp, sz, ctypes.c_int, u8pp, P(sz)], ctypes.c_int),
        "zt_container_sessions_feed": ([P(vp), P(vp), P(sz), P(ctypes.c_int), sz, u8pp, P(sz), P(ctypes.c_int)],
                                       ctypes.c_int),
        "zt_container_session_get_info": ([vp, P(ContainerSessionInfo)], ctypes.c_int),
        "zt_container_session_member": ([vp, sz, P(ContainerMember)], ctypes.c_int),
        "zt_container_session_message": ([vp], ctypes.c_char_p),
        # include/zt_strategy.h
        "zt_deflate_raw_strategy": ([vp, sz, P(DeflateOpts), ctypes.c_int, u8pp, P(sz)], ctypes.c_int),
        "zt_deflate_raw_batch_strategy": ([P(vp), P(sz), sz, P(DeflateOpts), ctypes.c_int, u8pp, P(sz),
                                          P(ctypes.c_int)], ctypes.c_int),
        "zt_zlib_compress_strategy": ([vp, sz, P(DeflateOpts), ctypes.c_int, u8pp, P(sz), P(u32)], ctypes.c_int),
        "zt_gzip_compress_strategy": ([vp, sz, P(GzipOpts), ctypes.c_int, u8pp, P(sz), P(u32)], ctypes.c_int),
        "zt_zlib_compress_batch_strategy": ([P(vp), P(sz), sz, P(DeflateOpts), ctypes.c_int, u8pp, P(sz),
                                            P(ctypes.c_int)], ctypes.c_int),
        "zt_gzip_compress_batch_strategy": ([P(vp), P(sz), sz, P(GzipOpts), ctypes.c_int, u8pp, P(sz),
                                            P(ctypes.c_int)], ctypes.c_int),
        "zt_deflate_plan_set_strategy": ([vp, ctypes.c_int], ctypes.c_int),
        "zt_debug_match_strategy": ([vp, sz, sz, ctypes.c_int, ctypes.c_int, vp, vp, vp], ctypes.c_int),  # debug
    }
    for name, (args, res) in sig.items():
        f = getattr(lib, name, None)
        if f is None:  # reported by tests/test_abi.py
            continue
        f.argtypes = args
        f.restype = res
    return lib


lib = _load()

# every symbol include/zt.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "zt_device_count", "zt_set_device", "zt_set_devices", "zt_last_error_message", "zt_version", "zt_free", "zt_crc32_update",
    "zt_adler32_update", "zt_checksums", "zt_deflate_raw", "zt_inflate_raw", "zt_inflate_raw_resume", "zt_inflate_raw_resume_final",
    "zt_inflate_raw_batch",
    "zt_deflate_raw_batch", "zt_gzip_compress", "zt_gzip_compress_batch", "zt_zlib_compress_batch", "zt_gunzip",
    "zt_crc32_batch", "zt_zip_compress", "zt_unzip", "zt_zlib_compress", "zt_zlib_decompress",
    "zt_dev_checksums", "zt_deflate_plan_create", "zt_deflate_plan_destroy",
    "zt_deflate_bound", "zt_deflate_dev", "zt_inflate_plan_create", "zt_inflate_plan_destroy", "zt_inflate_dev",
    "zt_synth_dev", "zt_synth_dev_at", "zt_timing_enable", "zt_timing_read", "zt_scratch_bytes",
    "zt_release_scratch",
]

# every symbol include/zt_zipcrypto.h declares (checked by tests/test_zipcrypto_ref.py)
ZIPCRYPTO_SYMBOLS = [
    "zt_zipcrypto_encrypt_batch", "zt_zipcrypto_decrypt_batch", "zt_zipcrypto_tile_bytes",
    "zt_zipcrypto_chunk_bytes", "zt_zipcrypto_last_kernel_ms", "zt_zip_compress_pw", "zt_unzip_pw",
]

# every symbol include/zt_dict.h declares (checked by tests/test_dict_host.py)
DICT_SYMBOLS = [
    "zt_deflate_raw_dict", "zt_inflate_raw_dict", "zt_deflate_raw_batch_dict", "zt_inflate_raw_batch_dict",
    "zt_zlib_compress_dict", "zt_zlib_compress_batch_dict", "zt_zlib_decompress_dict",
]


# every symbol include/zt_container_batch.h declares (checked by tests/test_container_batch_host.py)
CONTAINER_BATCH_SYMBOLS = [
    "zt_gunzip_batch", "zt_zlib_decompress_batch", "zt_zlib_decompress_batch_dict", "zt_container_batch_message",
    "zt_gunzip_batch_last_stats",
]


# every symbol include/zt_index.h declares (checked by tests/test_index_host.py)
INDEX_SYMBOLS = [
    "zt_inflate_index_build", "zt_inflate_range", "zt_inflate_ranges", "zt_index_stats_read",
]


# the write side of include/zt_index.h (checked by tests/test_deflate_index_host.py)
DEFLATE_INDEX_SYMBOLS = [
    "zt_deflate_raw_indexed", "zt_gzip_compress_indexed", "zt_zlib_compress_indexed",
]


# every symbol include/zt_checkpoint.h declares (checked by tests/test_ckpt_host.py)
CKPT_SYMBOLS = [
    "zt_inflate_ckpt_build", "zt_inflate_ckpt_range", "zt_inflate_ckpt_ranges", "zt_ckpt_stats_read",
]


# every symbol include/zt_bgzf.h declares (checked by tests/test_bgzf_host.py)
BGZF_SYMBOLS = [
    "zt_bgzf_compress", "zt_bgzf_index", "zt_bgzf_decompress", "zt_bgzf_read_ranges", "zt_bgzf_read_virtual",
    "zt_bgzf_stats_read",
]


# every symbol include/zt_dev_batch.h declares (checked by tests/test_dev_batch_host.py)
DEV_BATCH_SYMBOLS = [
    "zt_deflate_dev_batch", "zt_deflate_dev_batch_bound", "zt_inflate_dev_batch",
]


# every symbol include/zt_stream.h declares (checked by tests/test_stream_host.py)
STREAM_SYMBOLS = [
    "zt_inflate_session_create", "zt_inflate_session_destroy", "zt_inflate_session_feed",
    "zt_inflate_sessions_feed", "zt_inflate_session_get_info", "zt_inflate_session_message",
]


# every symbol include/zt_stream_container.h declares (checked by tests/test_container_stream_host.py)
CONTAINER_STREAM_SYMBOLS = [
    "zt_container_session_create", "zt_container_session_destroy", "zt_container_session_feed",
    "zt_container_sessions_feed", "zt_container_session_get_info", "zt_container_session_member",
    "zt_container_session_message",
]
SESSION_AUTO, SESSION_GZIP, SESSION_ZLIB = 0, 1, 2


# every symbol include/zt_strategy.h declares (checked by tests/test_strategy_ref.py)
STRATEGY_SYMBOLS = [
    "zt_deflate_raw_strategy", "zt_deflate_raw_batch_strategy", "zt_zlib_compress_strategy",
    "zt_gzip_compress_strategy", "zt_zlib_compress_batch_strategy", "zt_gzip_compress_batch_strategy",
    "zt_deflate_plan_set_strategy",
]
# zlib's numbers; strategy=None in the calls below is the plain entry point
STRATEGY_DEFAULT, STRATEGY_HUFFMAN_ONLY, STRATEGY_RLE = 0, 2, 3


def _no_dictionary(strategy, dictionary):
    if strategy is not None and dictionary is not None:
        raise ValueError("a strategy cannot be combined with a dictionary")


def _check(rc):
    if rc != ZT_OK:
        raise ZtError(rc, lib.zt_last_error_message().decode(errors="replace"))


def _cbuf(data):
    data = bytes(data)
    return ctypes.create_string_buffer(data, len(data) or 1), len(data)


def device_count():
    return lib.zt_device_count()


def set_devices(mask):
    """Devices the batch calls split over (bit d = device d; 0 = this thread's)."""
    _check(lib.zt_set_devices(mask))


def set_device(d):
    _check(lib.zt_set_device(d))


def crc32(data, crc=0):
    b, n = _cbuf(data)
    out = ctypes.c_uint32()
    _check(lib.zt_crc32_update(crc, b, n, ctypes.byref(out)))
    return out.value


def adler32(data, adler=1):
    b, n = _cbuf(data)
    out = ctypes.c_uint32()
    _check(lib.zt_adler32_update(adler, b, n, ctypes.byref(out)))
    return out.value


def checksums(data, crc=0, adler=1):
    b, n = _cbuf(data)
    c, a = ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib.zt_checksums(b, n, crc, adler, ctypes.byref(c), ctypes.byref(a)))
    return c.value, a.value


def deflate_raw(data, compression_type=2, lazy=0, level=-1, dictionary=None, strategy=None):
    """dictionary: preset dictionary (zlib's zdict), include/zt_dict.h.
    strategy: STRATEGY_RLE / STRATEGY_HUFFMAN_ONLY (include/zt_strategy.h)."""
    _no_dictionary(strategy, dictionary)
    b, n = _cbuf(data)
    opts = DeflateOpts(compression_type, lazy, level)
    out = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    if strategy is not None:
        _check(lib.zt_deflate_raw_strategy(b, n, ctypes.byref(opts), strategy, ctypes.byref(out), ctypes.byref(olen)))
    elif dictionary is not None:
        d, dn = _cbuf(dictionary)
        _check(lib.zt_deflate_raw_dict(b, n, ctypes.byref(opts), d, dn, ctypes.byref(out), ctypes.byref(olen)))
    else:
        _check(lib.zt_deflate_raw(b, n, ctypes.byref(opts), ctypes.byref(out), ctypes.byref(olen)))
    res = ctypes.string_at(out, olen.value)
    lib.zt_free(out)
    return res


def inflate_raw(data, index=0, ref_strict=False, buffer_type=1, buffer_size=0x8000, dictionary=None):
    """Returns (output bytes, end ip)."""
    b, n = _cbuf(data)
    opts = InflateOpts(buffer_type, buffer_size, 1 if ref_strict else 0)
    out = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    ip = ctypes.c_size_t()
    if dictionary is not None:
        d, dn = _cbuf(dictionary)
        _check(lib.zt_inflate_raw_dict(b, n, index, ctypes.byref(opts), d, dn, ctypes.byref(out),
                                       ctypes.byref(olen), ctypes.byref(ip)))
    else:
        _check(lib.zt_inflate_raw(b, n, index, ctypes.byref(opts), ctypes.byref(out), ctypes.byref(olen),
                                  ctypes.byref(ip)))
    res = ctypes.string_at(out, olen.value)
    lib.zt_free(out)
    return res, ip.value


def inflate_raw_resume(data, bit_pos=0, window=b"", final=False):
    """zt_inflate_raw_resume (final: zt_inflate_raw_resume_final -- no more
    input will come, errors are the stream's own): (output of the complete
    blocks, end bit, finished)."""
    b, n = _cbuf(data)
    w, wn = _cbuf(window)
    out = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    end = ctypes.c_uint64()
    fin = ctypes.c_int()
    fn = lib.zt_inflate_raw_resume_final if final else lib.zt_inflate_raw_resume
    _check(fn(b, n, bit_pos, w, wn, ctypes.byref(out), ctypes.byref(olen), ctypes.byref(end), ctypes.byref(fin)))
    res = ctypes.string_at(out, olen.value) if out else b""
    if out:
        lib.zt_free(out)
    return res, end.value, bool(fin.value)


class RawInflateStream:
    """The reference's streaming decoder surface (src/RawInflateStream.ts:
    52-120): ``decompress(new_input, ip)`` decodes what the input holds so far
    and returns the bytes produced by this call.  State between calls: the
    input position (byte ``ip`` and the bits of it already used), the last 32
    KiB of output (match history) and whether the final block was seen."""

    def __init__(self, data=b"", ip=0):
        self.input = bytes(data)
        self.ip = ip
        self.bit = 0
        self.window = b""
        self.bfinal = False
        self.total = 0

    def decompress(self, new_input=None, ip=None):
        return self._run(new_input, ip, False)

    def finish(self, new_input=None, ip=None):
        """The input is complete: decode what is left; a stream corrupt near
        its end, or one that ends before its final block, raises ZtError."""
        out = self._run(new_input, ip, True)
        if not self.bfinal:
            raise ZtError(-10, "input buffer is broken")
        return out

    def _run(self, new_input, ip, final):
        if new_input is not None:
            self.input = bytes(new_input)
        if ip is not None:  # (a re-based buffer: the bits of its byte `ip` already used stay used)
            self.ip = ip
        if self.bfinal or (self.ip >= len(self.input) and not final):
            return b""
        out, end, fin = inflate_raw_resume(self.input, self.ip * 8 + self.bit, self.window, final)
        self.ip, self.bit = end >> 3, end & 7
        self.bfinal = fin
        self.total += len(out)
        self.window = (self.window + out)[-32768:]
        return out


class InflateSession:
    """An inflate session (include/zt_stream.h): raw inflate fed piece by
    piece, only the new bytes each time, resumed at a token; its state stays
    on the device.  ``feed(data, last)`` returns the bytes this piece
    completes; ``window`` is a preset dictionary."""

    def __init__(self, window=b""):
        self._h = ctypes.c_void_p()
        w, wn = _cbuf(window)
        _check(lib.zt_inflate_session_create(w, wn, ctypes.byref(self._h)))

    def feed(self, data, last=False):
        b, n = _cbuf(data)
        out = ctypes.POINTER(ctypes.c_uint8)()
        olen = ctypes.c_size_t()
        _check(lib.zt_inflate_session_feed(self._handle(), b, n, int(bool(last)), ctypes.byref(out),
                                           ctypes.byref(olen)))
        return _take(out, olen) if out else b""

    def _handle(self):
        if not self._h:
            raise ValueError("the session is closed")
        return self._h

    def info(self):
        i = InflateSessionInfo()
        _check(lib.zt_inflate_session_get_info(self._handle(), ctypes.byref(i)))
        d = {k: getattr(i, k) for k, _ in InflateSessionInfo._fields_}
        d["message"] = lib.zt_inflate_session_message(self._h).decode(errors="replace")
        return d

    @property
    def finished(self):
        return bool(self.info()["finished"])

    @property
    def unused(self):
        """Fed bytes behind the stream's end (a container's trailer)."""
        i = self.info()
        return i["total_in"] - (i["end_bits"] + 7) // 8

    @property
    def crc32(self):
        return self.info()["crc32"]

    @property
    def adler32(self):
        return self.info()["adler32"]

    def close(self):
        if self._h:
            lib.zt_inflate_session_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def inflate_sessions_feed(sessions, chunks, last=False, return_code=False):
    """zt_inflate_sessions_feed: chunk i fed to session i, all in one call
    (one wavefront per session).  last: one flag, or one per session.
    Returns a list of (status, output): status a BatchStatus (0, or the
    session's sticky error with its message); a failed item has output b"".
    return_code: also the call's return code, as (code, list)."""
    k = len(sessions)
    bs, ptrs, lens = _batch_ptrs(chunks)
    if len(bs) != k:
        raise ValueError("one chunk per session")
    hs = (ctypes.c_void_p * k)(*[x._handle().value for x in sessions])
    flags = list(last) if isinstance(last, (list, tuple)) else [last] * k
    fl = (ctypes.c_int * k)(*[int(bool(f)) for f in flags])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    st = (ctypes.c_int * k)()
    rc = lib.zt_inflate_sessions_feed(hs, ptrs, lens, fl, k, outs, olens, st)
    if rc != ZT_OK and all(x == 0 for x in st):
        _check(rc)
    data = _batch_take(k, outs, olens)
    res = [(BatchStatus(st[i], lib.zt_inflate_session_message(hs[i]).decode(errors="replace") if st[i] else ""),
            data[i] if st[i] == 0 else b"") for i in range(k)]
    return (rc, res) if return_code else res


class _ContainerSession:
    """A container session (include/zt_stream_container.h): a gzip file or a
    zlib stream fed piece by piece, only the new bytes each time; the bodies
    are decoded by the inflate sessions' kernel.  ``feed(data, last)`` returns
    the bytes this piece completes; when it fails, the ZtError's ``output``
    holds the bytes the call decoded before the error."""

    def __init__(self, fmt, dictionary=None, verify=True):
        self._h = ctypes.c_void_p()
        d, dn = _cbuf(dictionary if dictionary is not None else b"")
        _check(lib.zt_container_session_create(fmt, d if dn else None, dn, int(bool(verify)), ctypes.byref(self._h)))

    def _handle(self):
        if not self._h:
            raise ValueError("the session is closed")
        return self._h

    def feed(self, data, last=False):
        b, n = _cbuf(data)
        out = ctypes.POINTER(ctypes.c_uint8)()
        olen = ctypes.c_size_t()
        rc = lib.zt_container_session_feed(self._handle(), b, n, int(bool(last)), ctypes.byref(out),
                                           ctypes.byref(olen))
        res = _take(out, olen) if out else b""
        if rc != ZT_OK:
            e = ZtError(rc, lib.zt_last_error_message().decode(errors="replace"))
            e.output = res
            raise e
        return res

    def info(self):
        i = ContainerSessionInfo()
        _check(lib.zt_container_session_get_info(self._handle(), ctypes.byref(i)))
        d = {k: getattr(i, k) for k, _ in ContainerSessionInfo._fields_}
        d["message"] = lib.zt_container_session_message(self._h).decode(errors="replace")
        return d

    def members(self):
        """The members whose trailer was checked, as gunzip() gives them (no
        ``data``: the bytes went out with the feeds; ``data_off`` / ``data_len``
        place them in the total output, ``in_off`` the member in the input)."""
        res = []
        for k in range(self.info()["members_done"]):
            m = ContainerMember()
            _check(lib.zt_container_session_member(self._handle(), k, ctypes.byref(m)))
            d = {f: getattr(m, f) for f, _ in ContainerMember._fields_ if f not in ("pad", "name", "comment")}
            d["name"] = ctypes.string_at(m.name, m.name_len) if m.flg & 0x08 else None
            d["comment"] = ctypes.string_at(m.comment, m.comment_len) if m.flg & 0x10 else None
            res.append(d)
        return res

    @property
    def finished(self):
        return bool(self.info()["finished"])

    @property
    def unused(self):
        """zlib: fed bytes behind the Adler-32."""
        return self.info()["unused"]

    def close(self):
        if self._h:
            lib.zt_container_session_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GunzipSession(_ContainerSession):
    """Streaming gunzip of one gzip file, any number of members."""

    def __init__(self, verify=True, auto=False):
        super().__init__(SESSION_AUTO if auto else SESSION_GZIP, None, verify)


class ZlibInflateSession(_ContainerSession):
    """Streaming inflate of one zlib stream; dictionary: used when it carries FDICT."""

    def __init__(self, dictionary=None, verify=True, auto=False):
        super().__init__(SESSION_AUTO if auto else SESSION_ZLIB, dictionary, verify)


def container_sessions_feed(sessions, chunks, last=False, return_code=False):
    """zt_container_sessions_feed: chunk i fed to container session i, all in
    one call.  last: one flag, or one per session.  Returns a list of (status,
    output): status a BatchStatus (0, or the session's sticky error with its
    message); a failed item's output is what the call decoded before the
    error.  return_code: also the call's return code, as (code, list)."""
    k = len(sessions)
    bs, ptrs, lens = _batch_ptrs(chunks)
    if len(bs) != k:
        raise ValueError("one chunk per session")
    hs = (ctypes.c_void_p * k)(*[x._handle().value for x in sessions])
    flags = list(last) if isinstance(last, (list, tuple)) else [last] * k
    fl = (ctypes.c_int * k)(*[int(bool(f)) for f in flags])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    st = (ctypes.c_int * k)()
    rc = lib.zt_container_sessions_feed(hs, ptrs, lens, fl, k, outs, olens, st)
    if rc != ZT_OK and all(x == 0 for x in st):
        _check(rc)
    data = _batch_take(k, outs, olens)
    res = [(BatchStatus(st[i], lib.zt_container_session_message(hs[i]).decode(errors="replace") if st[i] else ""),
            data[i]) for i in range(k)]
    return (rc, res) if return_code else res


def inflate_raw_batch(streams, ref_strict=False, dictionary=None):
    """Returns a list of (status, output bytes, end ip)."""
    k = len(streams)
    # the bytes objects' own buffers are passed (no copy); `bs` keeps them alive
    bs = [bytes(x) for x in streams]
    ptrs = (ctypes.c_void_p * k)(*[ctypes.cast(ctypes.c_char_p(x), ctypes.c_void_p).value for x in bs])
    lens = (ctypes.c_size_t * k)(*[len(x) for x in bs])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    ips = (ctypes.c_size_t * k)()
    st = (ctypes.c_int * k)()
    opts = InflateOpts(1, 0x8000, 1 if ref_strict else 0)
    if dictionary is not None:
        d, dn = _cbuf(dictionary)
        rc = lib.zt_inflate_raw_batch_dict(ptrs, lens, k, ctypes.byref(opts), d, dn, outs, olens, ips, st)
    else:
        rc = lib.zt_inflate_raw_batch(ptrs, lens, k, ctypes.byref(opts), outs, olens, ips, st)
    if rc != ZT_OK and all(s == 0 for s in st):
        _check(rc)
    res = []
    for i in range(k):
        data = ctypes.string_at(outs[i], olens[i]) if st[i] == 0 and outs[i] else b""
        if outs[i]:
            lib.zt_free(outs[i])
        res.append((st[i], data, ips[i]))
    return res


def deflate_raw_batch(items, compression_type=2, level=-1, dictionary=None, strategy=None):
    _no_dictionary(strategy, dictionary)
    k = len(items)
    bufs = [_cbuf(s) for s in items]
    ptrs = (ctypes.c_void_p * k)(*[ctypes.addressof(b) for b, _ in bufs])
    lens = (ctypes.c_size_t * k)(*[n for _, n in bufs])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    st = (ctypes.c_int * k)()
    opts = DeflateOpts(compression_type, 0, level)
    if strategy is not None:
        rc = lib.zt_deflate_raw_batch_strategy(ptrs, lens, k, ctypes.byref(opts), strategy, outs, olens, st)
    elif dictionary is not None:
        d, dn = _cbuf(dictionary)
        rc = lib.zt_deflate_raw_batch_dict(ptrs, lens, k, ctypes.byref(opts), d, dn, outs, olens, st)
    else:
        rc = lib.zt_deflate_raw_batch(ptrs, lens, k, ctypes.byref(opts), outs, olens, st)
    _check(rc)
    res = []
    for i in range(k):
        res.append(ctypes.string_at(outs[i], olens[i]))
        lib.zt_free(outs[i])
    return res


def _take(out, olen):
    res = ctypes.string_at(out, olen.value)
    lib.zt_free(out)
    return res


def gzip_compress(data, name=None, comment=None, hcrc=False, mtime=0, compression_type=2, lazy=0, level=-1,
                  strategy=None):
    """GZip.compress (src/GZip.ts:96-194); name/comment are header bytes.
    Returns (member bytes, crc32)."""
    b, n = _cbuf(data)
    o = GzipOpts()
    o.deflate = DeflateOpts(compression_type, lazy, level)
    o.fname, o.fcomment, o.fhcrc, o.mtime = int(name is not None), int(comment is not None), int(hcrc), mtime
    if name is not None:
        o.name, o.name_len = bytes(name), len(name)
    if comment is not None:
        o.comment, o.comment_len = bytes(comment), len(comment)
    out = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    crc = ctypes.c_uint32()
    if strategy is not None:
        _check(lib.zt_gzip_compress_strategy(b, n, ctypes.byref(o), strategy, ctypes.byref(out), ctypes.byref(olen),
                                             ctypes.byref(crc)))
    else:
        _check(lib.zt_gzip_compress(b, n, ctypes.byref(o), ctypes.byref(out), ctypes.byref(olen), ctypes.byref(crc)))
    return _take(out, olen), crc.value


def _batch_ptrs(items):
    bs = [bytes(x) for x in items]
    k = len(bs)
    ptrs = (ctypes.c_void_p * k)(*[ctypes.cast(ctypes.c_char_p(x), ctypes.c_void_p).value for x in bs])
    lens = (ctypes.c_size_t * k)(*[len(x) for x in bs])
    return bs, ptrs, lens


def _batch_take(k, outs, olens):
    res = []
    for i in range(k):
        res.append(ctypes.string_at(outs[i], olens[i]) if outs[i] else b"")
        if outs[i]:
            lib.zt_free(outs[i])
    return res


def gzip_compress_batch(items, name=None, comment=None, hcrc=False, mtime=0, compression_type=2, lazy=0, level=-1,
                        strategy=None):
    """GZip members of many buffers in one pipeline per device (config C4)."""
    bs, ptrs, lens = _batch_ptrs(items)
    k = len(bs)
    o = GzipOpts()
    o.deflate = DeflateOpts(compression_type, lazy, level)
    o.fname, o.fcomment, o.fhcrc, o.mtime = int(name is not None), int(comment is not None), int(hcrc), mtime
    if name is not None:
        o.name, o.name_len = bytes(name), len(name)
    if comment is not None:
        o.comment, o.comment_len = bytes(comment), len(comment)
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    st = (ctypes.c_int * k)()
    if strategy is not None:
        _check(lib.zt_gzip_compress_batch_strategy(ptrs, lens, k, ctypes.byref(o), strategy, outs, olens, st))
    else:
        _check(lib.zt_gzip_compress_batch(ptrs, lens, k, ctypes.byref(o), outs, olens, st))
    return _batch_take(k, outs, olens)


def zlib_compress_batch(items, compression_type=2, lazy=0, level=-1, dictionary=None, strategy=None):
    _no_dictionary(strategy, dictionary)
    bs, ptrs, lens = _batch_ptrs(items)
    k = len(bs)
    opts = DeflateOpts(compression_type, lazy, level)
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    st = (ctypes.c_int * k)()
    if strategy is not None:
        _check(lib.zt_zlib_compress_batch_strategy(ptrs, lens, k, ctypes.byref(opts), strategy, outs, olens, st))
    elif dictionary is not None:
        d, dn = _cbuf(dictionary)
        _check(lib.zt_zlib_compress_batch_dict(ptrs, lens, k, ctypes.byref(opts), d, dn, outs, olens, st))
    else:
        _check(lib.zt_zlib_compress_batch(ptrs, lens, k, ctypes.byref(opts), outs, olens, st))
    return _batch_take(k, outs, olens)


def crc32_batch(items):
    bs, ptrs, lens = _batch_ptrs(items)
    out = (ctypes.c_uint32 * len(bs))()
    _check(lib.zt_crc32_batch(ptrs, lens, len(bs), out))
    return list(out)


def dos_mtime(year, month, day, hour, minute, second):
    """The 4 DOS time / date bytes of src/Zip.ts:130-139 (month 1-12)."""
    return bytes([((minute & 7) << 5) | (second >> 1), ((hour << 3) | (minute >> 3)) & 0xFF,
                  ((month & 7) << 5) | day, (((year - 1980) & 0x7F) << 1) | (month >> 3)])


CRYPT_HEADERS = {"reference": 0, "pkware": 1}


def _pw_bytes(pw):
    """A password as bytes (a str as stringToByteArray does: charCode & 0xFF)."""
    return bytes(ord(ch) & 0xFF for ch in pw) if isinstance(pw, str) else bytes(pw)


def zip_compress(files, comment=b"", pw_call=False):
    """Zip.addFile(...) for each dict of `files` (data, name, comment, method,
    os, mtime = 4 DOS bytes, compression_type, lazy) then Zip.compress().
    A file with `password` (bytes or str) is encrypted with ZipCrypto:
    `crypt_header` 'reference' (default: header bytes as src/Zip.ts writes
    them) or 'pkware' (as other tools check them), `crypt_lead` = the 10
    leading header bytes (default zeros; the library draws no randomness).
    pw_call: go through zt_zip_compress_pw even when no file has a password
    (crypt = NULL)."""
    k = len(files)
    datas = [bytes(f["data"]) for f in files]
    bs, ptrs, lens = _batch_ptrs(datas)
    arr = (ZipFile * k)()
    keep = []
    for i, f in enumerate(files):
        nm, cm = bytes(f.get("name", b"")), f.get("comment")
        keep += [nm, cm]
        arr[i].name, arr[i].name_len = nm, len(nm)
        if cm is not None:
            arr[i].comment, arr[i].comment_len = bytes(cm), len(cm)
        arr[i].method = f.get("method", 8)
        arr[i].os = f.get("os", 0)
        arr[i].mtime = (ctypes.c_uint8 * 4)(*f.get("mtime", b"\0\0\0\0"))
        arr[i].deflate = DeflateOpts(f.get("compression_type", 2), f.get("lazy", 0), f.get("level", -1))
    out = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    cb = bytes(comment)
    if any(f.get("password") is not None for f in files):
        cr = (ZipCrypt * k)()
        for i, f in enumerate(files):
            if f.get("password") is None:
                continue
            pw = _pw_bytes(f["password"])
            keep.append(pw)
            cr[i].password, cr[i].password_len = pw, len(pw)
            cr[i].header_mode = CRYPT_HEADERS[f.get("crypt_header", "reference")]
            lead = bytes(f.get("crypt_lead", bytes(10)))
            if len(lead) != 10:
                raise ValueError("crypt_lead must be 10 bytes")
            cr[i].lead = (ctypes.c_uint8 * 10)(*lead)
        _check(lib.zt_zip_compress_pw(ptrs, lens, arr, cr, k, cb, len(cb), ctypes.byref(out), ctypes.byref(olen)))
    elif pw_call:
        _check(lib.zt_zip_compress_pw(ptrs, lens, arr, None, k, cb, len(cb), ctypes.byref(out), ctypes.byref(olen)))
    else:
        _check(lib.zt_zip_compress(ptrs, lens, arr, k, cb, len(cb), ctypes.byref(out), ctypes.byref(olen)))
    return _take(out, olen)


def _zipcrypto_batch(fn, items, passwords):
    bs, ptrs, lens = _batch_ptrs(items)
    k = len(bs)
    if not isinstance(passwords, (list, tuple)):
        passwords = [passwords] * k
    pws, pptrs, plens = _batch_ptrs([_pw_bytes(p) for p in passwords])
    if len(pws) != k:
        raise ValueError("one password per item")
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    _check(fn(ptrs, lens, k, pptrs, plens, outs))
    return _batch_take(k, outs, lens)


def zipcrypto_encrypt(items, passwords):
    """Raw ZipCrypto streams (no container) of `items` under `passwords` (one
    for all, or one per item)."""
    return _zipcrypto_batch(lib.zt_zipcrypto_encrypt_batch, items, passwords)


def zipcrypto_decrypt(items, passwords):
    return _zipcrypto_batch(lib.zt_zipcrypto_decrypt_batch, items, passwords)


def zipcrypto_geometry():
    """(tile bytes T, chunk bytes C) of the encrypt kernels."""
    return lib.zt_zipcrypto_tile_bytes(), lib.zt_zipcrypto_chunk_bytes()


def zipcrypto_last_kernel_ms():
    ms = ctypes.c_double()
    _check(lib.zt_zipcrypto_last_kernel_ms(ctypes.byref(ms)))
    return ms.value


def unzip(archive, verify=False, password=None, pw_call=False):
    """Unzip every entry.  Returns (first error or None, [entry dicts with
    name, comment, data (or None), status, message and the header fields]).
    `password` (bytes or str) decrypts the archive's ZipCrypto entries
    (pw_call: zt_unzip_pw even without one, password = NULL)."""
    b, n = _cbuf(archive)
    archive = bytes(archive)
    out = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    ents = ctypes.POINTER(UnzipEntry)()
    cnt = ctypes.c_size_t()
    if password is None and pw_call:
        rc = lib.zt_unzip_pw(b, n, int(verify), None, 0, ctypes.byref(out), ctypes.byref(olen), ctypes.byref(ents),
                             ctypes.byref(cnt))
    elif password is None:
        rc = lib.zt_unzip(b, n, int(verify), ctypes.byref(out), ctypes.byref(olen), ctypes.byref(ents),
                          ctypes.byref(cnt))
    else:
        pw, pn = _cbuf(_pw_bytes(password))
        rc = lib.zt_unzip_pw(b, n, int(verify), pw, pn, ctypes.byref(out), ctypes.byref(olen), ctypes.byref(ents),
                             ctypes.byref(cnt))
    if rc != ZT_OK and not ents:
        return ZtError(rc, lib.zt_last_error_message().decode(errors="replace")), []
    data = ctypes.string_at(out, olen.value) if out else b""
    res = []
    for i in range(cnt.value):
        e = ents[i]
        d = {f: getattr(e, f) for f, _ in UnzipEntry._fields_ if f != "message"}
        d["message"] = e.message.decode(errors="replace")
        d["name"] = archive[e.name_off:e.name_off + e.name_len]
        d["comment"] = archive[e.comment_off:e.comment_off + e.comment_len]
        d["data"] = data[e.data_off:e.data_off + e.data_len] if e.status == 0 else None
        res.append(d)
    if out:
        lib.zt_free(out)
    if ents:
        lib.zt_free(ents)
    err = None if rc == ZT_OK else ZtError(rc, lib.zt_last_error_message().decode(errors="replace"))
    return err, res


def gunzip(data):
    """GUnzip.decompress + getMembers (src/GUnzip.ts:43-175).  Returns
    (output, [member dicts])."""
    b, n = _cbuf(data)
    raw = bytes(data)
    out = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    mem = ctypes.POINTER(GzipMember)()
    cnt = ctypes.c_size_t()
    _check(lib.zt_gunzip(b, n, ctypes.byref(out), ctypes.byref(olen), ctypes.byref(mem), ctypes.byref(cnt)))
    res = _take(out, olen)
    members = []
    for i in range(cnt.value):
        m = mem[i]
        d = {k: getattr(m, k) for k, _ in GzipMember._fields_}
        d["name"] = raw[m.name_off:m.name_off + m.name_len] if m.flg & 0x08 else None
        d["comment"] = raw[m.comment_off:m.comment_off + m.comment_len] if m.flg & 0x10 else None
        d["data"] = res[m.data_off:m.data_off + m.data_len]
        members.append(d)
    lib.zt_free(mem)
    return res, members


def zlib_compress(data, compression_type=2, lazy=0, level=-1, dictionary=None, strategy=None):
    """Deflate.compress (src/Deflate.ts:60-99).  Returns (stream, adler32).
    dictionary: the stream carries FDICT and the dictionary's Adler-32."""
    _no_dictionary(strategy, dictionary)
    b, n = _cbuf(data)
    o = DeflateOpts(compression_type, lazy, level)
    out = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    adler = ctypes.c_uint32()
    if strategy is not None:
        _check(lib.zt_zlib_compress_strategy(b, n, ctypes.byref(o), strategy, ctypes.byref(out), ctypes.byref(olen),
                                             ctypes.byref(adler)))
    elif dictionary is not None:
        d, dn = _cbuf(dictionary)
        _check(lib.zt_zlib_compress_dict(b, n, ctypes.byref(o), d, dn, ctypes.byref(out), ctypes.byref(olen),
                                         ctypes.byref(adler)))
    else:
        _check(lib.zt_zlib_compress(b, n, ctypes.byref(o), ctypes.byref(out), ctypes.byref(olen),
                                    ctypes.byref(adler)))
    return _take(out, olen), adler.value


def zlib_decompress(data, index=0, verify=False, dictionary=None):
    """Inflate.decompress (src/Inflate.ts:34-93).  Returns (output, ip).
    dictionary: used when the stream carries FDICT (ignored otherwise)."""
    b, n = _cbuf(data)
    out = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    ip = ctypes.c_size_t()
    adler = ctypes.c_uint32()
    if dictionary is not None:
        d, dn = _cbuf(dictionary)
        _check(lib.zt_zlib_decompress_dict(b, n, index, int(verify), d, dn, ctypes.byref(out), ctypes.byref(olen),
                                           ctypes.byref(ip), ctypes.byref(adler)))
    else:
        _check(lib.zt_zlib_decompress(b, n, index, int(verify), ctypes.byref(out), ctypes.byref(olen),
                                      ctypes.byref(ip), ctypes.byref(adler)))
    return _take(out, olen), ip.value


# ---- indexed random access (include/zt_index.h) ------------------------------------
def inflate_index_build(stream, index=0, want_output=False):
    """zt_inflate_index_build: decodes the raw stream at stream[index:] once
    and returns its index blob (bytes); want_output: (blob, output, end ip)."""
    b, n = _cbuf(stream)
    idx = ctypes.POINTER(ctypes.c_uint8)()
    ilen = ctypes.c_size_t()
    olen = ctypes.c_size_t()
    ip = ctypes.c_size_t()
    if want_output:
        out = ctypes.POINTER(ctypes.c_uint8)()
        _check(lib.zt_inflate_index_build(b, n, index, ctypes.byref(idx), ctypes.byref(ilen), ctypes.byref(out),
                                          ctypes.byref(olen), ctypes.byref(ip)))
        return _take(idx, ilen), _take(out, olen), ip.value
    _check(lib.zt_inflate_index_build(b, n, index, ctypes.byref(idx), ctypes.byref(ilen), None, ctypes.byref(olen),
                                      ctypes.byref(ip)))
    return _take(idx, ilen)


def inflate_range(stream, idx, off, length):
    """zt_inflate_range: bytes [off, off + length) of the stream's output (pread
    semantics: length is clamped, off past the end raises ZT_E_ARG)."""
    b, n = _cbuf(stream)
    ib, il = _cbuf(idx)
    out = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    _check(lib.zt_inflate_range(b, n, ib, il, off, length, ctypes.byref(out), ctypes.byref(olen)))
    return _take(out, olen)


def inflate_ranges(stream, idx, ranges, return_code=False):
    """zt_inflate_ranges: [(off, len), ...] in one call.  Returns a list of
    (status, bytes) pairs (bytes None for a failed range); return_code: also
    the call's return code, as (code, list).  A call that fails before any
    range is looked at (a bad index) raises."""
    b, n = _cbuf(stream)
    ib, il = _cbuf(idx)
    k = len(ranges)
    offs = (ctypes.c_uint64 * k)(*[r[0] for r in ranges])
    lens = (ctypes.c_uint64 * k)(*[r[1] for r in ranges])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    st = (ctypes.c_int * k)()
    rc = lib.zt_inflate_ranges(b, n, ib, il, offs, lens, k, outs, olens, st)
    if rc != ZT_OK and all(s == 0 for s in st):
        _check(rc)
    res = []
    for i in range(k):
        res.append((st[i], ctypes.string_at(outs[i], olens[i]) if st[i] == 0 else None))
        if outs[i]:
            lib.zt_free(outs[i])
    return (rc, res) if return_code else res


def _take_pair(out, olen, idx, ilen):
    blob = ctypes.string_at(idx, ilen.value)
    lib.zt_free(idx)
    return _take(out, olen), blob


def deflate_raw_indexed(data, compression_type=2, lazy=0, level=-1, stream_start=0):
    """zt_deflate_raw_indexed: (stream, index blob).  The stream is
    deflate_raw's; the blob describes it placed at byte `stream_start` of the
    buffer later given to inflate_range."""
    b, n = _cbuf(data)
    opts = DeflateOpts(compression_type, lazy, level)
    out, idx = ctypes.POINTER(ctypes.c_uint8)(), ctypes.POINTER(ctypes.c_uint8)()
    olen, ilen = ctypes.c_size_t(), ctypes.c_size_t()
    _check(lib.zt_deflate_raw_indexed(b, n, ctypes.byref(opts), stream_start, ctypes.byref(out), ctypes.byref(olen),
                                      ctypes.byref(idx), ctypes.byref(ilen)))
    return _take_pair(out, olen, idx, ilen)


def gzip_compress_indexed(data, name=None, comment=None, hcrc=False, mtime=0, compression_type=2, lazy=0, level=-1):
    """zt_gzip_compress_indexed: (member bytes, index blob); the blob's
    stream_start is the header's length, so both go straight into
    inflate_range."""
    b, n = _cbuf(data)
    o = GzipOpts()
    o.deflate = DeflateOpts(compression_type, lazy, level)
    o.fname, o.fcomment, o.fhcrc, o.mtime = int(name is not None), int(comment is not None), int(hcrc), mtime
    if name is not None:
        o.name, o.name_len = bytes(name), len(name)
    if comment is not None:
        o.comment, o.comment_len = bytes(comment), len(comment)
    out, idx = ctypes.POINTER(ctypes.c_uint8)(), ctypes.POINTER(ctypes.c_uint8)()
    olen, ilen = ctypes.c_size_t(), ctypes.c_size_t()
    crc = ctypes.c_uint32()
    _check(lib.zt_gzip_compress_indexed(b, n, ctypes.byref(o), ctypes.byref(out), ctypes.byref(olen),
                                        ctypes.byref(crc), ctypes.byref(idx), ctypes.byref(ilen)))
    return _take_pair(out, olen, idx, ilen)


def zlib_compress_indexed(data, compression_type=2, lazy=0, level=-1, dictionary=None):
    """zt_zlib_compress_indexed: (stream, index blob), stream_start 2.  A
    preset dictionary is refused (ZT_E_ARG): the range path has none."""
    if dictionary is not None:
        raise ZtError(-103, "an indexed zlib stream cannot use a preset dictionary")
    b, n = _cbuf(data)
    o = DeflateOpts(compression_type, lazy, level)
    out, idx = ctypes.POINTER(ctypes.c_uint8)(), ctypes.POINTER(ctypes.c_uint8)()
    olen, ilen = ctypes.c_size_t(), ctypes.c_size_t()
    adler = ctypes.c_uint32()
    _check(lib.zt_zlib_compress_indexed(b, n, ctypes.byref(o), ctypes.byref(out), ctypes.byref(olen),
                                        ctypes.byref(adler), ctypes.byref(idx), ctypes.byref(ilen)))
    return _take_pair(out, olen, idx, ilen)


def index_stats(reset=False):
    """Work counters of the index calls (zt_index_stats_read)."""
    s = IndexStats()
    _check(lib.zt_index_stats_read(ctypes.byref(s), 1 if reset else 0))
    return {f: int(getattr(s, f)) for f, _ in IndexStats._fields_}


INDEX_HEADER_BYTES = 64
INDEX_ENTRY_BYTES = 24


def index_entries(idx):
    """An index blob parsed with numpy: (header dict, entries) -- entries a
    record array (in_off, out_off, ntok, flags) of nunits + 1 rows, the
    sentinel last.  Raises ValueError on a blob that is not an index."""
    import numpy as np

    idx = bytes(idx)
    if len(idx) < INDEX_HEADER_BYTES or idx[:4] != b"ZTIX":
        raise ValueError("not an index blob")
    version, nunits, nseg = (int(x) for x in np.frombuffer(idx, dtype="<u4", count=3, offset=4))
    start, end_ip, total = (int(x) for x in np.frombuffer(idx, dtype="<u8", count=3, offset=16))
    if version != 1 or len(idx) != INDEX_HEADER_BYTES + (nunits + 1) * INDEX_ENTRY_BYTES:
        raise ValueError("index blob version or length is wrong")
    ent_t = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("ntok", "<u4"), ("flags", "<u4")])
    ent = np.frombuffer(idx, dtype=ent_t, count=nunits + 1, offset=INDEX_HEADER_BYTES)
    return {"version": version, "nunits": nunits, "nseg": nseg, "stream_start": start, "end_ip": end_ip,
            "total_out": total}, ent


# ---- checkpoint index (include/zt_checkpoint.h) --------------------------------------
CKPT_HEADER_BYTES = 64
CKPT_ENTRY_BYTES = 48
CKPT_WINDOW_BYTES = 32768
CKPT_WINDOW_RECORD_BYTES = 32784
CKPT_FIXED_HDR = 1 << 62
CKPT_KINDS = {"block": 0, "huff": 1, "stored": 2, "shdr": 3, "final": 4}


def inflate_ckpt_build(stream, index=0, span=0, want_output=False):
    """zt_inflate_ckpt_build: decodes the raw stream at stream[index:] once on
    the general path and returns its checkpoint blob (bytes); span: output
    bytes between window checkpoints (0: 1 MiB); want_output: (blob, output,
    end ip)."""
    b, n = _cbuf(stream)
    idx = ctypes.POINTER(ctypes.c_uint8)()
    ilen = ctypes.c_size_t()
    olen = ctypes.c_size_t()
    ip = ctypes.c_size_t()
    if want_output:
        out = ctypes.POINTER(ctypes.c_uint8)()
        _check(lib.zt_inflate_ckpt_build(b, n, index, span, ctypes.byref(idx), ctypes.byref(ilen), ctypes.byref(out),
                                         ctypes.byref(olen), ctypes.byref(ip)))
        return _take(idx, ilen), _take(out, olen), ip.value
    _check(lib.zt_inflate_ckpt_build(b, n, index, span, ctypes.byref(idx), ctypes.byref(ilen), None,
                                     ctypes.byref(olen), ctypes.byref(ip)))
    return _take(idx, ilen)


def inflate_ckpt_range(stream, blob, off, length):
    """zt_inflate_ckpt_range: bytes [off, off + length) of the stream's output
    (pread semantics: length is clamped, off past the end raises ZT_E_ARG)."""
    b, n = _cbuf(stream)
    ib, il = _cbuf(blob)
    out = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    _check(lib.zt_inflate_ckpt_range(b, n, ib, il, off, length, ctypes.byref(out), ctypes.byref(olen)))
    return _take(out, olen)


def inflate_ckpt_ranges(stream, blob, ranges, return_code=False):
    """zt_inflate_ckpt_ranges: [(off, len), ...] in one call.  Returns a list
    of (status, bytes) pairs (bytes None for a failed range); return_code:
    also the call's return code, as (code, list).  A call that fails before
    any range is looked at (a bad blob) raises."""
    b, n = _cbuf(stream)
    ib, il = _cbuf(blob)
    k = len(ranges)
    offs = (ctypes.c_uint64 * k)(*[r[0] for r in ranges])
    lens = (ctypes.c_uint64 * k)(*[r[1] for r in ranges])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    st = (ctypes.c_int * k)()
    rc = lib.zt_inflate_ckpt_ranges(b, n, ib, il, offs, lens, k, outs, olens, st)
    if rc != ZT_OK and all(s == 0 for s in st):
        _check(rc)
    res = []
    for i in range(k):
        res.append((st[i], ctypes.string_at(outs[i], olens[i]) if st[i] == 0 else None))
        if outs[i]:
            lib.zt_free(outs[i])
    return (rc, res) if return_code else res


def ckpt_stats(reset=False):
    """Work counters of the checkpoint calls (zt_ckpt_stats_read)."""
    s = CkptStats()
    _check(lib.zt_ckpt_stats_read(ctypes.byref(s), 1 if reset else 0))
    return {f: int(getattr(s, f)) for f, _ in CkptStats._fields_}


def ckpt_entries(blob):
    """A checkpoint blob parsed with numpy: (header dict, entries, windows) --
    entries a record array (pos, hdr, out_off, kind, rem, flags, ntok, win) of
    nunits + 1 rows, the sentinel last; windows a list of (bytes, crc32) in
    window order.  Raises ValueError on a blob that is not a checkpoint blob."""
    import numpy as np

    blob = bytes(blob)
    if len(blob) < CKPT_HEADER_BYTES or blob[:4] != b"ZTCK":
        raise ValueError("not a checkpoint blob")
    version, nunits, nwin = (int(x) for x in np.frombuffer(blob, dtype="<u4", count=3, offset=4))
    start, end_ip, total, span = (int(x) for x in np.frombuffer(blob, dtype="<u8", count=4, offset=16))
    ent_bytes = (nunits + 1) * CKPT_ENTRY_BYTES
    if version != 1 or len(blob) != CKPT_HEADER_BYTES + ent_bytes + nwin * CKPT_WINDOW_RECORD_BYTES:
        raise ValueError("checkpoint blob version or length is wrong")
    ent_t = np.dtype([("pos", "<u8"), ("hdr", "<u8"), ("out_off", "<u8"), ("kind", "<u4"), ("rem", "<u4"),
                      ("flags", "<u4"), ("ntok", "<u4"), ("win", "<u4"), ("pad", "<u4")])
    ent = np.frombuffer(blob, dtype=ent_t, count=nunits + 1, offset=CKPT_HEADER_BYTES)
    wins = []
    for w in range(nwin):
        at = CKPT_HEADER_BYTES + ent_bytes + w * CKPT_WINDOW_RECORD_BYTES
        wins.append((blob[at:at + CKPT_WINDOW_BYTES],
                     int.from_bytes(blob[at + CKPT_WINDOW_BYTES:at + CKPT_WINDOW_BYTES + 4], "little")))
    return {"version": version, "nunits": nunits, "nwin": nwin, "stream_start": start, "end_ip": end_ip,
            "total_out": total, "span": span}, ent, wins


class BatchStatus(int):
    """An item's status of a container batch call (an int: 0 = decoded) with
    the item's message as `.message`."""

    def __new__(cls, code, message=""):
        self = super().__new__(cls, code)
        self.message = message
        return self


def _batch_statuses(k, st):
    return [BatchStatus(st[i], lib.zt_container_batch_message(i).decode(errors="replace") if st[i] else "")
            for i in range(k)]


def _member_dicts(raw, res, mem, cnt):
    members = []
    for i in range(cnt):
        m = mem[i]
        d = {k: getattr(m, k) for k, _ in GzipMember._fields_}
        d["name"] = raw[m.name_off:m.name_off + m.name_len] if m.flg & 0x08 else None
        d["comment"] = raw[m.comment_off:m.comment_off + m.comment_len] if m.flg & 0x10 else None
        d["data"] = res[m.data_off:m.data_off + m.data_len]
        members.append(d)
    return members


def gunzip_batch(items, return_code=False):
    """zt_gunzip_batch: gunzip() of every item in one call.  Returns a list of
    (status, output, members): status a BatchStatus (0, or the item's error
    code with its message), members as gunzip() gives them; a failed item
    has output None and no members.  return_code: also the call's return code
    (the first failing item's), as (code, list)."""
    bs, ptrs, lens = _batch_ptrs(items)
    k = len(bs)
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    mems = (ctypes.POINTER(GzipMember) * k)()
    cnts = (ctypes.c_size_t * k)()
    st = (ctypes.c_int * k)()
    rc = lib.zt_gunzip_batch(ptrs, lens, k, outs, olens, mems, cnts, st)
    if rc != ZT_OK and all(s == 0 for s in st):
        _check(rc)
    status = _batch_statuses(k, st)
    res = []
    for i in range(k):
        if st[i] == 0:
            data = ctypes.string_at(outs[i], olens[i])
            res.append((status[i], data, _member_dicts(bs[i], data, mems[i], cnts[i])))
        else:
            res.append((status[i], None, []))
        if outs[i]:
            lib.zt_free(outs[i])
        if mems[i]:
            lib.zt_free(mems[i])
    return (rc, res) if return_code else res


def zlib_decompress_batch(items, verify=False, dictionary=None, index=None, return_code=False):
    """zt_zlib_decompress_batch (dictionary: zt_zlib_decompress_batch_dict):
    zlib_decompress() of every item in one call; index: one start per item.
    Returns a list of (status, output, end ip, adler): status a BatchStatus,
    adler the output's Adler-32 when verify is set, else 1; a failed item has
    output None."""
    bs, ptrs, lens = _batch_ptrs(items)
    k = len(bs)
    idx = (ctypes.c_size_t * k)(*index) if index is not None else None
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    ips = (ctypes.c_size_t * k)()
    adl = (ctypes.c_uint32 * k)()
    st = (ctypes.c_int * k)()
    if dictionary is not None:
        d, dn = _cbuf(dictionary)
        rc = lib.zt_zlib_decompress_batch_dict(ptrs, lens, idx, k, int(verify), d, dn, outs, olens, ips, adl, st)
    else:
        rc = lib.zt_zlib_decompress_batch(ptrs, lens, idx, k, int(verify), outs, olens, ips, adl, st)
    if rc != ZT_OK and all(s == 0 for s in st):
        _check(rc)
    status = _batch_statuses(k, st)
    res = []
    for i in range(k):
        res.append((status[i], ctypes.string_at(outs[i], olens[i]) if st[i] == 0 else None, ips[i], adl[i]))
        if outs[i]:
            lib.zt_free(outs[i])
    return (rc, res) if return_code else res


def gunzip_batch_stats():
    """Counters of this thread's last gunzip_batch call (zt_gunzip_batch_stats)."""
    s = GunzipBatchStats()
    _check(lib.zt_gunzip_batch_last_stats(ctypes.byref(s)))
    return {f: int(getattr(s, f)) for f, _ in GunzipBatchStats._fields_}


# ---- device-resident helpers (torch tensors as HBM buffers) -----------------------
# ---- BGZF (include/zt_bgzf.h) -----------------------------------------------------------
BGZF_BLOCK_MAX = 65280


def bgzf_voffset(coffset, uoffset):
    """The virtual offset of byte `uoffset` of the block at file offset `coffset`."""
    return (coffset << 16) | uoffset


def _bgzf_info(info):
    return {f: int(getattr(info, f)) for f, _ in BgzfInfo._fields_}


def bgzf_compress(data, level=-1, compression_type=2, block_size=0, want_index=False):
    """zt_bgzf_compress: the BGZF file of `data`; want_index: (file, .gzi bytes)."""
    b, n = _cbuf(data)
    o = BgzfOpts(DeflateOpts(compression_type, 0, level), block_size)
    out, gzi = ctypes.POINTER(ctypes.c_uint8)(), ctypes.POINTER(ctypes.c_uint8)()
    olen, glen = ctypes.c_size_t(), ctypes.c_size_t()
    if want_index:
        _check(lib.zt_bgzf_compress(b, n, ctypes.byref(o), ctypes.byref(out), ctypes.byref(olen), ctypes.byref(gzi),
                                    ctypes.byref(glen)))
        return _take_pair(out, olen, gzi, glen)
    _check(lib.zt_bgzf_compress(b, n, ctypes.byref(o), ctypes.byref(out), ctypes.byref(olen), None, None))
    return _take(out, olen)


def bgzf_index(data, return_info=False):
    """zt_bgzf_index: the file's .gzi from a host walk (no GPU); return_info:
    (.gzi, info dict).  A malformed file raises ZtError with `.info`."""
    b, n = _cbuf(data)
    gzi = ctypes.POINTER(ctypes.c_uint8)()
    glen = ctypes.c_size_t()
    info = BgzfInfo()
    rc = lib.zt_bgzf_index(b, n, ctypes.byref(gzi), ctypes.byref(glen), ctypes.byref(info))
    if rc != ZT_OK:
        err = ZtError(rc, lib.zt_last_error_message().decode(errors="replace"))
        err.info = _bgzf_info(info)
        raise err
    blob = ctypes.string_at(gzi, glen.value)
    lib.zt_free(gzi)
    return (blob, _bgzf_info(info)) if return_info else blob


def bgzf_decompress(data, return_info=False):
    """zt_bgzf_decompress: the whole file; return_info: (output, info dict).
    A failure raises ZtError with `.info` (error_offset: the failing block)."""
    b, n = _cbuf(data)
    out = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    info = BgzfInfo()
    rc = lib.zt_bgzf_decompress(b, n, ctypes.byref(out), ctypes.byref(olen), ctypes.byref(info))
    if rc != ZT_OK:
        err = ZtError(rc, lib.zt_last_error_message().decode(errors="replace"))
        err.info = _bgzf_info(info)
        raise err
    res = _take(out, olen)
    return (res, _bgzf_info(info)) if return_info else res


def _bgzf_results(rc, k, outs, olens, st, return_code):
    if rc != ZT_OK and all(s == 0 for s in st):
        _check(rc)
    msg = lib.zt_last_error_message().decode(errors="replace") if rc != ZT_OK else ""
    res, first = [], True
    for i in range(k):
        m = ""
        if st[i] != 0:
            m = msg if first and st[i] == rc else ERRORS.get(st[i], str(st[i]))
            first = False
        res.append((BatchStatus(st[i], m), ctypes.string_at(outs[i], olens[i]) if st[i] == 0 else None))
        if outs[i]:
            lib.zt_free(outs[i])
    return (rc, res) if return_code else res


def bgzf_read_ranges(data, ranges, gzi=None, return_code=False):
    """zt_bgzf_read_ranges: [(off, len), ...] by uncompressed offset in one
    call.  Returns a list of (BatchStatus, bytes) pairs (bytes None for a failed
    range); return_code: (code, list).  A call that fails before any range is
    looked at (a bad .gzi, a file that is not BGZF) raises."""
    b, n = _cbuf(data)
    gb, gl = _cbuf(gzi) if gzi is not None else (None, 0)
    k = len(ranges)
    offs = (ctypes.c_uint64 * k)(*[r[0] for r in ranges])
    lens = (ctypes.c_uint64 * k)(*[r[1] for r in ranges])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    st = (ctypes.c_int * k)()
    rc = lib.zt_bgzf_read_ranges(b, n, gb, gl, offs, lens, k, outs, olens, st)
    return _bgzf_results(rc, k, outs, olens, st, return_code)


def bgzf_read_virtual(data, chunks, return_code=False):
    """zt_bgzf_read_virtual: [(vbeg, vend), ...] virtual-offset chunks in one
    call; results as bgzf_read_ranges gives them."""
    b, n = _cbuf(data)
    k = len(chunks)
    vb = (ctypes.c_uint64 * k)(*[c[0] for c in chunks])
    ve = (ctypes.c_uint64 * k)(*[c[1] for c in chunks])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    st = (ctypes.c_int * k)()
    rc = lib.zt_bgzf_read_virtual(b, n, vb, ve, k, outs, olens, st)
    return _bgzf_results(rc, k, outs, olens, st, return_code)


def bgzf_stats(reset=False):
    """Work counters of the BGZF read calls (zt_bgzf_stats_read)."""
    s = BgzfStats()
    _check(lib.zt_bgzf_stats_read(ctypes.byref(s), 1 if reset else 0))
    return {f: int(getattr(s, f)) for f, _ in BgzfStats._fields_}


def dev_checksums(ptr, n, crc=0, adler=1, stream=None):
    c, a = ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib.zt_dev_checksums(ptr, n, crc, adler, ctypes.byref(c), ctypes.byref(a), stream))
    return c.value, a.value


class DeflatePlan:
    def __init__(self, max_n, level=-1, compression_type=2, strategy=None):
        self.h = ctypes.c_void_p()
        opts = DeflateOpts(compression_type, 0, level)
        _check(lib.zt_deflate_plan_create(max_n, ctypes.byref(opts), ctypes.byref(self.h)))
        if strategy is not None:
            self.set_strategy(strategy)

    def set_strategy(self, strategy):
        """The strategy of every later run (include/zt_strategy.h)."""
        _check(lib.zt_deflate_plan_set_strategy(self.h, strategy))

    def run(self, d_in, n, d_out, halo=0, final=1, stream=None):
        olen = ctypes.c_size_t()
        _check(lib.zt_deflate_dev(self.h, d_in, n, halo, final, d_out, ctypes.byref(olen), stream))
        return olen.value

    def close(self):
        if self.h and lib is not None:
            lib.zt_deflate_plan_destroy(self.h)
            self.h = ctypes.c_void_p()

    __del__ = close


class InflatePlan:
    def __init__(self, max_in, max_out):
        self.h = ctypes.c_void_p()
        _check(lib.zt_inflate_plan_create(max_in, max_out, ctypes.byref(self.h)))

    def run(self, d_in, n, d_out, out_cap, stream=None):
        olen, ip = ctypes.c_size_t(), ctypes.c_size_t()
        _check(lib.zt_inflate_dev(self.h, d_in, n, d_out, out_cap, ctypes.byref(olen), ctypes.byref(ip), stream))
        return olen.value, ip.value

    def close(self):
        if self.h and lib is not None:
            lib.zt_inflate_plan_destroy(self.h)
            self.h = ctypes.c_void_p()

    __del__ = close


def deflate_bound(n):
    return lib.zt_deflate_bound(n)


# ---- include/zt_dev_batch.h: batches of device buffers, by pointer ----------------
DEV_BATCH_FORMATS = {"raw": 0, "zlib": 1, "gzip": 2}


def deflate_dev_batch_bound(n, compression_type=2, format="raw", level=-1):
    """Upper bound of one item's output (level 0 writes stored blocks, as type 0)."""
    return lib.zt_deflate_dev_batch_bound(n, 0 if level == 0 else compression_type,
                                          DEV_BATCH_FORMATS.get(format, format))


def _ptr_array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*[int(p) or None for p in ptrs])


def deflate_dev_batch(ptrs, sizes, out_ptrs, out_caps, format="raw", level=-1, compression_type=2, stream=None):
    """Device buffers (ptrs[i], sizes[i]) deflated into (out_ptrs[i], out_caps[i]).
    Returns (out_lens, statuses); an item that does not fit has ZT_E_ARG and the
    length it needs.  Raises only when the call fails as a whole."""
    k = len(ptrs)
    olens, st = (ctypes.c_size_t * k)(), (ctypes.c_int * k)()
    opts = DeflateOpts(compression_type, 0, level)
    rc = lib.zt_deflate_dev_batch(_ptr_array(ptrs), (ctypes.c_size_t * k)(*sizes), k, ctypes.byref(opts),
                                  DEV_BATCH_FORMATS.get(format, format), _ptr_array(out_ptrs),
                                  (ctypes.c_size_t * k)(*out_caps), olens, st, stream)
    if rc != ZT_OK and all(s == 0 for s in st):
        _check(rc)
    return list(olens), list(st)


def inflate_dev_batch(ptrs, sizes, out_ptrs, out_caps=None, index=None, checksums=False, stream=None):
    """Raw DEFLATE streams in device buffers decoded into device buffers.
    out_ptrs None: sizes only.  Returns (out_lens, end_ips, statuses), with
    checksums=True also (crcs, adlers).  Per-item failures are statuses, with
    the first one's message in zt_last_error_message as zt_inflate_raw_batch
    leaves it; raises only when the call fails as a whole."""
    k = len(ptrs)
    olens, ips, st = (ctypes.c_size_t * k)(), (ctypes.c_size_t * k)(), (ctypes.c_int * k)()
    crcs = (ctypes.c_uint32 * k)() if checksums else None
    adlers = (ctypes.c_uint32 * k)() if checksums else None
    rc = lib.zt_inflate_dev_batch(_ptr_array(ptrs), (ctypes.c_size_t * k)(*sizes),
                                  (ctypes.c_size_t * k)(*index) if index is not None else None, k,
                                  _ptr_array(out_ptrs) if out_ptrs is not None else None,
                                  (ctypes.c_size_t * k)(*out_caps) if out_ptrs is not None else None,
                                  olens, ips, st, crcs, adlers, stream)
    if rc != ZT_OK and all(s == 0 for s in st):
        _check(rc)
    res = (list(olens), list(ips), list(st))
    return res + (list(crcs), list(adlers)) if checksums else res


def debug_dev_batch_times(enable):
    """(gather ms, scatter ms) by HIP events since the last call, cleared; the
    timing is on for the following calls when `enable` (measurement only)."""
    v = (ctypes.c_double * 2)()
    _check(lib.zt_debug_dev_batch_times(1 if enable else 0, v))
    return v[0], v[1]


def _torch_stream(tensors, stream):
    """The stream handle to pass for a list of cuda tensors: the given one, else
    torch's current stream.  NULL names the library's own stream, which does
    not wait for torch's default stream, so with that one current it is
    synchronised first (the calls wait for their own work before returning)."""
    import torch

    if stream is not None:
        return stream
    s = torch.cuda.current_stream(tensors[0].device if tensors else None)
    if not s.cuda_stream:
        s.synchronize()
        return None
    return s.cuda_stream


def _check_tensors(tensors):
    import torch

    for t in tensors:
        if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 1 or (t.numel() > 1 and t.stride(0) != 1):
            raise ValueError("expected one-dimensional contiguous uint8 cuda tensors")


def deflate_tensors(tensors, format="raw", level=-1, compression_type=2, stream=None):
    """Every uint8 cuda tensor of the list deflated on the device; returns a list
    of uint8 cuda tensors, views into one output tensor sized by the bound."""
    import torch

    _check_tensors(tensors)
    if not tensors:
        return []
    sizes = [t.numel() for t in tensors]
    caps = [deflate_dev_batch_bound(n, compression_type, format, level) for n in sizes]
    offs, tot = [], 0
    for c in caps:
        offs.append(tot)
        tot += (c + 15) & ~15
    s = _torch_stream(tensors, stream)
    out = torch.empty(tot, dtype=torch.uint8, device=tensors[0].device)
    base = out.data_ptr()
    lens, st = deflate_dev_batch([t.data_ptr() for t in tensors], sizes, [base + o for o in offs], caps,
                                 format=format, level=level, compression_type=compression_type, stream=s)
    if any(st):
        _check(st[[bool(x) for x in st].index(True)])
    return [out[o:o + n] for o, n in zip(offs, lens)]


def inflate_tensors(tensors, out_sizes=None, stream=None):
    """Every raw DEFLATE stream of the list (uint8 cuda tensors) decoded on the
    device; returns a list of uint8 cuda tensors, views into one output tensor.
    out_sizes None: the sizes come from a sizes-only call first."""
    import torch

    _check_tensors(tensors)
    if not tensors:
        return []
    ptrs, sizes = [t.data_ptr() for t in tensors], [t.numel() for t in tensors]
    s = _torch_stream(tensors, stream)
    if out_sizes is None:
        out_sizes, _, st = inflate_dev_batch(ptrs, sizes, None, stream=s)
        if any(st):
            _check(st[[bool(x) for x in st].index(True)])
    offs, tot = [], 0
    for c in out_sizes:
        offs.append(tot)
        tot += (c + 15) & ~15
    out = torch.empty(max(tot, 1), dtype=torch.uint8, device=tensors[0].device)
    base = out.data_ptr()
    lens, _, st = inflate_dev_batch(ptrs, sizes, [base + o for o in offs], list(out_sizes), stream=s)
    if any(st):
        _check(st[[bool(x) for x in st].index(True)])
    return [out[o:o + n] for o, n in zip(offs, lens)]


GEN_KINDS = {"xorshift32": 0, "wordsalad": 1, "structured": 2, "mixed": 3}


def synth_dev(kind, seed, ptr, n, stream=None):
    """Fill device memory with a synthetic corpus (64 KiB piece i = generator
    seeded with seed + i)."""
    _check(lib.zt_synth_dev(GEN_KINDS.get(kind, kind), seed, ptr, n, stream))


def synth_dev_at(kind, seed, offset, ptr, n, stream=None):
    """Bytes [offset, offset + n) of the corpus synth_dev would write from 0
    (offset a multiple of 64 KiB): one rank's shard of a sharded buffer."""
    if offset % 65536:
        raise ValueError("offset must be a multiple of 64 KiB")
    _check(lib.zt_synth_dev_at(GEN_KINDS.get(kind, kind), seed, offset // 65536, ptr, n, stream))


def timing_enable(on=True):
    _check(lib.zt_timing_enable(1 if on else 0))


def timing_read():
    t = KernelTimes()
    _check(lib.zt_timing_read(ctypes.byref(t)))
    return {"deflate_ms": t.deflate_ms, "deflate_launches": t.deflate_launches,
            "inflate_ms": t.inflate_ms, "inflate_launches": t.inflate_launches,
            "deflate_pipeline_ms": t.deflate_pipeline_ms, "deflate_pipelines": t.deflate_pipelines,
            "inflate_tok_ms": t.inflate_tok_ms, "inflate_toks": t.inflate_toks,
            "inflate_paths": list(t.inflate_paths), "general_passes": t.general_passes,
            "blocks_unsearched": t.blocks_unsearched}


def debug_match_modes():
    """(queued, at once): blocks of the deflate match kernel by the way they measured
    their candidates, since the last call (reads and clears the device counter)."""
    v = (ctypes.c_uint64 * 2)()
    _check(lib.zt_debug_match_modes(v))
    return int(v[0]), int(v[1])


def debug_head_formats():
    """(u32 -> u16, u16 -> u32): chain-head format changes of the deflate match
    kernel's workgroups since the last call (reads and clears the device counter)."""
    v = (ctypes.c_uint64 * 2)()
    _check(lib.zt_debug_head_formats(v))
    return int(v[0]), int(v[1])


# the record zt_debug_match fills, in its order (csrc/zt_internal.h)
DEBUG_MATCH_INFO = ("block", "sub", "maxdist", "segment", "blocks_per_wg", "max_chain", "nice_len", "skip_len", "good",
                    "klen", "probe", "too_far", "p4far", "adapt_depth", "adapt_thr", "adapt_depth2", "adapt_thr2",
                    "mq_thr", "nblocks", "nwg")


def debug_match_strategy(data, strategy, level=6, halo=0):
    """debug_match with a strategy (zt_debug_match_strategy): what the
    strategy calls launch in place of match_kernel.  Same returns."""
    return debug_match(data, level, halo, strategy)


def debug_match(data, level=6, halo=0, strategy=None):
    """The deflate match stage's result for `data` (the first `halo` <= 32768
    bytes are history in front of the stream, not positions): what deflate_raw
    (DYNAMIC) runs up to and including match_kernel, environment hooks
    included.  Returns (res, store, info): res uint32[n], per position
    byte << 24 | len << 15 | dist, 0xFFFFFFFF where the kernel wrote nothing;
    store uint8[blocks], classify_kernel's flags; info: a dict of the
    constants and parameters the call used (DEBUG_MATCH_INFO)."""
    import numpy as np

    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n = buf.size - halo
    if n <= 0 or halo < 0:
        raise ValueError("debug_match needs at least one byte after the halo")
    res = np.zeros(n, dtype=np.uint32)
    info = np.zeros(len(DEBUG_MATCH_INFO), dtype=np.uint32)
    store = np.zeros(n // 4096 + 2, dtype=np.uint8)  # (room whatever the build's block size: a block holds sub-chunks)
    if strategy is not None:
        _check(lib.zt_debug_match_strategy(buf.ctypes.data, n, halo, level, strategy, res.ctypes.data,
                                           store.ctypes.data, info.ctypes.data))
    else:
        _check(lib.zt_debug_match(buf.ctypes.data, n, halo, level, res.ctypes.data, store.ctypes.data,
                                  info.ctypes.data))
    d = {k: int(v) for k, v in zip(DEBUG_MATCH_INFO, info)}
    return res, store[:d["nblocks"]], d


def debug_huffman(freqs, n, limit):
    """The deflate block kernel's code construction on given histograms: freqs
    is count * n frequencies (count histograms of n <= 286 symbols), limit 7 or
    15.  Returns (lens uint8[count, n], codes uint32[count, n]); a code is
    len << 16 | the canonical code bit-reversed, 0 for an unused symbol.
    Frequencies of 2^23 or more and histograms summing to 2^27 or more are
    rejected (ZT_E_ARG)."""
    import numpy as np

    f = np.ascontiguousarray(freqs, dtype=np.uint32).reshape(-1)
    if n <= 0 or f.size == 0 or f.size % n:
        raise ValueError("freqs must hold a whole number of n-entry histograms")
    count = f.size // n
    lens = np.zeros((count, n), dtype=np.uint8)
    codes = np.zeros((count, n), dtype=np.uint32)
    _check(lib.zt_debug_huffman(f.ctypes.data, count, n, limit, lens.ctypes.data, codes.ctypes.data))
    return lens, codes


def debug_chain(res, restart, tok_off, out_cap, desc_cap, max_seg, host=False):
    """The segment chain of one stream's unit tables (csrc/inflate_chain.h), built by
    chain_kernel on the device or, host=True, by seg_chain_host.  res: numpy
    records (out_len u8, end_bits u8, ntok u4, status i4, detail i4, stop_idx
    i4), restart: u1[units - 1], tok_off: u8[units].  Returns (info, units,
    segs): info = dict(ok, nseg, total, end_bits, desc_total), units / segs numpy
    records of ChainUnit / SegJob (empty unless info['ok']); host=True adds
    info['outcome'] (0 built, 1 fallback, 2 ran out of input)."""
    import numpy as np

    cu_t = np.dtype([("tok_off", "<u8"), ("out_off", "<u8"), ("seg_off", "<u8"), ("desc_off", "<u8"),
                     ("ntok", "<u4"), ("out_len", "<u4")])
    sj_t = np.dtype([("first", "<u4"), ("count", "<u4")])
    info_t = np.dtype([("ok", "<i4"), ("nseg", "<u4"), ("total", "<u8"), ("end_bits", "<u8"), ("desc_total", "<u8")])
    n = len(res)
    res = np.ascontiguousarray(res)
    assert res.dtype.itemsize == 32 and len(tok_off) == n
    rs = np.zeros(max(n, 1), dtype=np.uint8)
    rs[:n - 1] = restart
    to = np.ascontiguousarray(tok_off, dtype=np.uint64)
    info = np.zeros(1, dtype=info_t)
    cu = np.zeros(n, dtype=cu_t)
    sj = np.zeros(max(n if host else max_seg, 1), dtype=sj_t)
    if host:
        nchain, outcome = ctypes.c_uint32(0), ctypes.c_int(0)
        _check(lib.zt_debug_chain_host(res.ctypes.data, rs.ctypes.data, to.ctypes.data, n, info.ctypes.data,
                                       cu.ctypes.data, sj.ctypes.data, ctypes.byref(nchain), ctypes.byref(outcome)))
        cu = cu[:nchain.value]
    else:
        _check(lib.zt_debug_chain(res.ctypes.data, rs.ctypes.data, to.ctypes.data, n, out_cap, desc_cap, max_seg,
                                  info.ctypes.data, cu.ctypes.data, sj.ctypes.data))
    d = {k: int(info[0][k]) for k in info_t.names}
    if host:
        d["outcome"] = outcome.value
    if not d["ok"]:
        return d, cu[:0], sj[:0]
    return d, cu, sj[:d["nseg"]]


def scratch_bytes():
    """(device scratch, pinned host staging) bytes the device context caches."""
    d, h = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _check(lib.zt_scratch_bytes(ctypes.byref(d), ctypes.byref(h)))
    return d.value, h.value


def release_scratch():
    _check(lib.zt_release_scratch())
