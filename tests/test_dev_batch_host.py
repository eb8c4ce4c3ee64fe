"""Host-only checks of the device-resident batch calls (include/zt_dev_batch.h):
tools/dev_batch_host_check.cpp (the copy and patch job tables of
zlib.ts_amd/csrc/dev_batch_plan.h run by a host model of the kernels' accesses,
the stored-block jobs, the bound, the groups, the capacity masking and the tile
limit, against slow restatements) built with ASan + UBSan as a stand-alone
program and run on the CPU; the ABI of the header; and the calls' answer
without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ZT_E_NO_DEVICE = -100


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ missing")
def test_dev_batch_host_check_sanitized(tmp_path):
    exe = str(tmp_path / "dev_batch_host_check")
    b = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-pthread", "-o", exe, os.path.join(ROOT, "tools", "dev_batch_host_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("dev_batch_host_check ok")


def test_header_declares_what_the_binding_binds():
    """every function include/zt_dev_batch.h declares is in the Python binding's
    list and exported by libzt.so, and the other way round; none of them is in
    zt.h's list"""
    import ztamd

    src = open(os.path.join(ROOT, "include", "zt_dev_batch.h")).read()
    declared = set(re.findall(r"^(?:int|size_t) (zt_\w+)\(", src, flags=re.M))
    assert declared == set(ztamd.DEV_BATCH_SYMBOLS) and len(declared) == 3
    lib = ctypes.CDLL(ztamd.LIBPATH)
    assert not [n for n in declared if not hasattr(lib, n)]
    assert not set(ztamd.DEV_BATCH_SYMBOLS) & set(ztamd.SYMBOLS)
    for name, v in (("RAW", 0), ("ZLIB", 1), ("GZIP", 2)):
        assert re.search(rf"#define ZT_DEV_BATCH_{name}\s+{v}\b", src)
        assert ztamd.DEV_BATCH_FORMATS[name.lower()] == v


def test_bound_needs_no_device():
    """the bound is plain arithmetic: stored exact, the pipeline's worst case per
    32 KiB block, the framing on top; 0 for an unknown type or format"""
    import ztamd

    b = ztamd.deflate_dev_batch_bound
    assert b(0) == 5 and b(0, format="gzip") == 23 and b(0, format="zlib") == 11
    assert b(65535, 0) == 65540 and b(65536, 0) == 65536 + 10 and b(1, level=0) == 6
    assert b(32768) == 32778 and b(32769) == 32769 + 20 and b(100001, format="gzip") == 100001 + 40 + 18
    assert b(33 * 32768) == 33 * 32768 + 330 + 10  # one restart marker after the 32nd block
    assert b(1000, 1) == b(1000, 2) + 1000 // 8 + 64
    assert ztamd.lib.zt_deflate_dev_batch_bound(10, 3, 0) == 0 and ztamd.lib.zt_deflate_dev_batch_bound(10, 2, 3) == 0


def test_calls_without_a_device():
    """without a GPU the calls return ZT_E_NO_DEVICE (count 0: ZT_OK, no device asked for)"""
    import ztamd

    assert ztamd.lib.zt_deflate_dev_batch(None, None, 0, None, 0, None, None, None, None, None) == 0
    assert ztamd.lib.zt_inflate_dev_batch(None, None, None, 0, None, None, None, None, None, None, None, None) == 0
    import torch

    if torch.cuda.is_available():
        return  # tests/test_gpu_dev_batch.py runs the calls
    assert ztamd.device_count() == 0
    with pytest.raises(ztamd.ZtError) as e:
        ztamd.deflate_dev_batch([0x1000], [16], [0x2000], [64])
    assert e.value.code == ZT_E_NO_DEVICE
    with pytest.raises(ztamd.ZtError) as e:
        ztamd.inflate_dev_batch([0x1000], [16], [0x2000], [64])
    assert e.value.code == ZT_E_NO_DEVICE
    with pytest.raises(ztamd.ZtError) as e:
        ztamd.inflate_dev_batch([0x1000], [16], None)
    assert e.value.code == ZT_E_NO_DEVICE
