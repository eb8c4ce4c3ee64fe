"""Host-only check of the member framing (zlib.ts_amd/csrc/member_frame.h and
dict_host.h's zlib_header_status): tools/member_frame_host_check.cpp (the zlib
and gzip headers byte for byte and read back by the read side's parsers, the
trailers, the stored blocks against the device-resident batch's jobs run by the
kernels' host model, the header statuses and their texts) built with ASan +
UBSan as a stand-alone program and run on the CPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ missing")
def test_member_frame_host_check_sanitized(tmp_path):
    exe = str(tmp_path / "member_frame_host_check")
    b = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tools", "member_frame_host_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("member_frame_host_check ok")
