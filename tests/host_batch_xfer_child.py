"""Child process of tests/test_gpu_host_batch.py: the staged host transfers
(xfer.cpp: upload, download, the pipeline's stages) on one host buffer of
argv[1] bytes.  Run with ZT_HOST_POOL_MB=0 nothing is host_direct, so every
copy of 8 MiB or more goes through the pinned chunks; argv[2] = "pool": the
pool stays on and every call runs twice, the second one finding the first
one's output buffer registered (the host_direct branch).  Prints a JSON
verdict.  Test infrastructure only."""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "zlib.ts_amd", "py"))
import ztamd as zt  # noqa: E402

n = int(sys.argv[1])
rounds = 2 if sys.argv[2:] == ["pool"] else 1
a = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
a[: n // 2: 2] = 0x41  # (half of it compresses)
data = a.tobytes()
res = {"n": n, "rounds": rounds}
for r in range(rounds):
    ok = {}
    ok["crc32"] = zt.crc32(data) == zlib.crc32(data)  # upload
    ok["adler32"] = zt.adler32(data) == zlib.adler32(data)
    stored = zt.deflate_raw(data, compression_type=0)  # upload and download
    ok["stored_len"] = len(stored) == n + 5 * ((n + 65534) // 65535)
    ok["stored_zlib"] = zlib.decompress(stored, -15) == data
    ok["stored_round_trip"] = zt.inflate_raw(stored) == (data, len(stored))
    if n >= 64 << 20:  # the three-stage pipeline, both directions
        s = zt.deflate_raw(data)
        ok["pipe_zlib"] = zlib.decompress(s, -15) == data
        ok["pipe_round_trip"] = zt.inflate_raw(s) == (data, len(s))
    res["round%d" % r] = all(ok.values()) or ok
print(json.dumps(res), flush=True)
