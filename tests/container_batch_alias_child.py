"""Child process of tests/test_gpu_container_batch.py::test_alias_devices:
with ZT_ALIAS_DEVICES set the library presents that many logical devices on
the one GPU (one context and host thread each); 256 gzip items and 256 zlib
items are decoded spread over all of them by zt_set_devices (LPT split,
container_batch_api.cpp run_shares) and the digests of outputs and members
are printed as JSON.  Test infrastructure only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "zlib.ts_amd", "py"))
import ztamd as zt  # noqa: E402
import zt_oracle  # noqa: E402
from container_batch_corpus import alias_items, results_digest  # noqa: E402

gz, zl, _ = alias_items(zt_oracle.Oracle())
ndev = zt.device_count()
zt.set_devices((1 << ndev) - 1)
try:
    g = zt.gunzip_batch(gz)
    stats = zt.gunzip_batch_stats()
    z = zt.zlib_decompress_batch(zl, verify=True)
finally:
    zt.set_devices(0)
print(json.dumps({"logical_devices": ndev, "gzip": results_digest(g), "zlib": results_digest(z),
                  "items": stats["items"], "members": stats["members"]}), flush=True)
