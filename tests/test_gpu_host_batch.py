"""The host batch layer (zlib.ts_amd/csrc/host_batch.cpp, xfer.cpp) on the
GPU: the device fan-out with fewer items than devices, and the staged
transfers at the sizes where they change path.  Both run in child processes:
ZT_ALIAS_DEVICES and ZT_HOST_POOL_MB are read once when the library loads.
(The fan-out's collection of a failed share's code and message is checked on
the CPU: tools/batch_plan_check.cpp, tests/test_container_batch_host.py.)"""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MiB = 1 << 20


def _child(script, args, env):
    p = subprocess.run([sys.executable, os.path.join(HERE, script), *args], env=env, capture_output=True, text=True,
                       timeout=100)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_fewer_items_than_devices():
    """Batches of one and two items under zt_set_devices(0b111) on three
    aliased devices: every compress, dictionary and decode batch gives the
    one-device outputs, and they decode with Python's zlib -- the device
    count is clamped to the item count in one place (for_each_device), which
    also gives the dictionary inflate its copy-thread budget."""
    res = _child("host_batch_few_items_child.py", [], dict(os.environ, ZT_ALIAS_DEVICES="3"))
    good = {"equal": True, "decodes": True}
    assert res == {"logical_devices": 3, "two": good, "empty_and_one": good, "one_empty": good}, res


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8 * MiB - 1, 8 * MiB, 32 * MiB + 1, 64 * MiB + 4097])
def test_staged_transfers_at_their_edges(n):
    """With the host pool off nothing is host_direct: below 8 MiB one copy,
    from 8 MiB on the two pinned 32 MiB chunks -- one chunk, a second chunk of
    one byte, three chunks with a ragged tail.  CRC-32 and Adler-32 (upload)
    equal zlib's, a stored deflate and its inflate return the input (upload
    and download), and at 64 MiB + 4097 the pipelined deflate and inflate do
    (both staged stages of the three-stage pipeline)."""
    res = _child("host_batch_xfer_child.py", [str(n)], dict(os.environ, ZT_HOST_POOL_MB="0"))
    assert res == {"n": n, "rounds": 1, "round0": True}, res


@pytest.mark.gpu
def test_staged_transfers_pool_on_twice():
    """The 64 MiB + 4097 case with the pool on, twice in a row: the second
    round's outputs land in the buffers the first round returned to the pool,
    registered by then -- the host_direct branch of download and of the
    pipeline's download stage."""
    env = {k: v for k, v in os.environ.items() if k != "ZT_HOST_POOL_MB"}
    res = _child("host_batch_xfer_child.py", [str(64 * MiB + 4097), "pool"], env)
    assert res == {"n": 64 * MiB + 4097, "rounds": 2, "round0": True, "round1": True}, res
