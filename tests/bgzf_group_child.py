"""Child process of tests/test_gpu_bgzf.py::test_grouping_does_not_change_a_byte:
runs with ZT_BGZF_GROUP_BLOCKS set (read once per process), writes the 13-block
inputs below and prints the SHA-256 of each file and of its .gzi as one JSON
line.  The parent writes the same inputs in one group and compares.  Test
infrastructure only."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "zlib.ts_amd", "py"))


def inputs():
    import zt_oracle

    o = zt_oracle.Oracle()
    return {"4096": (o.gen("wordsalad", 21, 13 * 4096 - 100), 4096),
            "65280": (o.gen("structured", 22, 12 * 65280 + 77), 65280)}


if __name__ == "__main__":
    import ztamd as zt

    res = {}
    for name, (data, bs) in inputs().items():
        f, gzi = zt.bgzf_compress(data, block_size=bs, want_index=True)
        assert zt.bgzf_decompress(f) == data
        res[name] = [hashlib.sha256(f).hexdigest(), hashlib.sha256(gzi).hexdigest()]
    print(json.dumps(res), flush=True)
