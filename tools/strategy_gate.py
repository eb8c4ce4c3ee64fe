# Size of the strategies' streams against zlib's at the same strategy and
# level 6, on the 16 windows of the ratio gate's corpus (tests/ratio_corpus.py):
# per window this build's bytes over Python zlib's (raw streams), per strategy
# the worst window.  Both sides are deterministic.  The GPU test
# (tests/test_gpu_strategy.py::test_size_against_zlib) holds one window per
# generator to the worst recorded here, rounded up to the next 0.005.
#   usage: python tools/strategy_gate.py [profiles/strategy_gate.txt]
import math, os, sys, zlib
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'tests')); sys.path.insert(0, os.path.join(HERE, '..', 'zlib.ts_amd', 'py'))
import ztamd as zt, zt_oracle
from ratio_corpus import windows

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, '..', 'profiles', 'strategy_gate.txt')
wins = windows(zt_oracle.Oracle())
lines = ["# this build's bytes / zlib's bytes, raw DEFLATE, level 6, same strategy; 4 MiB windows (tests/ratio_corpus.py)"]
for name, st in (("rle", zt.STRATEGY_RLE), ("huffman_only", zt.STRATEGY_HUFFMAN_ONLY)):
    worst = (0.0, "")
    for g, label, data in wins:
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, st)
        ref = len(c.compress(data) + c.flush())
        ours = len(zt.deflate_raw(data, level=6, strategy=st))
        assert zlib.decompress(zt.deflate_raw(data, level=6, strategy=st), -15) == data
        ratio = ours / ref
        worst = max(worst, (ratio, label))
        lines.append(f"{name:13s} {label:24s} ours {ours:9d}  zlib {ref:9d}  ratio {ratio:.5f}")
    bound = math.ceil(worst[0] / 0.005 - 1e-9) * 0.005
    lines.append(f"{name:13s} worst {worst[1]} {worst[0]:.5f}  -> test bound {bound:.3f}")
text = "\n".join(lines) + "\n"
print(text, end="")
with open(out, "w") as f:
    f.write(text)
