# Hop statistics of the match kernel (needs libzt built with -DZT_DF_COUNT, ZT_LIB=...).
# ZT_DF_MQ=0 / 1 / <n> chooses which blocks measure through the queues: "queued"
# is the share of the measured candidates that went through a queue, a pass is
# one wave-level run of the measurement (at once: whenever a lane has a
# candidate; queued: 64 at a time), and the improve / no-gain shares count the
# candidates measured at once only.
import ctypes, os, sys; sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'zlib.ts_amd', 'py'))
import torch, ztamd as zt
buf = (ctypes.c_ulonglong * 8)()
for kind in sys.argv[1:]:
    n = 128 << 20
    d_in = torch.empty(n, dtype=torch.uint8, device="cuda")
    zt.synth_dev(kind, 5, d_in.data_ptr(), n)
    d_c = torch.empty(zt.deflate_bound(n), dtype=torch.uint8, device="cuda")
    dp = zt.DeflatePlan(n)
    dp.run(d_in.data_ptr(), n, d_c.data_ptr()); torch.cuda.synchronize()
    zt.lib.zt_debug_df_count(buf)
    zt.debug_match_modes()
    dp.run(d_in.data_ptr(), n, d_c.data_ptr()); torch.cuda.synchronize()
    zt.lib.zt_debug_df_count(buf)
    v = list(buf)
    at_once = max(1, v[2] - v[7])
    print(kind, 'blocks queued / at once', zt.debug_match_modes(),
          'pair-steps/wave', v[0], 'lane hops', v[1], 'measured', v[2], 'queued %.3f' % (v[7] / max(1, v[2])),
          'hops/position %.2f' % (v[1] / n),
          'lane-util %.2f' % (v[1] / max(1, v[0] * 128)), 'passes/step %.2f' % (v[3] / max(1, v[0])),
          'lanes/pass %.1f' % (v[2] / max(1, v[3])),
          'at once: improve %.3f, < 8 bytes %.3f, no gain %.3f' % (v[4] / at_once, v[5] / at_once, v[6] / at_once),
          flush=True)
