"""bcp_mppi against the composition the package allowed before it -- per iteration torch.randn of [H, N, K, 2], add / clip,
a per-env env.lookahead, and torch reductions for the weights and the new mean -- and against I plain look-aheads, the floor
(the roll-outs alone, their actions already in memory).  Metric configuration (RandomMiniEnv seed-0 geometry, shared map
and path) at steady state.  HIP events around every repetition, after warm-up; median (min - max).

    python tools/bench_mppi.py [reps]"""
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
import bench

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
SIGMA, LAM, PENALTY = (0.2, 0.6), 0.3, 2.0


def timed(fn, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return "%.3f ms (%.3f - %.3f)" % (float(np.median(ms)), float(np.min(ms)), float(np.max(ms))), float(np.median(ms))


for n, k, h, it in ((4096, 64, 16, 4), (65536, 16, 8, 2)):
    env, g = bench.make_env(n, 0, 0, 2024)
    rng = np.random.RandomState(1234)
    pool = torch.from_numpy(np.stack([env.action_space.sample_batch(n, rng) for _ in range(16)])).cuda()
    bench.steady_state(env, pool, rng)
    low = torch.from_numpy(np.asarray(env.action_space.low, np.float64)).cuda()
    high = torch.from_numpy(np.asarray(env.action_space.high, np.float64)).cuda()
    sigma = torch.tensor(SIGMA, dtype=torch.float64, device="cuda")
    mean0 = (0.5 * (low + high)).expand(n, h, 2).contiguous()
    mean = mean0.clone()
    out = {}

    def fused():
        mean.copy_(mean0)
        out["fused"] = env.mppi(mean, SIGMA, it, k, LAM, PENALTY, seed=1, draw_index=0)

    def composed():
        m = mean0.clone()                                                  # [N, H, 2]
        for _ in range(it):
            eps = torch.randn(h, n, k, 2, dtype=torch.float32, device="cuda")
            eps[:, :, 0] = 0.0
            u = torch.minimum(torch.maximum(m.transpose(0, 1)[:, :, None] + sigma * eps.double(), low), high).contiguous()
            la = env.lookahead(u, want=())
            score = torch.where((la.reason & 4) != 0, la.ret - PENALTY, la.ret)
            w = torch.softmax(score / LAM, dim=1)                          # [N, K]
            m = (w[None, :, :, None] * u).sum(dim=2).transpose(0, 1).contiguous()
        out["composed"] = m

    u_fixed = torch.minimum(torch.maximum(mean0.transpose(0, 1)[:, :, None] + sigma *
                                          torch.randn(h, n, k, 2, dtype=torch.float64, device="cuda"), low), high).contiguous()

    def floor():
        for _ in range(it):
            out["la"] = env.lookahead(u_fixed, want=())

    f_txt, f_med = timed(fused)
    c_txt, c_med = timed(composed)
    l_txt, l_med = timed(floor)
    print("N = %d, K = %d, H = %d, I = %d (%d candidate steps): bcp_mppi %s | randn + clip + lookahead + softmax update, I "
          "times %s | I x lookahead alone %s | composition / fused %.2f, fused / floor %.2f | bytes of the composition's "
          "buffers per iteration: %.1f MB, of the fused call: %.3f MB"
          % (n, k, h, it, n * k * h * it, f_txt, c_txt, l_txt, c_med / f_med, f_med / l_med,
             (4 + 8) * 2 * h * n * k / 1e6, 16 * h * n / 1e6), flush=True)
    env.check_errors()
    del env, out, u_fixed, mean, mean0
    torch.cuda.empty_cache()
