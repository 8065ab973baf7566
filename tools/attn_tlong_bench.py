"""Developer aid: temporal-attention forward and backward at T = 32 (the per-window kernels) and T = 64 (the long-window
kernels, attention_temporal_long.hip) for the same shapes; run under `rocprofv3 --kernel-trace --stats` for per-kernel
times."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-flexible-video-diffusion-modeling_amd"))
import torch as th
from improved_diffusion import _native as nat

def timeit(fn, reps=20):
    for _ in range(3): fn()
    th.cuda.synchronize()
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); th.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / reps

for C in (64, 128):
    for P in (256, 64, 16, 4):
        res = {}
        for T in (32, 64):
            B, h = 2, 4
            M = B * T * P
            g = lambda *s: th.randn(*s, device="cuda")
            qkv, do = g(M, 3 * C), g(M, C)
            Rq, Rk, Rv = (0.3 * g(B, T, T, C) for _ in range(3))
            mask = (th.rand(B, T, device="cuda") > 0.4).float()
            o = th.empty(M, C, device="cuda")
            ws_p, ws_ds = g(B * P * h * T, T), g(B * P * h * T, T)
            dqkv = th.empty(M, 3 * C, device="cuda")
            dRq, dRk, dRv = (th.empty(B, T, T, C, device="cuda") for _ in range(3))
            fwd = lambda: nat.attn_temporal(qkv, Rq, Rk, Rv, mask, o, None, B, T, P, C, h)
            bwd = lambda: nat.attn_temporal_bwd(qkv, do, Rq, Rk, Rv, mask, ws_p, ws_ds, dqkv, dRq, dRk, dRv, B, T, P, C, h)
            res[T] = (timeit(fwd), timeit(bwd))
        print(f"B=2 C={C} heads=4 P={P}: fwd T=32 {res[32][0]:7.1f} us  T=64 {res[64][0]:7.1f} us ({res[64][0] / res[32][0]:.2f}x)  "
              f"bwd T=32 {res[32][1]:7.1f} us  T=64 {res[64][1]:7.1f} us ({res[64][1] / res[32][1]:.2f}x)", flush=True)
