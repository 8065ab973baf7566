"""Developer aid: what the video prediction metrics cost on the device, native launch pair (lfvdm_frame_metrics) against the
same definition composed from PyTorch ops (separable Gaussian filters of the five maps through conv2d and the elementwise
SSIM expression, float32), at an evaluation's size: 10 samples x 8 videos x 100 frames of 3 x 64 x 64 and of 3 x 128 x 128,
float32 in [-1, 1] and uint8.  The two alternate inside each repeat; medians and spreads over ``--repeats`` (default 7) timed
windows of ``--calls`` calls each, device events.  Also printed: the bytes one pass must move (every pixel of pred once, truth
once per sample: it is re-read through the cache), the achieved rate of the native pair, and the largest difference of the
two results.

    timeout -k 10 600 python tools/video_metrics_bench.py [--repeats 7] [--calls 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-flexible-video-diffusion-modeling_amd"))
import torch as th  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from improved_diffusion import video_metrics as vm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert th.cuda.is_available(), "this tool measures on the device"
dev = th.device("cuda:0")
med = statistics.median


def timed(fn, calls):
    th.cuda.synchronize()
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def composed(pred, truth, lo, hi):
    """frame_metrics from torch ops in float32 on the device, one sample at a time (bounds the temporaries)"""
    g = vm._window(th.float32, pred.device)
    gh, gv = g.view(1, 1, 1, -1), g.view(1, 1, -1, 1)
    blur = lambda a: F.conv2d(F.conv2d(a, gh), gv)      # noqa: E731
    K, lead, (C, H, W) = pred.shape[0], pred.shape[1:-3], pred.shape[-3:]
    y = ((truth.float() - lo) / (hi - lo)).reshape(-1, 1, H, W)
    my, yy = blur(y), blur(y * y)
    mse, ssim = [], []
    for k in range(K):
        x = ((pred[k].float() - lo) / (hi - lo)).reshape(-1, 1, H, W)
        mx = blur(x)
        sxx, syy, sxy = blur(x * x) - mx * mx, yy - my * my, blur(x * y) - mx * my
        m = (2 * mx * my + vm.C1) * (2 * sxy + vm.C2) / ((mx * mx + my * my + vm.C1) * (sxx + syy + vm.C2))
        ssim.append(m.mean(dim=(1, 2, 3)).view(*lead, C).mean(-1))
        mse.append(((x - y) ** 2).mean(dim=(1, 2, 3)).view(*lead, C).mean(-1))
    return th.stack(mse), th.stack(ssim)


rows = []
K, B, T, C = 10, 8, 100, 3
for side in (64, 128):
    for dtype in (th.float32, th.uint8):
        gen = th.Generator(device=dev).manual_seed(side)
        base = th.rand(B, T, C, side, side, device=dev, generator=gen)
        base = F.avg_pool2d(base.view(-1, 1, side, side), 7, 1, 3).view(B, T, C, side, side)
        noisy = (base.unsqueeze(0) + 0.05 * th.randn(K, B, T, C, side, side, device=dev, generator=gen)).clamp(0, 1)
        if dtype == th.uint8:
            pred, truth, lo, hi = (255 * noisy).round().to(th.uint8), (255 * base).round().to(th.uint8), 0.0, 255.0
        else:
            pred, truth, lo, hi = 2 * noisy - 1, 2 * base - 1, -1.0, 1.0
        del noisy, base
        native = lambda: vm.frame_metrics(pred, truth)      # noqa: E731
        torch_ops = lambda: composed(pred, truth, lo, hi)      # noqa: E731
        a, b = native(), torch_ops()      # warm-up of both, and the comparison
        dm = float((a["mse"] / b[0] - 1).abs().max())
        ds = float((a["ssim"] - b[1]).abs().max())
        tn, tt = [], []
        for _ in range(args.repeats):
            tn.append(timed(native, args.calls))
            tt.append(timed(torch_ops, args.calls))
        nbytes = (pred.numel() + truth.numel()) * pred.element_size()
        row = {"shape": [K, B, T, C, side, side], "dtype": str(dtype).replace("torch.", ""), "native_ms": med(tn),
               "native_spread_ms": max(tn) - min(tn), "torch_ms": med(tt), "torch_spread_ms": max(tt) - min(tt),
               "speedup": med(tt) / med(tn), "bytes": nbytes, "native_gb_per_s": nbytes / med(tn) / 1e6,
               "max_rel_mse_diff": dm, "max_abs_ssim_diff": ds}
        rows.append(row)
        print(f"{K}x{B}x{T} frames of {C}x{side}x{side} {row['dtype']:<8} native {row['native_ms']:8.3f} ms "
              f"({row['native_spread_ms']:.3f})  torch ops {row['torch_ms']:8.3f} ms ({row['torch_spread_ms']:.3f})  "
              f"x{row['speedup']:.2f}  {nbytes / 1e6:.0f} MB at {row['native_gb_per_s']:.0f} GB/s  "
              f"mse differs by {dm:.1e} (rel), ssim by {ds:.1e}", flush=True)
        del pred, truth
        th.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/video_metrics_bench.py", "repeats": args.repeats, "calls": args.calls, "rows": rows}, f, indent=1)
        f.write("\n")
