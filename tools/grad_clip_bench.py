"""Cost of gradient clipping at ch128: `bench.bench_train` - the training leg of `bench.py --full` - of the checkout at
--root, one `PERF {json}` line (optimizer steps/s, ms per step, the optimizer phase's HBM record).  Run it once per
process, alternating checkouts / settings:

    python tools/grad_clip_bench.py --root <parent checkout> --tag parent                 # the commit before
    python tools/grad_clip_bench.py --root . --tag off                                     # clipping off
    LFVDM_MAX_GRAD_NORM=1 python tools/grad_clip_bench.py --root . --tag on --norm-bench   # clipping on

--norm-bench adds the two norm launches alone, on arena-sized buffers rotated through more memory than the 256 MB
Infinity Cache holds (a single 122 MB buffer would be served from it and overstate the HBM rate)."""
import argparse, json, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--root", required=True)
ap.add_argument("--tag", required=True)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--norm-bench", action="store_true")
a = ap.parse_args()
root = os.path.abspath(a.root)
sys.path[:0] = [os.path.join(root, "latent-flexible-video-diffusion-modeling_amd"), root]
os.chdir(root)
import torch as th
import bench
dev = th.device("cuda:0")
out = bench.bench_train(0, 1, dev, a.steps, 4)
rec = {"tag": a.tag, "max_grad_norm_env": os.environ.get("LFVDM_MAX_GRAD_NORM"), "optimizer_steps_per_s": out["optimizer_steps_per_s"],
       "ms_per_step": out["ms_per_step"], "params": out["params"], "hbm_adamw_ema": out.get("hbm_phases", {}).get("adamw_ema")}
if a.norm_bench:
    from improved_diffusion import _native as nat
    n = (out["params"] + 3) // 4 * 4
    bufs = [th.randn(n, device=dev) for _ in range(4)]          # 4 x 4n bytes: past the 256 MB Infinity Cache
    parts = th.empty(nat.grad_norm_nparts(n), device=dev)
    stat = th.zeros(4, device=dev)
    k = [0]
    def both():
        nat.grad_clip_stat(bufs[k[0] % 4], 1.0, 1.0, parts, stat); k[0] += 1
    def partials_only():
        nat.check(nat.lib().lfvdm_grad_norm_partials(bufs[k[0] % 4].data_ptr(), n, 1.0, parts.data_ptr(), parts.numel(), nat.stream()), "p"); k[0] += 1
    def finalize_only():
        nat.check(nat.lib().lfvdm_grad_norm_finalize(parts.data_ptr(), parts.numel(), 1.0, stat.data_ptr(), nat.stream()), "f")
    us_both = bench._event_time_us(both, reps=40, warm=4)
    us_part = bench._event_time_us(partials_only, reps=40, warm=4)
    us_fin = bench._event_time_us(finalize_only, reps=40, warm=4)
    rec["norm_bench"] = {"n": n, "nparts": parts.numel(), "bytes": 4 * n, "us_both": round(us_both, 2), "us_partials": round(us_part, 2),
                         "us_finalize": round(us_fin, 2), "gb_per_s_both": round(4 * n / us_both / 1e3, 1),
                         "gb_per_s_partials": round(4 * n / us_part / 1e3, 1), "frac_of_8000_both": round(4 * n / us_both / 1e3 / 8000, 4),
                         "frac_of_8000_partials": round(4 * n / us_part / 1e3 / 8000, 4)}
print("PERF " + json.dumps(rec), flush=True)
