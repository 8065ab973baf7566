"""Developer aid: what dynamic thresholding of x0-hat costs inside the replayed sampling step.

Per shape - the latent workload of bench.py (cfg B: num_channels=64, batch 2, 20 frames of 4 x 16 x 16) and the pixel-space
network (128 x 128 x 3, num_channels=128, num_res_blocks=2, batch 1, 20 frames) - one ancestral step, same run, the variants
alternating inside each repeat:

  static          the captured step with the static clamp (head conv fused with the update where the shape allows)
  static_unfused  the same captured with LFVDM_FUSED_HEAD=0: head conv and update as two launches
  dynamic         the captured step under set_dynamic_threshold(0.995): un-fused head + 4 threshold launches + update
  threshold_only  lfvdm_dyn_threshold alone on the dynamic sampler's buffers (device events, back to back)
  eager_fn        p_sample with denoised_fn = dynamic_threshold_reference and clip_denoised=False: the only way to get this
                  behaviour without the native path (an eager model call + elementwise torch ops + a full sort)

and the launches per step of the three captured variants.  overhead = dynamic - static, split into unfuse = static_unfused
- static and threshold = dynamic - static_unfused.  Medians and spreads over ``--repeats`` windows of ``--steps`` steps
(host clock around a synchronised window; threshold_only: device events over ``--calls`` calls).

Without ``--leg`` every shape runs as a child process under its own ``timeout``; the merged result carries the running
code's stamp (abi, source_digest):

    python tools/dyn_threshold_bench.py --out profiles/dyn_threshold_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "latent-flexible-video-diffusion-modeling_amd"))
os.environ.setdefault("LFVDM_TUNE_CACHE", os.path.join(ROOT, "profiles", "tune_cache_mi355x.json"))
LEGS = {"latent": 300, "pixel": 420}      # seconds each leg may take

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=sorted(LEGS), default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--steps", type=int, default=16)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--warmup", type=int, default=6)
ap.add_argument("--percentile", type=float, default=0.995)
ap.add_argument("--out", default=None)
args = ap.parse_args()

if args.leg is None:
    merged = {"tool": "tools/dyn_threshold_bench.py", "repeats": args.repeats, "steps": args.steps, "calls": args.calls,
              "percentile": args.percentile}
    for leg, limit in LEGS.items():
        with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--out", tmp.name,
                   "--repeats", str(args.repeats), "--steps", str(args.steps), "--calls", str(args.calls),
                   "--warmup", str(args.warmup), "--percentile", str(args.percentile)]
            rc = subprocess.call(cmd)
            if rc != 0:      # a failed or hung leg ends the run: nothing more is started on the device
                sys.exit(f"leg {leg} ended with status {rc}")
            res = json.load(open(tmp.name))
            merged.update(res.pop("stamp"))
            merged[leg] = res
    merged["dynamic_faster_than_eager_fn"] = all(merged[k]["dynamic"]["ms"] < merged[k]["eager_fn"]["ms"] for k in LEGS)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")
    print(json.dumps({k: merged[k]["summary"] for k in LEGS}))
    sys.exit(0)

import torch as th  # noqa: E402

import bench  # noqa: E402
from improved_diffusion import _native as nat  # noqa: E402
from improved_diffusion.gaussian_diffusion import dynamic_threshold_reference  # noqa: E402

assert th.cuda.is_available(), "this tool measures on the device"
dev = th.device("cuda:0")
th.cuda.set_device(dev)
med = statistics.median

if args.leg == "latent":
    B, T = 2, 20
    make = lambda: bench.make_model_and_diffusion(64, dev)      # noqa: E731
    inputs = bench.synthetic_inputs(B, T, 0, dev)
    what = "cfg B: num_channels=64, batch 2, 20 frames of 4x16x16"
else:
    B, T = 1, 20
    make = lambda: bench.make_pixel_model(dev, 2)               # noqa: E731
    g = th.Generator().manual_seed(11)
    obs = th.zeros(B, T, 1, 1, 1)
    obs[:, :T // 3] = 1.0
    inputs = {"x0": th.randn(B, T, 3, 128, 128, generator=g).clamp(-1, 1).to(dev), "frame_indices": th.arange(T)[None].to(dev),
              "obs_mask": obs.to(dev), "latent_mask": (1.0 - obs).to(dev)}
    what = "pixel space: 128x128x3, num_channels=128, num_res_blocks=2, batch 1, 20 frames"

model, _ = make()
model = model.eval()
shape = tuple(inputs["x0"].shape)
th.manual_seed(3)
start = th.randn(*shape, device=dev)


def captured(threshold, fused_head):
    """A sampler of its own diffusion object, begun and warmed up; the environment is read at capture"""
    _, diffusion = make()
    if threshold:
        diffusion.set_dynamic_threshold(args.percentile)
    os.environ["LFVDM_FUSED_HEAD"] = "1" if fused_head else "0"
    s = diffusion._graph_sampler(model, shape, True)
    s.begin(start.clone(), inputs)
    os.environ.pop("LFVDM_FUSED_HEAD")
    for _ in range(args.warmup):
        s.step(s.expected_t)
    return s, diffusion


samplers = {"static": captured(False, True), "static_unfused": captured(False, False), "dynamic": captured(True, True)}
dyn, diff_dyn = samplers["dynamic"]
_, diff_eager = make()
lm = inputs["latent_mask"]
fn = lambda p: dynamic_threshold_reference(p, lm, args.percentile, None)      # noqa: E731
state = {"x": start.clone(), "t": th.full((B,), diff_eager.num_timesteps - 1, device=dev, dtype=th.long)}


def eager_step():
    with th.no_grad():
        state["x"] = diff_eager.p_sample(model, state["x"], state["t"], clip_denoised=False, denoised_fn=fn,
                                         model_kwargs=inputs)["sample"]
    state["t"] = (state["t"] - 1).clamp(min=0)


def window(step):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    th.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / args.steps


def threshold_only():
    recip, recipm1, _, _, _, _, M = dyn.update
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    th.cuda.synchronize()
    e0.record()
    for _ in range(args.calls):
        nat.dyn_threshold(dyn.plan.x_in, dyn.plan.out, dyn.t_buf, recip, recipm1, M, False, dyn.frame_mask, dyn.threshold[0],
                          dyn.threshold[1], dyn.xhat, dyn.dyn_stats, dyn.dyn_ws)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / args.calls


for _ in range(2):
    eager_step()
threshold_only()
variants = {k: (lambda s=s: s.step(s.expected_t)) for k, (s, _) in samplers.items()}
times = {k: [] for k in list(variants) + ["eager_fn", "threshold_only"]}
for _ in range(args.repeats):
    for k, step in variants.items():
        times[k].append(window(step))
    times["eager_fn"].append(window(eager_step))
    times["threshold_only"].append(threshold_only())
res = {"what": what, "shape": list(shape), "elements_per_sample": int(start[0].numel())}
for k, v in times.items():
    res[k] = {"ms": round(med(v), 4), "spread_ms": round(max(v) - min(v), 4)}
for k, (s, _) in samplers.items():
    res[k]["launches_per_step"] = len(s.plan.steps) + s.extra_launches
    res[k]["head_fused"] = bool(s.plan.head_fused)
ms = {k: res[k]["ms"] for k in times}
res["summary"] = {"overhead_ms": round(ms["dynamic"] - ms["static"], 4), "unfuse_ms": round(ms["static_unfused"] - ms["static"], 4),
                  "threshold_ms": round(ms["dynamic"] - ms["static_unfused"], 4), "threshold_only_ms": ms["threshold_only"],
                  "dynamic_ms": ms["dynamic"], "eager_fn_ms": ms["eager_fn"],
                  "eager_fn_over_dynamic": round(ms["eager_fn"] / ms["dynamic"], 2),
                  "last_s": dyn.dyn_stats[:, 2].tolist(), "finite": bool(th.isfinite(dyn.plan.x_in).all())}
res["stamp"] = {k: v for k, v in bench.running_code_stamp().items() if k in ("abi", "source_digest")}
print(json.dumps(res["summary"]), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
