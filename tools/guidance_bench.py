"""Developer aid: what classifier-free guidance on the observed frames costs inside the replayed sampling step.

Per shape - the latent workload of bench.py (cfg B: num_channels=64, batch 2, 20 frames of 4 x 16 x 16) and the pixel-space
network (128 x 128 x 3, num_channels=128, num_res_blocks=2, batch 1, 20 frames) - one ancestral step, same run, the variants
alternating inside each repeat:

  guided      the captured step under set_guidance(2.0) at batch B: forward at 2B, un-fused head, combine, update, mirror
  guided_phi  the same under set_guidance(2.0, 0.7): the combine is then two launches (reduce, apply)
  plain       the captured step at batch B with guidance off (head conv fused with the update where the shape allows)
  plain_2b    the captured step at batch 2B with guidance off: the code path of a plain sampler, twice the batch
  eager       the eager composition: two model calls (the window as given, and with obs_mask = 0), torch ops for the
              combination and the x0-model update (``_update_denoised``)

and the launches per step of the four captured variants.  The number to report is guided - plain_2b: the combine, the mirror
and the un-fused head.  Medians and spreads over ``--repeats`` windows of ``--steps`` steps (host clock around a synchronised
window).

Without ``--leg`` every shape runs as a child process under its own ``timeout``; the merged result carries the running
code's stamp (abi, source_digest):

    python tools/guidance_bench.py --out profiles/guidance_bench.json
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
# four live sampler plans per leg, two of them at batch 2B: room for all their timestep tables, so that every variant runs
# the same kind of plan (the pixel leg holds 3 x 5.9 + 3.0 GiB)
os.environ.setdefault("LFVDM_TIME_TABLE_GB", "32")
LEGS = {"latent": 300, "pixel": 420}      # seconds each leg may take

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=sorted(LEGS), default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--steps", type=int, default=16)
ap.add_argument("--warmup", type=int, default=6)
ap.add_argument("--scale", type=float, default=2.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()

if args.leg is None:
    merged = {"tool": "tools/guidance_bench.py", "repeats": args.repeats, "steps": args.steps, "scale": args.scale}
    for leg, limit in LEGS.items():
        with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--out", tmp.name,
                   "--repeats", str(args.repeats), "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--scale", str(args.scale)]
            rc = subprocess.call(cmd)
            if rc != 0:      # a failed or hung leg ends the run: nothing more is started on the device
                sys.exit(f"leg {leg} ended with status {rc}")
            res = json.load(open(tmp.name))
            merged.update(res.pop("stamp"))
            merged[leg] = res
    if args.out:
        with open(args.out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")
    print(json.dumps({k: merged[k]["summary"] for k in LEGS}))
    sys.exit(0)

import torch as th  # noqa: E402

import bench  # noqa: E402
from improved_diffusion.gaussian_diffusion import guidance_reference  # noqa: E402

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
twice = lambda v: th.cat([v, v], dim=0)      # noqa: E731
inputs_2b = {k: twice(v) if v.shape[0] == B else v.expand(2 * B, *v.shape[1:]).contiguous() for k, v in inputs.items()}


def captured(guided, doubled, rescale=0.0):
    """A sampler of its own diffusion object, begun and warmed up"""
    _, diffusion = make()
    if guided:
        diffusion.set_guidance(args.scale, rescale)
    x, kw = (twice(start), inputs_2b) if doubled else (start.clone(), inputs)
    s = diffusion._graph_sampler(model, tuple(x.shape), True)
    s.begin(x, kw)
    for _ in range(args.warmup):
        s.step(s.expected_t)
    return s, diffusion


samplers = {"guided": captured(True, False), "guided_phi": captured(True, False, 0.7), "plain": captured(False, False),
            "plain_2b": captured(False, True)}
_, diff_eager = make()
uncond = dict(inputs, obs_mask=th.zeros_like(inputs["obs_mask"]))
state = {"x": start.clone(), "t": th.full((B,), diff_eager.num_timesteps - 1, device=dev, dtype=th.long)}
net = diff_eager._wrap_model(model) if hasattr(diff_eager, "_wrap_model") else model


def eager_step():
    with th.no_grad():
        x, t = state["x"], state["t"]
        o_c, _ = net(x, diff_eager._scale_timesteps(t), return_attn_weights=False, **inputs)
        o_u, _ = net(x, diff_eager._scale_timesteps(t), return_attn_weights=False, **uncond)
        tb = diff_eager.tables(dev)
        xhat = guidance_reference(x, th.cat([o_c, o_u]), t, args.scale, 0.0, None, tb["sqrt_recip_alphas_cumprod"],
                                  tb["sqrt_recipm1_alphas_cumprod"], dtype=th.float32).clamp(-1, 1)
        _, _, c1, c2, sg, _, _ = diff_eager._update_args(dev)
        v = lambda a: a[t].view(-1, 1, 1, 1, 1)      # noqa: E731
        sigma = ((t != 0).float() * th.exp(0.5 * sg[t])).view(-1, 1, 1, 1, 1)
        state["x"] = v(c1) * xhat + v(c2) * x + sigma * th.randn_like(x)
    state["t"] = (state["t"] - 1).clamp(min=0)


def window(step):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    th.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / args.steps


for _ in range(2):
    eager_step()
variants = {k: (lambda s=s: s.step(s.expected_t)) for k, (s, _) in samplers.items()}
times = {k: [] for k in list(variants) + ["eager"]}
for _ in range(args.repeats):
    for k, step in variants.items():
        times[k].append(window(step))
    times["eager"].append(window(eager_step))
res = {"what": what, "shape": list(shape), "elements_per_sample": int(start[0].numel())}
for k, v in times.items():
    res[k] = {"ms": round(med(v), 4), "spread_ms": round(max(v) - min(v), 4)}
for k, (s, _) in samplers.items():
    res[k]["launches_per_step"] = len(s.plan.steps) + s.extra_launches
    res[k]["head_fused"] = bool(s.plan.head_fused)
    res[k]["plan_batch"] = int(s.plan.B)
ms = {k: res[k]["ms"] for k in times}
gs = samplers["guided"][0]
res["summary"] = {"guided_minus_plain_2b_ms": round(ms["guided"] - ms["plain_2b"], 4),
                  "guided_phi_minus_plain_2b_ms": round(ms["guided_phi"] - ms["plain_2b"], 4),
                  "guided_over_plain": round(ms["guided"] / ms["plain"], 3), "guided_ms": ms["guided"],
                  "guided_phi_ms": ms["guided_phi"], "plain_ms": ms["plain"],
                  "plain_2b_ms": ms["plain_2b"], "eager_ms": ms["eager"], "eager_over_guided": round(ms["eager"] / ms["guided"], 2),
                  "finite": bool(th.isfinite(gs.plan.x_in).all())}
res["stamp"] = {k: v for k, v in bench.running_code_stamp().items() if k in ("abi", "source_digest")}
print(json.dumps(res["summary"]), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
