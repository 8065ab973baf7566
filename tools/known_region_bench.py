"""Developer aid: what the known-region blend costs a replayed sampling step.  The bench configuration (BASELINE.json
configs[1]: ch64, batch 2, 20 frames, 4x16x16) at respacing 250: the plain ancestral and DDIM (eta = 0) samplers ("off")
against their known-region twins ("on": fresh in-kernel noise under the ancestral rule, fixed noise under DDIM) - GPU-event
time of the whole replayed chain (K steps per graph launch) per step.  Beside it the two stand-alone launches the step's
tail can be compared with, lfvdm_update_rng_x0 and lfvdm_known_blend at the same shape, each as a captured graph of 200
launches.  All legs run in one process, alternating, ``--repeats`` times (default 7); medians are reported, and the spread
(max - min) of the plain ancestral repeats is the yardstick for "no slower".  On a tree without known-region sampling only
the "off" legs run: the same script measures the commit before.

    python tools/known_region_bench.py [--repeats 7]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "latent-flexible-video-diffusion-modeling_amd"))
import torch as th  # noqa: E402
import bench  # noqa: E402  (the flagship workload's model and inputs)
from improved_diffusion import script_util as su, _native as nat  # noqa: E402
from improved_diffusion.gaussian_diffusion import GaussianDiffusion  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()

dev = th.device("cuda:0")
model, _ = bench.make_model_and_diffusion(64, dev)
inputs = bench.synthetic_inputs(2, 20, 0, dev)
shape = (2, 20, 4, 16, 16)
PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
diff = su.create_gaussian_diffusion(steps=1000, timestep_respacing="250", diffusion_space_kwargs=dict(PIXEL))
HAVE = hasattr(GaussianDiffusion, "known_region_sample_loop")
RULES = {"ancestral": ("ancestral",), "ddim": ("ddim", 0.0)}
LEGS = [(f"{r} {k}", r, k == "on") for r in RULES for k in (("off", "on") if HAVE else ("off",))]
known = th.randn(*shape, device=dev)
mask = (th.rand(2, 20, 16, 16, device=dev) < 0.5).float()


def chain(rule_name, on):
    """The steps alone: begin() outside the timed region, then the whole chain, GPU events."""
    rule = RULES[rule_name]
    if on:
        fixed = rule_name == "ddim"
        s = diff._known_region_sampler(model, shape, True, rule, fixed)
        s.begin(th.randn(*shape, device=dev), inputs, known=known, known_mask=mask, known_eps=th.randn_like(known) if fixed else None)
    else:
        s = diff._graph_sampler(model, shape, True, rule=rule)
        s.begin(th.randn(*shape, device=dev), inputs)
    th.cuda.synchronize()
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    e0.record()
    s.run(diff.num_timesteps - 1, diff.num_timesteps)
    e1.record()
    e1.synchronize()
    assert not s.chain_timed_out()
    return 1e3 * e0.elapsed_time(e1) / diff.num_timesteps, len(s.plan.steps) + s.extra_launches


def launch_graph(fn, n=200):
    """``fn`` n times in one captured graph -> a callable returning the microseconds per launch of one replay."""
    fn()
    th.cuda.synchronize()
    g = th.cuda.CUDAGraph()
    with th.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()

    def timed():
        th.cuda.synchronize()
        e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / n
    return timed


x, out, z = (th.randn(*shape, device=dev) for _ in range(3))
t = th.full((2,), 125, device=dev, dtype=th.int64)
seed = th.tensor([1234], device=dev, dtype=th.int64)
recip, recipm1, c1, c2, sg, R, M = diff._update_args(dev)
OPS = {"lfvdm_update_rng_x0": launch_graph(lambda: nat.update_rng_x0(x, out, z, t, recip, recipm1, c1, c2, sg, R, M, True, x, seed, out))}
if HAVE:
    tb = diff.known_region_tables(dev)
    OPS["lfvdm_known_blend fresh"] = launch_graph(lambda: nat.known_blend(x, known, mask, t, tb["a"], tb["s"], seed=seed))
    OPS["lfvdm_known_blend fixed"] = launch_graph(lambda: nat.known_blend(x, known, mask, t, tb["a"], tb["s"], eps=z))

th.manual_seed(0)
for _, r, on in LEGS:      # builds, tunes and captures every sampler; not timed
    chain(r, on)
    chain(r, on)
us, launches = {n: [] for n, _, _ in LEGS}, {}
ops = {n: [] for n in OPS}
for _ in range(args.repeats):
    for name, r, on in LEGS:
        v, launches[name] = chain(r, on)
        us[name].append(v)
    for name, f in OPS.items():
        ops[name].append(f())

med = statistics.median
base = us["ancestral off"]
print(f"repeats {args.repeats}; plain ancestral step: median {med(base):.2f} us, spread (max - min) {max(base) - min(base):.2f} us")
print(f"{'leg':<16}{'launches':>9}{'us/step':>10}{'spread':>9}{'on - off':>10}")
for name, r, on in LEGS:
    d = f"{med(us[name]) - med(us[r + ' off']):+.2f}" if on else ""
    print(f"{name:<16}{launches[name]:>9}{med(us[name]):>10.2f}{max(us[name]) - min(us[name]):>9.2f}{d:>10}")
print(f"{'stand-alone launch, 200 per graph':<36}{'us/launch':>10}{'spread':>9}")
for name, v in ops.items():
    print(f"{name:<36}{med(v):>10.2f}{max(v) - min(v):>9.2f}")
print("all us/step:", {k: [round(v, 2) for v in vs] for k, vs in us.items()}, flush=True)
