"""Developer aid: the replayed step at the bench configuration (BASELINE.json configs[1]: ch64, batch 2, 20 frames, 4x16x16)
of an epsilon sampler and of an x0-prediction sampler (predict_xstart=True) in ONE process, alternating, ``--repeats`` times
(default 5): ms per step of the ancestral chain at respacing 250 and of DDIM (eta = 0) on the same schedule.  Medians are
reported; the spread (max - min) of the epsilon repeats is the yardstick for "equal".  Run it under a time limit:

    timeout -k 10 600 python tools/xstart_bench.py [--repeats 5]
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
from improved_diffusion import script_util as su  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

dev = th.device("cuda:0")
model, _ = bench.make_model_and_diffusion(64, dev)
inputs = bench.synthetic_inputs(2, 20, 0, dev)
shape = (2, 20, 4, 16, 16)
PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
RULES = [("ancestral", ("ancestral",)), ("ddim", ("ddim", 0.0))]
LEGS = [(f"{mean}/{rn}", px, rule) for rn, rule in RULES for mean, px in (("eps", False), ("x0", True))]
diffs = {name: su.create_gaussian_diffusion(steps=1000, timestep_respacing="250", predict_xstart=px,
                                            diffusion_space_kwargs=dict(PIXEL)) for name, px, _ in LEGS}


def chain(name, rule):
    """begin() outside the timed region, then the whole chain (K steps per graph launch), GPU events -> ms per step."""
    d = diffs[name]
    s = d._graph_sampler(model, shape, True, rule=rule)
    s.begin(th.randn(*shape, device=dev), inputs)
    th.cuda.synchronize()
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    e0.record()
    s.run(d.num_timesteps - 1, d.num_timesteps)
    e1.record()
    e1.synchronize()
    assert not s.chain_timed_out()
    return e0.elapsed_time(e1) / d.num_timesteps, len(s.plan.steps) + s.extra_launches


th.manual_seed(0)
launches = {}
for name, _, rule in LEGS:      # builds, tunes and captures every sampler; not timed
    chain(name, rule)
    launches[name] = chain(name, rule)[1]
step_ms = {n: [] for n, _, _ in LEGS}
for _ in range(args.repeats):
    for name, _, rule in LEGS:
        step_ms[name].append(chain(name, rule)[0])

med = statistics.median
print(f"repeats {args.repeats}")
print(f"{'leg':<16}{'launches':>9}{'ms/step':>10}{'spread':>10}{'x0 - eps':>10}")
for name, _, rule in LEGS:
    v = step_ms[name]
    ref = step_ms["eps/" + name.split("/")[1]]
    print(f"{name:<16}{launches[name]:>9}{med(v):>10.4f}{max(v) - min(v):>10.4f}{med(v) - med(ref):>+10.4f}", flush=True)
print("all ms/step:", {k: [round(v, 4) for v in vs] for k, vs in step_ms.items()})
