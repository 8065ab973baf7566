"""Developer aid: one window at the bench configuration (BASELINE.json configs[1]: ch64, batch 2, 20 frames, 4x16x16) with
the ancestral chain at respacing 250 and with DDIM (eta = 0) at ddim50 and ddim25 - ms per step and ms per window, the
table build of ``begin()`` included and shown on its own.  ``ddim250`` is DDIM on the ancestral leg's own 250-step schedule:
the like-for-like step.  All legs run in one process, alternating, ``--repeats`` times (default 5); medians are reported,
and the spread (max - min) of the ancestral repeats is the yardstick for "not slower".

    python tools/ddim_bench.py [--repeats 5]
"""
import argparse
import os
import statistics
import sys
import time

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
LEGS = [("ancestral250", "250", ("ancestral",)), ("ddim250", "250", ("ddim", 0.0)), ("ddim50", "ddim50", ("ddim", 0.0)),
        ("ddim25", "ddim25", ("ddim", 0.0))]
diffs = {name: su.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, diffusion_space_kwargs=dict(PIXEL))
         for name, resp, _ in LEGS}


def window(name, rule):
    """One whole window through the public loop (begin + chain + the final clone), host wall clock around a synchronise."""
    d = diffs[name]
    th.cuda.synchronize()
    t0 = time.perf_counter()
    if rule[0] == "ddim":
        d.ddim_sample_loop(model, shape, model_kwargs=inputs, eta=rule[1], return_decoded=False)
    else:
        d.p_sample_loop(model, shape, model_kwargs=inputs, return_decoded=False)
    th.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def chain(name, rule):
    """The steps alone: begin() outside the timed region, then the whole chain (K steps per graph launch), GPU events."""
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
    return e0.elapsed_time(e1) / d.num_timesteps, s.table_build_ms


th.manual_seed(0)
for name, _, rule in LEGS:      # builds, tunes and captures every sampler; not timed
    window(name, rule)
    window(name, rule)
step_ms, table_ms, window_ms = ({n: [] for n, _, _ in LEGS} for _ in range(3))
for _ in range(args.repeats):
    for name, _, rule in LEGS:
        ms, tb = chain(name, rule)
        step_ms[name].append(ms)
        table_ms[name].append(tb)
    for name, _, rule in LEGS:
        window_ms[name].append(window(name, rule))

med = statistics.median
anc = step_ms["ancestral250"]
print(f"repeats {args.repeats}; ancestral step: median {med(anc):.4f} ms, spread (max - min) {max(anc) - min(anc):.4f} ms")
print(f"{'leg':<14}{'steps':>6}{'ms/step':>10}{'vs anc':>10}{'ms/window':>11}{'table build ms':>16}{'share':>8}")
for name, _, rule in LEGS:
    n = diffs[name].num_timesteps
    w, tb = med(window_ms[name]), med(table_ms[name])
    print(f"{name:<14}{n:>6}{med(step_ms[name]):>10.4f}{med(step_ms[name]) - med(anc):>+10.4f}{w:>11.2f}{tb:>16.3f}"
          f"{100 * tb / w:>7.1f}%", flush=True)
print("all ms/step:", {k: [round(v, 4) for v in vs] for k, vs in step_ms.items()})
print("all ms/window:", {k: [round(v, 2) for v in vs] for k, vs in window_ms.items()})
