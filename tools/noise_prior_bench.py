"""Developer aid: what the temporally correlated noise prior costs, in sampling and in training.

  sampling  the latent workload of bench.py (cfg B: num_channels=64, batch 2, 20 frames of 4 x 16 x 16), one replayed
            ancestral step, same run, the variants alternating inside each repeat:
              fused     the default captured step (head conv fused with the update, noise drawn in that launch)
              unfused   the same captured with LFVDM_FUSED_HEAD=0: head conv, then lfvdm_update_rng_x0
              prior     the captured step under set_noise_prior("progressive:2"): un-fused head, lfvdm_noise_prior_fill
                        (draw mode), lfvdm_update_x0
            and, on the prior sampler's buffers, back to back under device events: fill_only (the draw-mode fill),
            normal_only (``noise.normal_()``, the launch the fill replaces in the un-fused torch-noise branch) and
            factor_only (lfvdm_noise_prior_factor, once per chain).
  training  cfg C (num_channels=128, batch 2, 20 of 40 frames, AdamW + EMA, the captured micro-step): ``run_step`` of a
            TrainLoop without and with noise_prior="progressive:2" - one child process each, one after the other: the
            grouped embedding state of ``_backward`` is one per process and a captured training graph holds pointers into
            it, so two captured TrainLoops must not alternate inside one process.

Medians and spreads over ``--repeats`` windows of ``--steps`` steps (host clock around a synchronised window; the *_only
figures: device events over ``--calls`` calls).  Without ``--leg`` every leg runs as a child process under its own
``timeout``; the merged result carries the running code's stamp (abi, source_digest):

    python tools/noise_prior_bench.py --out profiles/noise_prior_bench.json
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
LEGS = {"sampling": 300, "train_independent": 300, "train_prior": 300}      # seconds each leg may take

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=sorted(LEGS), default=None)
ap.add_argument("--legs", default=",".join(LEGS), help="the legs the parent runs, comma separated")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--steps", type=int, default=16)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--warmup", type=int, default=6)
ap.add_argument("--prior", default="progressive:2")
ap.add_argument("--out", default=None)
args = ap.parse_args()

if args.leg is None:
    merged = {"tool": "tools/noise_prior_bench.py", "repeats": args.repeats, "steps": args.steps, "calls": args.calls,
              "prior": args.prior}
    legs = [k for k in LEGS if k in args.legs.split(",")]
    for leg in legs:
        limit = LEGS[leg]
        with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--out", tmp.name,
                   "--repeats", str(args.repeats), "--steps", str(args.steps), "--calls", str(args.calls),
                   "--warmup", str(args.warmup), "--prior", args.prior]
            rc = subprocess.call(cmd)
            if rc != 0:      # a failed or hung leg ends the run: nothing more is started on the device
                sys.exit(f"leg {leg} ended with status {rc}")
            res = json.load(open(tmp.name))
            merged.update(res.pop("stamp"))
            merged[leg] = res
    if "train_independent" in merged and "train_prior" in merged:
        a, b = merged["train_independent"]["step"]["ms"], merged["train_prior"]["step"]["ms"]
        merged["training_summary"] = {"independent_ms": a, "prior_ms": b, "prior_minus_independent_ms": round(b - a, 4)}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")
    print(json.dumps({k: merged[k]["summary"] for k in legs} | {"training": merged.get("training_summary")}))
    sys.exit(0)

import numpy as np  # noqa: E402
import torch as th  # noqa: E402

import bench  # noqa: E402
from improved_diffusion import _native as nat  # noqa: E402

assert th.cuda.is_available(), "this tool measures on the device"
dev = th.device("cuda:0")
th.cuda.set_device(dev)
med = statistics.median


def window(step):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    th.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / args.steps


def events(fn):
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    th.cuda.synchronize()
    e0.record()
    for _ in range(args.calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / args.calls


def finish(res, times):
    for k, v in times.items():
        res.setdefault(k, {}).update({"ms": round(med(v), 4), "spread_ms": round(max(v) - min(v), 4)})
    res["stamp"] = {k: v for k, v in bench.running_code_stamp().items() if k in ("abi", "source_digest")}
    print(json.dumps(res["summary"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if args.leg == "sampling":
    B, T = 2, 20
    model, _ = bench.make_model_and_diffusion(64, dev)
    model = model.eval()
    inputs = bench.synthetic_inputs(B, T, 0, dev)
    shape = tuple(inputs["x0"].shape)
    th.manual_seed(3)
    start = th.randn(*shape, device=dev)

    def captured(prior, fused_head):
        """A sampler of its own diffusion object, begun and warmed up; the environment is read at capture"""
        _, diffusion = bench.make_model_and_diffusion(64, dev)
        if prior:
            diffusion.set_noise_prior(args.prior)
        os.environ["LFVDM_FUSED_HEAD"] = "1" if fused_head else "0"
        s = diffusion._graph_sampler(model, shape, True)
        s.begin(start.clone(), inputs)
        os.environ.pop("LFVDM_FUSED_HEAD")
        for _ in range(args.warmup):
            s.step(s.expected_t)
        return s

    samplers = {"fused": captured(False, True), "unfused": captured(False, False), "prior": captured(True, True)}
    p = samplers["prior"]
    only = {"fill_only": lambda: nat.noise_prior_fill(p.prior_L, p.noise, seed=p.seed, t=p.t_buf),
            "normal_only": lambda: p.noise.normal_(),
            "factor_only": lambda: nat.noise_prior_factor(p.prior_frames, *p.prior, out=p.prior_L)}
    for fn in only.values():
        events(fn)
    variants = {k: (lambda s=s: s.step(s.expected_t)) for k, s in samplers.items()}
    times = {k: [] for k in list(variants) + list(only)}
    for _ in range(args.repeats):
        for k, step in variants.items():
            times[k].append(window(step))
        for k, fn in only.items():
            times[k].append(events(fn))
    res = {"what": "cfg B: num_channels=64, batch 2, 20 frames of 4x16x16", "shape": list(shape),
           "noise_bytes": 4 * int(start.numel())}
    for k, s in samplers.items():
        res[k] = {"launches_per_step": len(s.plan.steps) + s.extra_launches, "head_fused": bool(s.plan.head_fused)}
    ms = {k: med(v) for k, v in times.items()}
    res["summary"] = {"fused_ms": round(ms["fused"], 4), "unfused_ms": round(ms["unfused"], 4), "prior_ms": round(ms["prior"], 4),
                      "prior_minus_unfused_ms": round(ms["prior"] - ms["unfused"], 4),
                      "prior_minus_fused_ms": round(ms["prior"] - ms["fused"], 4),
                      "fill_only_ms": round(ms["fill_only"], 4), "normal_only_ms": round(ms["normal_only"], 4),
                      "factor_only_ms": round(ms["factor_only"], 4), "finite": bool(th.isfinite(p.plan.x_in).all())}
    finish(res, times)
else:
    from improved_diffusion.train_util import TrainLoop

    def make_loop(prior):
        model, diffusion = bench.make_model_and_diffusion(128, dev)
        model.train()
        th.manual_seed(99)
        np.random.seed(99)
        return TrainLoop(model=model, diffusion=diffusion, data=bench.synthetic_video_stream(2, 40, 4321), batch_size=2,
                         microbatch=-1, lr=1e-4, ema_rate="0.9999", log_interval=10 ** 9, save_interval=10 ** 9,
                         resume_checkpoint="", use_fp16=False, diffusion_space_kwargs={}, fp16_scale_growth=1e-3,
                         schedule_sampler=None, weight_decay=0.0, lr_anneal_steps=0, sample_interval=None,
                         pad_with_random_frames=True, max_frames=20, enc_dec_chunk_size=20,
                         args=argparse.Namespace(resume_id=""), noise_prior=prior)

    prior = args.prior if args.leg == "train_prior" else "none"
    loop = make_loop(prior)

    def step():
        loop.run_step()
        loop.step += 1

    for _ in range(args.warmup):
        step()
    times = {"step": [window(step) for _ in range(args.repeats)]}
    th.cuda.synchronize()
    res = {"what": "cfg C: num_channels=128, batch 2, 20 of 40 frames, AdamW + EMA, one optimizer step", "noise_prior": loop.noise_prior,
           "graph_replayed": loop._graph_state.get("graph") is not None}
    res["summary"] = {"step_ms": round(med(times["step"]), 4), "noise_prior": loop.noise_prior,
                      "finite": bool(th.isfinite(loop.arena.p).all())}
    finish(res, times)
