"""Developer aid: what the variational-bound paths cost at the bench configuration (BASELINE.json configs[1]: ch64, batch 2,
20 frames, 4x16x16), in ONE process, ``--repeats`` times (default 5), medians and spreads:

  (a) ms per replayed evaluation step of ``calc_bpd_loop`` (BpdEvaluator) against ms per eager evaluation step (one model
      call and one fused launch per step) and against the replayed ancestral sampling step, all on respacing 250.  The
      sampling step is measured HERE, in the same process and on the same schedule, as ``bench.py`` measures its
      ``ms_per_step`` (whole chain, K steps per graph launch, GPU events); the headline figure of the parent commit itself
      comes from ``bench.py --gpus 1 --steps K --warmup W`` run next to this tool (DESIGN.md §4 records both);
  (b) the two kernels alone, lfvdm_vb_terms (with both MSEs) and lfvdm_vb_terms_bwd, at the bench shape and at a large one
      (batch 64): microseconds, achieved bandwidth (bytes the launch must move / time) and its share of the HBM peak that
      ``bench.py --full`` reports against (``bench.HBM_PEAK_GBS``), next to that report's own memory-bound phases at the
      bench shape (``bench.hbm_phases_latent``: q_sample, masked_mse);
  (c) with ``--train``: ms per optimizer step (TrainLoop.run_step, captured micro-step) of a use_kl=True diffusion against the
      MSE diffusion on the same model.

Run it under a time limit:

    timeout -k 10 600 python tools/vb_bench.py [--repeats 5] [--train]
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
from improved_diffusion import _native as nat, script_util as su  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--train", action="store_true")
args = ap.parse_args()

dev = th.device("cuda:0")
model, _ = bench.make_model_and_diffusion(64, dev)
inputs = bench.synthetic_inputs(2, 20, 0, dev)
shape = (2, 20, 4, 16, 16)
PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
diff = su.create_gaussian_diffusion(steps=1000, timestep_respacing="250", diffusion_space_kwargs=dict(PIXEL))
n = diff.num_timesteps
med = statistics.median


def timed(fn):
    th.cuda.synchronize()
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


th.manual_seed(0)
x0 = 0.8 * th.randn(*shape, device=dev)
ev = diff._bpd_evaluator(model, shape, True)


def replayed():
    ev.begin(x0, inputs)
    ms = timed(lambda: [ev.step(i) for i in range(n - 1, -1, -1)]) / n
    assert not ev.chain_timed_out()
    return ms


def eager():
    return timed(lambda: diff.calc_bpd_loop(lambda *a, **k: model(*a, **k), x0, model_kwargs=inputs)) / n


def sampling():
    s = diff._graph_sampler(model, shape, True)
    s.begin(th.randn(*shape, device=dev), inputs)
    ms = timed(lambda: s.run(n - 1, n)) / n
    assert not s.chain_timed_out()
    return ms


legs = {"bpd replayed": replayed, "bpd eager": eager, "sampling step": sampling}
for fn in legs.values():      # builds, tunes and captures; not timed
    fn()
res = {k: [] for k in legs}
for _ in range(args.repeats):
    for k, fn in legs.items():
        res[k].append(fn())
print(f"(a) respacing 250, {args.repeats} repeats, ms per step: median (spread)")
for k, v in res.items():
    print(f"    {k:<16}{med(v):>9.4f} ({max(v) - min(v):.4f})   x sampling step {med(v) / med(res['sampling step']):.3f}", flush=True)
print(f"    replayed evaluation step launches: {len(ev.plan.steps)} (plan) + 4 (tick, noise, q_sample, term)")

print(f"(b) the kernels alone: microseconds (median of 20 timed launches of 50), bytes moved, achieved GB/s, share of the "
      f"{bench.HBM_PEAK_GBS:.0f} GB/s HBM peak of bench.py --full")
# (its timesteps go up to 801: the unspaced 1000-step tables)
for k, rec in bench.hbm_phases_latent(su.create_gaussian_diffusion(steps=1000, diffusion_space_kwargs=dict(PIXEL)), dev).items():
    print(f"    bench.py --full {k:<14} B=2          {rec['us']:>8.2f} us  {rec['bytes'] / 1e6:>7.2f} MB  {rec['gb_per_s']:>8.1f} GB/s  "
          f"{100 * rec['frac']:.2f} %", flush=True)
tabs = diff._vb_tables(dev)
for B in (2, 64):
    shp = (B,) + shape[1:]
    xs, xt, out, nz = (th.randn(*shp, device=dev) for _ in range(4))
    g = th.ones(B, device=dev)
    d = th.empty_like(xs)
    vb, xm, em = (th.empty(B, device=dev) for _ in range(3))
    for tname, t in (("t>0", th.full((B,), 100, device=dev, dtype=th.int64)), ("t=0", th.zeros(B, device=dev, dtype=th.int64))):
        fwd = lambda: nat.vb_terms(xs, xt, out, nz, t, *tabs, None, nat.MEAN_EPS, True, vb, xm, em)      # noqa: E731
        bwd = lambda: nat.vb_terms_bwd(xs, xt, out, t, *tabs[:4], tabs[5], None, g, nat.MEAN_EPS, False, d)      # noqa: E731
        for name, fn, streams in (("lfvdm_vb_terms", fwd, 4), ("lfvdm_vb_terms_bwd", bwd, 4)):
            fn()
            us = med([timed(lambda: [fn() for _ in range(50)]) / 50 * 1e3 for _ in range(20)])
            nbytes = streams * xs.numel() * 4
            print(f"    {name:<20} B={B:<3} {tname:<6} {us:>8.2f} us  {nbytes / 1e6:>7.2f} MB  {nbytes / us / 1e3:>8.1f} GB/s  "
                  f"{100 * nbytes / us / 1e3 / bench.HBM_PEAK_GBS:.2f} %", flush=True)

if args.train:
    from improved_diffusion import dist_util  # noqa: E402
    from improved_diffusion.train_util import TrainLoop  # noqa: E402
    dist_util.setup_dist()

    def videos(B, T, seed=0):
        gen = th.Generator().manual_seed(seed)
        while True:
            yield (th.randn(B, T, 4, 16, 16, generator=gen).clamp(-1, 1), {})

    def make_loop(m, diffusion):
        return TrainLoop(model=m, diffusion=diffusion, data=videos(2, 40), batch_size=2, microbatch=-1, lr=1e-4, ema_rate="0.9999",
                         log_interval=10 ** 9, save_interval=10 ** 9, resume_checkpoint="", use_fp16=False,
                         diffusion_space_kwargs={}, fp16_scale_growth=1e-3, schedule_sampler=None, weight_decay=0.0,
                         lr_anneal_steps=0, sample_interval=None, pad_with_random_frames=True, max_frames=20,
                         enc_dec_chunk_size=20, args=argparse.Namespace(resume_id=""))
    print("(c) optimizer step (TrainLoop.run_step, batch 2 x 20 frames, captured micro-step), ms: median (spread)")
    for name, kw in (("mse", {}), ("use_kl", {"use_kl": True}), ("mse", {}), ("use_kl", {"use_kl": True})):
        m, _ = bench.make_model_and_diffusion(64, dev)
        loop = make_loop(m.train(), su.create_gaussian_diffusion(steps=1000, rescale_timesteps=True,
                                                                 diffusion_space_kwargs=dict(PIXEL), **kw))
        for _ in range(4):
            loop.run_step()
            loop.step += 1
        ms = []
        for _ in range(10):
            ms.append(timed(loop.run_step))
            loop.step += 1
        print(f"    {name:<8}{med(ms):>9.3f} ({max(ms) - min(ms):.3f})", flush=True)
