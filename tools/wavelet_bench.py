"""Developer aid: what the wavelet diffusion space costs and saves on the device.

  kernels  lfvdm_wavelet_encode / _decode and the fused batch preparation (lfvdm_prepare_batch_wavelet) on 8 x 20 frames of
           3 x 128 x 128, float32 and uint8, one and two levels, against the same transform composed from torch ops on the
           device (strided slices, adds, cat; for the batch preparation an index gather first) and - batch preparation only -
           against the two native launches it replaces.  Bytes = every pixel once + every coefficient once, against the HBM
           peak bench.py reports against (``bench.HBM_PEAK_GBS``).  The two alternate inside each repeat; medians and
           spreads over ``--repeats`` windows of ``--calls`` calls, device events.
  train    one TrainLoop optimizer step of the 128 x 128 x 3, num_channels=128, num_res_blocks=1, 20-frame recipe in pixel
           space and in wavelet space (level 1: 12 x 64 x 64, attention at the same 16 x 16 and 8 x 8 maps), same run.
  sample   one captured denoising step of the num_res_blocks=2 network in both spaces, same run.

Without ``--leg`` every leg runs as a child process under its own ``timeout`` and the results are merged into ``--out``:

    python tools/wavelet_bench.py --out profiles/wavelet_bench.json
"""
import argparse
import json
import math
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
LEGS = {"kernels": 240, "train": 420, "sample": 420}      # seconds each leg may take

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=sorted(LEGS), default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--out", default=None)
args = ap.parse_args()

if args.leg is None:
    merged = {"tool": "tools/wavelet_bench.py", "repeats": args.repeats, "calls": args.calls, "steps": args.steps}
    for leg, limit in LEGS.items():
        with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--out", tmp.name,
                   "--repeats", str(args.repeats), "--calls", str(args.calls), "--steps", str(args.steps), "--warmup", str(args.warmup)]
            rc = subprocess.call(cmd)
            if rc != 0:      # a failed or hung leg ends the run: nothing more is started on the device
                sys.exit(f"leg {leg} ended with status {rc}")
            merged[leg] = json.load(open(tmp.name))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch as th  # noqa: E402

import bench  # noqa: E402
from improved_diffusion import _native as nat, wavelet  # noqa: E402

assert th.cuda.is_available(), "this tool measures on the device"
dev = th.device("cuda:0")
th.cuda.set_device(dev)
med = statistics.median


def timed(fn, calls):
    th.cuda.synchronize()
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / calls      # microseconds per call


def compare(variants):
    """{name: fn} -> {name: {"us", "spread_us"}}, the variants alternating inside each repeat"""
    for fn in variants.values():
        fn()
    t = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            t[k].append(timed(fn, args.calls))
    return {k: {"us": round(med(v), 2), "spread_us": round(max(v) - min(v), 2)} for k, v in t.items()}


def unit(x):
    return x.float() * (1.0 / 127.5) - 1.0 if x.dtype == th.uint8 else x


def leg_kernels():
    rows = []
    B, Tp, F, C, H, W = 8, 24, 20, 3, 128, 128
    gen = th.Generator(device=dev).manual_seed(5)
    table = th.zeros(B, F, 4, dtype=th.int32)
    for b in range(B):
        table[b, :, 0] = th.randperm(Tp)[:F].sort().values.int()
        table[b, :, 1] = table[b, :, 0]
        table[b, : F // 3, 2] = 1
        table[b, F // 3:, 3] = 1
    table = table.to(dev)
    rows_idx = table[:, :, 0].long()
    for dtype in (th.float32, th.uint8):
        pool = th.rand(B, Tp, C, H, W, device=dev, generator=gen) * 2 - 1
        if dtype == th.uint8:
            pool = ((pool + 1) * 127.5).round().clamp(0, 255).to(th.uint8)
        frames = pool[:, :F].reshape(B * F, C, H, W).contiguous()
        for L in (1, 2):
            m = 1 << L
            coef = th.empty(B * F, C * m * m, H // m, W // m, device=dev)
            back = th.empty_like(frames)
            batch = th.empty(B, F, C * m * m, H // m, W // m, device=dev)
            gathered = th.empty(B, F, C, H, W, device=dev)
            fi = th.empty(B, F, dtype=th.int64, device=dev)
            obs, lat = th.empty(B, F, 1, 1, 1, device=dev), th.empty(B, F, 1, 1, 1, device=dev)
            nbytes = frames.numel() * (frames.element_size() + 4)
            res = {"encode": compare({"native": lambda: nat.wavelet_encode(frames, coef, L, "range"),
                                      "torch": lambda: wavelet._encode_torch(unit(frames), L, "range")})}
            nat.wavelet_encode(frames, coef, L, "range")
            diff = float((coef - wavelet._encode_torch(unit(frames), L, "range")).abs().max())

            def torch_decode():
                x = wavelet._decode_torch(coef, L, "range")
                return ((x + 1) * 127.5).round().clamp(0, 255).to(th.uint8) if dtype == th.uint8 else x
            res["decode"] = compare({"native": lambda: nat.wavelet_decode(coef, back, L, "range"), "torch": torch_decode})
            variants = {"native": lambda: nat.prepare_batch_wavelet(pool, table, batch, fi, obs, lat, L, "range"),
                        "torch": lambda: wavelet._encode_torch(
                            unit(th.stack([pool[b].index_select(0, rows_idx[b]) for b in range(B)]).view(B * F, C, H, W)), L, "range")}
            if dtype == th.float32:      # lfvdm_prepare_batch gathers floats only

                def two_launches():
                    nat.prepare_batch(pool, table, gathered, fi, obs, lat)
                    nat.wavelet_encode(gathered.view(B * F, C, H, W), coef, L, "range")
                variants["two_native_launches"] = two_launches
            res["batch_prep"] = compare(variants)
            for op, r in res.items():
                us = r["native"]["us"]
                row = {"op": op, "frames": [B * F, C, H, W], "dtype": str(dtype).replace("torch.", ""), "levels": L, "bytes": nbytes,
                       "native_us": us, "native_spread_us": r["native"]["spread_us"], "torch_us": r["torch"]["us"],
                       "torch_spread_us": r["torch"]["spread_us"], "speedup_vs_torch": round(r["torch"]["us"] / us, 2),
                       "native_gb_per_s": round(nbytes / us / 1e3, 1), "hbm_peak_gb_per_s": bench.HBM_PEAK_GBS,
                       "frac_of_hbm_peak": round(nbytes / us / 1e3 / bench.HBM_PEAK_GBS, 4)}
                if "two_native_launches" in r:
                    row["two_native_launches_us"] = r["two_native_launches"]["us"]
                if op == "encode":
                    row["max_abs_diff_vs_torch"] = diff
                rows.append(row)
                print(json.dumps(row), flush=True)
    return {"note": "63 MB (float32) / 39 MB (uint8) per call: the working set fits the 256 MB last-level cache, so a rate "
                    "above what HBM alone sustains is the cache's", "rows": rows}


def make_model(space, num_res_blocks):
    """The 128 x 128 x 3, num_channels=128 network of BASELINE.json configs[4] (``bench.make_pixel_model``), or its level-1
    wavelet-space counterpart: 12 x 64 x 64, attention at the same 16 x 16 and 8 x 8 maps."""
    if space == "pixel":
        return bench.make_pixel_model(dev, num_res_blocks)
    from improved_diffusion import script_util as su
    sp = wavelet.space_args(128, channels=3, levels=1)
    kw = su.model_and_diffusion_defaults()
    kw.update(image_size=sp["image_size"], in_channels=sp["in_channels"], num_channels=128, num_res_blocks=num_res_blocks,
              num_heads=4, attention_resolutions="16,8", diffusion_steps=1000, timestep_respacing="",
              diffusion_space_kwargs=sp["diffusion_space_kwargs"])
    model, diffusion = su.create_model_and_diffusion(**kw)
    g = th.Generator().manual_seed(7)
    with th.no_grad():
        for name, p in model.named_parameters():
            if p.dim() == 1:
                p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.1 * th.randn(p.shape, generator=g))
            else:
                p.copy_(th.randn(p.shape, generator=g) / math.sqrt(p[0].numel()))
    return model.to(dev), diffusion


def train_step(space):
    from improved_diffusion.logger import logger
    from improved_diffusion.train_util import TrainLoop
    model, diffusion = make_model(space, 1)
    model.train()
    g = th.Generator().manual_seed(4321)
    video = th.randn(1, 24, 3, 128, 128, generator=g).clamp(-1, 1)
    loop = TrainLoop(model=model, diffusion=diffusion, data=bench._repeat_batch(video), batch_size=1, microbatch=-1, lr=1e-4,
                     ema_rate="0.9999", log_interval=10 ** 9, save_interval=10 ** 9, resume_checkpoint="", use_fp16=False,
                     diffusion_space_kwargs={}, fp16_scale_growth=1e-3, schedule_sampler=None, weight_decay=0.0,
                     lr_anneal_steps=0, sample_interval=None, pad_with_random_frames=True, max_frames=20,
                     enc_dec_chunk_size=20, args=argparse.Namespace(resume_id=""))
    th.manual_seed(99)
    np.random.seed(99)
    for _ in range(args.warmup):
        loop.run_step()
        loop.step += 1
    windows = []
    for _ in range(3):
        th.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loop.run_step()
            loop.step += 1
        th.cuda.synchronize()
        windows.append(1e3 * (time.perf_counter() - t0) / args.steps)
    loop._flush_loss_log()
    loss = float(logger.name2val.get("loss", float("nan")))
    logger.dumpkvs()
    out = {"space": space, "ms_per_step": round(med(windows), 2), "spread_ms": round(max(windows) - min(windows), 2),
           "params": sum(p.numel() for p in model.parameters()), "last_loss": loss,
           "graph_replay": loop._graph_state.get("graph") is not None,
           "device_batch_prep": loop._device_prep_ok(video)}
    del loop, model
    th.cuda.empty_cache()
    return out


def sample_step(space):
    model, diffusion = make_model(space, 2)
    model.eval()
    B, T = 1, 20
    g = th.Generator().manual_seed(11)
    pixels = th.randn(B, T, 3, 128, 128, generator=g).clamp(-1, 1).to(dev)
    x0 = diffusion.encode(pixels)
    shape = tuple(x0.shape)
    obs = th.zeros(B, T, 1, 1, 1)
    obs[:, :T // 3] = 1.0
    inputs = {"x0": x0, "frame_indices": th.arange(T)[None].to(dev), "obs_mask": obs.to(dev), "latent_mask": (1.0 - obs).to(dev)}
    sampler = diffusion._graph_sampler(model, shape, True)
    th.manual_seed(3)
    sampler.begin(th.randn(*shape, device=dev), inputs)
    for _ in range(args.warmup):
        sampler.step(sampler.expected_t)
    windows = []
    for _ in range(3):
        th.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            sampler.step(sampler.expected_t)
        th.cuda.synchronize()
        windows.append(1e3 * (time.perf_counter() - t0) / args.steps)
    out = {"space": space, "shape": list(shape), "ms_per_step": round(med(windows), 2),
           "spread_ms": round(max(windows) - min(windows), 2), "head_fused": bool(sampler.plan.head_fused),
           "finite": bool(th.isfinite(sampler.plan.x_in).all())}
    del sampler, model
    th.cuda.empty_cache()
    return out


def two_spaces(fn, what):
    rows = [fn("pixel"), fn("wavelet")]
    for r in rows:
        print(json.dumps(r), flush=True)
    return {"what": what, "rows": rows, "wavelet_over_pixel": round(rows[1]["ms_per_step"] / rows[0]["ms_per_step"], 3)}


if args.leg == "kernels":
    result = leg_kernels()
elif args.leg == "train":
    result = two_spaces(train_step, "TrainLoop optimizer step: 128x128x3 frames, 20 frames, batch 1, num_channels=128, "
                                    "num_res_blocks=1; wavelet = level 1, 12x64x64, device batch preparation with the encode inside")
else:
    result = two_spaces(sample_step, "captured ancestral denoising step: 20 frames, batch 1, num_channels=128, "
                                     "num_res_blocks=2; wavelet = level 1, 12x64x64 (decode not included: it runs once per chain)")
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
