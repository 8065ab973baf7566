"""Developer aid: what preparing one training micro-batch of the bouncing_shapes dataset costs, at the pixel recipe's shape
(batch 2, 20 of 40 frames, 3 x 128 x 128) and at 3 x 64 x 64.

  rendered   the fused launch pair: the host stages the video indices and the index table (pinned, one H2D copy),
             lfvdm_shapes_trajectories + lfvdm_shapes_render (table mode) write the batch, its frame indices and masks
  host       what the code did before the dataset had kernels: the host reference renders video 1 and the padding video of each
             batch element, the pool (thinned to the named frames above TrainLoop.POOL_WHOLE_VIDEO_BYTES, as _pool_and_table
             does) is staged in pinned memory and copied, lfvdm_prepare_batch gathers.  Reported with and without the render,
             since DataLoader workers can hide the render but not the staging and the copy.

Wall time per micro-batch, host clock around work that ends in a device synchronise; the two alternate inside each repeat;
medians and spreads over ``--repeats`` windows of ``--calls`` calls.  Also: the render launch alone (device events) and the
fraction of the HBM write peak its output bytes amount to - the batch is a few MB and stays in the last-level cache, so this
says how far the launch is from being bound by its stores, not what HBM sustains.

    timeout -k 10 600 python tools/shapes_bench.py [--repeats 7] [--calls 20] [--out profiles/shapes_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "latent-flexible-video-diffusion-modeling_amd")
sys.path.insert(0, PKG)
import numpy as np  # noqa: E402
import torch as th  # noqa: E402
from improved_diffusion import _native as nat, shapes as sh  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert th.cuda.is_available(), "this tool measures on the device"
dev = th.device("cuda:0")
med = statistics.median
HBM_PEAK_GB_S = 8000.0
POOL_WHOLE_VIDEO_BYTES = 2 << 20
B, F, T = 2, 20, 40


def stamp():
    try:
        with open(os.path.join(PKG, "lib", "build_manifest.json")) as f:
            digest = json.load(f).get("source_digest")
    except (OSError, ValueError):
        digest = None
    return {"abi": int(nat.lib().lfvdm_abi_version()), "source_digest": digest}


def make_table(rng):
    """An index table as sample_index_table makes them: sorted frames of video 1, then random frames of the padding video."""
    table = np.zeros((B, F, 4), dtype=np.int32)
    for b in range(B):
        n = int(rng.randint(F // 2, F + 1))
        own, pads = np.sort(rng.choice(T, n, replace=False)), rng.randint(0, T, F - n)
        table[b, :, 0], table[b, :, 1] = np.concatenate([own, T + pads]), np.concatenate([own, pads])
        table[b, :, 2] = rng.randint(0, 2, F)
        table[b, :, 3] = 1 - table[b, :, 2]
    return table


def wall(fn, calls):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(calls):
        fn(i)
    th.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


rows = []
for side in (128, 64):
    params = sh.ShapesParams(H=side, W=side, T=T)
    src = sh.ShapesBatches(sh.BouncingShapes(params, "train"), B).device_source
    lut = src.lut(dev)
    rng = np.random.RandomState(side)
    work = [(rng.randint(0, 4096, B), rng.randint(0, 4096, B), make_table(rng)) for _ in range(args.calls)]
    pin_small = th.empty(B * 2 * 8 + B * F * 16, dtype=th.uint8).pin_memory()
    frame_bytes = 3 * side * side * 4
    whole = 2 * T * frame_bytes <= POOL_WHOLE_VIDEO_BYTES
    Tp = 2 * T if whole else F
    pin_pool = th.empty(B * Tp * frame_bytes + B * F * 16, dtype=th.uint8).pin_memory()
    out = {}

    def rendered(i):
        i1, i2, table = work[i]
        nb = B * 2 * 8
        pin_small[:nb].view(th.int64).copy_(th.from_numpy(np.stack([i1, i2], 1).astype(np.int64)).reshape(-1))
        pin_small[nb:].view(th.int32).copy_(th.from_numpy(table).reshape(-1))
        d = pin_small.to(dev, non_blocking=True)
        out["rendered"] = src.render_table(d[:nb].view(th.int64).view(B, 2), d[nb:].view(th.int32).view(B, F, 4))

    def host_pool(i):
        i1, i2, table = work[i]
        v = sh.uint8_to_float(th.from_numpy(sh.videos_ref(params, "train", np.concatenate([i1, i2]))))
        pool = th.cat([v[:B], v[B:]], dim=1)
        if not whole:
            rows_ = th.from_numpy(table[:, :, 0].astype(np.int64))
            pool = th.stack([pool[b].index_select(0, rows_[b]) for b in range(B)])
            table = table.copy()
            table[:, :, 0] = np.arange(F, dtype=np.int32)[None]
        return pool, table

    def upload_and_gather(pool, table):
        nb = pool.numel() * 4
        pin_pool[:nb].view(th.float32).copy_(pool.reshape(-1))
        pin_pool[nb:].view(th.int32).copy_(th.from_numpy(table).reshape(-1))
        d = pin_pool.to(dev, non_blocking=True)
        dpool, dtable = d[:nb].view(th.float32).view(pool.shape), d[nb:].view(th.int32).view(B, F, 4)
        batch = th.empty(B, F, 3, side, side, device=dev)
        fi = th.empty(B, F, device=dev, dtype=th.int64)
        obs = th.empty(B, F, 1, 1, 1, device=dev)
        lat = th.empty_like(obs)
        nat.prepare_batch(dpool, dtable, batch, fi, obs, lat)
        out["host"] = (batch, fi, obs, lat)

    def host(i):
        upload_and_gather(*host_pool(i))

    prepared = [host_pool(i) for i in range(args.calls)]

    def host_without_render(i):
        upload_and_gather(*prepared[i])

    # warm-up of every path, and the comparison: the same bytes
    rendered(0), host(0)
    th.cuda.synchronize()
    same = all(th.equal(a, b) for a, b in zip(out["rendered"], out["host"]))
    t_r, t_h, t_s = [], [], []
    for _ in range(args.repeats):
        t_r.append(wall(rendered, args.calls))
        t_h.append(wall(host, args.calls))
        t_s.append(wall(host_without_render, args.calls))

    # the render launch alone
    i1, i2, table = work[0]
    vid = th.from_numpy(np.stack([i1, i2], 1).astype(np.int64)).to(dev)
    dtable = th.from_numpy(table).to(dev)
    traj, consts = src.trajectories(vid.reshape(-1))
    batch = th.empty(B, F, 3, side, side, device=dev)
    fi, obs = th.empty(B, F, device=dev, dtype=th.int64), th.empty(B, F, 1, 1, 1, device=dev)
    lat = th.empty_like(obs)

    def launch():
        nat.shapes_render(traj, consts, batch, table=dtable, lut=lut, frame_indices=fi, obs_mask=obs, latent_mask=lat)
    for _ in range(10):
        launch()
    t_k = []
    for _ in range(args.repeats):
        th.cuda.synchronize()
        e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            launch()
        e1.record()
        e1.synchronize()
        t_k.append(e0.elapsed_time(e1) * 1e3 / 200)
    nbytes = batch.numel() * 4
    row = {"shape": [B, F, 3, side, side], "T": T, "same_bytes": bool(same), "rendered_ms": med(t_r),
           "rendered_spread_ms": max(t_r) - min(t_r), "host_ms": med(t_h), "host_spread_ms": max(t_h) - min(t_h),
           "host_without_render_ms": med(t_s), "host_without_render_spread_ms": max(t_s) - min(t_s),
           "pool": "whole videos" if whole else "named frames", "render_launch_us": med(t_k),
           "render_launch_spread_us": max(t_k) - min(t_k), "render_bytes_written": nbytes,
           "render_gb_per_s": nbytes / med(t_k) / 1e3, "hbm_peak_gb_per_s": HBM_PEAK_GB_S,
           "frac_of_hbm_write_peak": nbytes / med(t_k) / 1e3 / HBM_PEAK_GB_S}
    rows.append(row)
    print(f"batch {B} x {F} of {T} frames 3x{side}x{side}: rendered {row['rendered_ms']:.3f} ms ({row['rendered_spread_ms']:.3f})  "
          f"host {row['host_ms']:.3f} ms ({row['host_spread_ms']:.3f})  host without the render {row['host_without_render_ms']:.3f} ms "
          f"({row['host_without_render_spread_ms']:.3f})  same bytes: {same}  render launch {row['render_launch_us']:.2f} us = "
          f"{row['render_gb_per_s']:.0f} GB/s written ({100 * row['frac_of_hbm_write_peak']:.1f} % of {HBM_PEAK_GB_S:.0f})", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/shapes_bench.py", "repeats": args.repeats, "calls": args.calls, "stamp": stamp(), "rows": rows}, f,
                  indent=1)
        f.write("\n")
