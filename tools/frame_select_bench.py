"""Developer aid: what choosing the conditioning frames of the adaptive sampling schemes costs on the device.  The whole
index sequence of ``adaptive-autoreg`` and of ``adaptive-hierarchy-2`` with ``just_get_indices=True`` (no network runs: every
window copies its frames from the given video), T = 1000 frames, windows of K = 20 with 10 new frames, B = 8 videos of
4 x 16 x 16 (a latent) and of 3 x 128 x 128 (pixels), by two routes in the same run:

  native   ``sample_video(adaptive_metric="msl2:1")``: the cached distance matrix (lfvdm_frame_dist_rows for the frames that became
           done) and one selection launch per window (lfvdm_fps_select), one device-to-host copy of the picks; also timed with
           "msl2:3" (the three-level kernel; the embedding route has no counterpart of it here);
  embed    what the schemes did before the metric existed: an identity ``embed_fn`` (every finished frame re-stacked per window)
           and the Python loop over videos and picks with one ``.cpu()`` per (video, pick).  ``sample_video`` has no argument
           for an ``embed_fn``, so ``drive`` below repeats its ``just_get_indices`` window loop around a scheme built here; the
           warm-up checks that ``drive`` with the metric gives the windows of ``sample_video`` with the metric.

Host clock around the whole sequence, ending in a device synchronise; the routes alternate inside each repeat.  Both times
contain the same window gathers and scatters.  Also recorded: windows, and in how many of them the two routes chose different
frames for some video (float32 sums in another order: near-ties may flip; msl2:1 and the identity embedding rank alike
otherwise).

    timeout -k 10 1100 python tools/frame_select_bench.py [--repeats 5] [--frames 1000] [--out profiles/frame_select_bench.json]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-flexible-video-diffusion-modeling_amd"))
import torch as th  # noqa: E402
from improved_diffusion.sampling_schemes import sampling_schemes  # noqa: E402
from improved_diffusion.video_sampler import default_sampling_args, sample_video, window_inputs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_select_bench.json"))
args = ap.parse_args()
assert th.cuda.is_available(), "this tool measures on the device"
dev = th.device("cuda:0")
B, K, STEP, N_OBS = 8, 20, 10, 36


def identity_embed(vids, idx):
    return th.stack([vids[:, i].flatten(1) for i in idx], dim=1)


def picks_of(used):
    return [[list(map(int, o)) for o in obs] for obs, _ in used]


def timed(fn):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        used = fn()
    th.cuda.synchronize()
    return time.perf_counter() - t0, picks_of(used)


def via_sample_video(name, video, metric):
    a = default_sampling_args(sampling_scheme=name, n_obs=N_OBS, max_frames=K, max_latent_frames=STEP, device="cuda:0",
                              adaptive_metric=metric)
    return sample_video(a, None, None, video, just_get_indices=True, verbose=False)[1]


def drive(name, video, metric=None, embed_fn=None):
    """The ``just_get_indices`` window loop of ``sample_video`` around a scheme configured here."""
    T = video.shape[1]
    scheme = iter(sampling_schemes[name](video_length=T, num_obs=N_OBS, max_frames=K, step_size=STEP))
    if metric is not None:
        scheme.set_frame_metric(metric)
    if embed_fn is not None:
        scheme.set_embed_fn(embed_fn)
    samples = th.zeros_like(video, memory_format=th.contiguous_format)
    samples[:, :N_OBS] = video[:, :N_OBS]
    rows = th.arange(video.shape[0], device=video.device)[:, None]
    used = []
    while True:
        scheme.set_videos(samples)
        try:
            obs_idx, lat_idx = next(scheme)
        except StopIteration:
            break
        frame_indices = window_inputs(samples, obs_idx, lat_idx, video.device)[0]
        n_lat = len(lat_idx[0])
        local = video[rows, frame_indices]
        samples[rows, frame_indices[:, -n_lat:]] = local[:, -n_lat:]
        used.append((obs_idx, lat_idx))
    return used


rows_out = []
for shape in ((4, 16, 16), (3, 128, 128)):
    gen = th.Generator(device=dev).manual_seed(shape[1])
    video = th.randn(B, args.frames, *shape, device=dev, generator=gen).mul_(0.3).cumsum_(dim=1)      # a random walk
    short = video[:, :100].contiguous()
    for name in ("adaptive-autoreg", "adaptive-hierarchy-2"):
        # warm-up of every route (code objects, allocator), and the driver against sample_video
        w = timed(lambda: via_sample_video(name, short, "msl2:1"))[1]
        assert timed(lambda: drive(name, short, metric="msl2:1"))[1] == w, "drive() is not sample_video's window loop"
        timed(lambda: via_sample_video(name, short, "msl2:3"))
        timed(lambda: drive(name, short, embed_fn=identity_embed))
        tn, t3, te = [], [], []
        for _ in range(args.repeats):
            t, picks_n = timed(lambda: via_sample_video(name, video, "msl2:1"))
            tn.append(t)
            t, picks_e = timed(lambda: drive(name, video, embed_fn=identity_embed))
            te.append(t)
            t3.append(timed(lambda: via_sample_video(name, video, "msl2:3"))[0])
        differ = sum(1 for x, y in zip(picks_n, picks_e) if x != y)
        med = statistics.median
        row = {"scheme": name, "frame": list(shape), "B": B, "T": args.frames, "K": K, "step": STEP, "n_obs": N_OBS,
               "windows": len(picks_n), "native_s": med(tn), "native_spread_s": max(tn) - min(tn),
               "native_msl2_3_s": med(t3), "native_msl2_3_spread_s": max(t3) - min(t3),
               "embed_s": med(te), "embed_spread_s": max(te) - min(te), "speedup": med(te) / med(tn),
               "saved_ms_per_window": 1e3 * (med(te) - med(tn)) / len(picks_n), "windows_with_different_picks": differ}
        rows_out.append(row)
        print(f"{name:<22} {B} x {args.frames} frames of {'x'.join(map(str, shape)):<10} {row['windows']} windows: native msl2:1 "
              f"{row['native_s']:.3f} s ({row['native_spread_s']:.3f})  msl2:3 {row['native_msl2_3_s']:.3f} s "
              f"({row['native_msl2_3_spread_s']:.3f})  identity embed_fn + host loop {row['embed_s']:.3f} s "
              f"({row['embed_spread_s']:.3f})  x{row['speedup']:.1f}  {row['saved_ms_per_window']:.2f} ms per window saved  "
              f"different picks in {differ} windows", flush=True)
    del video, short
    th.cuda.empty_cache()
with open(args.out, "w") as f:
    json.dump({"tool": "tools/frame_select_bench.py", "repeats": args.repeats, "rows": rows_out}, f, indent=1)
    f.write("\n")
