"""Video prediction metrics that need no network: per-frame PSNR and SSIM against the ground-truth continuation, and the
best-of-K protocol of conditional video prediction (MCVD / RaMViD / SVG) on top of them.

    frame_metrics(pred, truth)                      -> {"mse", "psnr", "ssim"}, one value per frame
    prediction_metrics(samples, truth, n_obs)       -> per-frame curves over the predicted frames, mean sample and best of K

    python -m improved_diffusion.video_metrics --samples S.npy --truth T.npy --n_obs N [--best_of ssim|psnr] [--out metrics.json]

SSIM is Wang et al. 2004 as everybody reports it: 11 x 11 Gaussian window (sigma 1.5, sum 1), valid positions only, data in
[0, 1] (L = 1, C1 = 0.01^2, C2 = 0.03^2), biased moments from the same window, the map averaged over positions and channels.
MSE is over all pixels of the [0, 1] values; PSNR = -10 log10(mse) (inf for identical frames).

Tensors on the device go through one launch pair of csrc/video_metrics.hip for the whole call (lfvdm_frame_metrics: no float
atomics, bitwise reproducible); CPU tensors go through ``_frame_metrics_torch``, the same definition in plain float64 torch.
"""
import argparse
import json
import math

import numpy as np
import torch
import torch.nn.functional as F

WIN, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2
_CHUNK_PLANES = 1024      # planes per slice of the CPU path (bounds its float64 temporaries)


def _ranges(pred, truth, data_range):
    """Validate; -> (K, lead shape of the result, C, H, W, lo, hi)."""
    if not (torch.is_tensor(pred) and torch.is_tensor(truth)):
        raise ValueError("frame_metrics takes torch tensors")
    if pred.dtype not in (torch.uint8, torch.float32) or truth.dtype != pred.dtype:
        raise ValueError(f"pred and truth must both be uint8 or both float32, got {pred.dtype} and {truth.dtype}")
    if pred.dim() < 3:
        raise ValueError(f"pred must be (..., C, H, W), got {tuple(pred.shape)}")
    if tuple(truth.shape) == tuple(pred.shape):
        K = None
    elif pred.dim() >= 4 and tuple(truth.shape) == tuple(pred.shape[1:]):
        K = pred.shape[0]
    else:
        raise ValueError(f"truth {tuple(truth.shape)} has neither the shape of pred {tuple(pred.shape)} nor that shape without "
                         "its leading sample axis")
    if pred.device != truth.device:
        raise ValueError(f"pred is on {pred.device}, truth on {truth.device}")
    C, H, W = pred.shape[-3:]
    if H < WIN or W < WIN:
        raise ValueError(f"frames of {H} x {W} have no valid position of the {WIN} x {WIN} SSIM window")
    if pred.numel() == 0:
        raise ValueError(f"empty input {tuple(pred.shape)}")
    if data_range is None:
        data_range = (0.0, 255.0) if pred.dtype == torch.uint8 else (-1.0, 1.0)
    try:
        lo, hi = (float(v) for v in data_range)
    except (TypeError, ValueError):
        raise ValueError(f"data_range must be (lo, hi), got {data_range!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError(f"data_range must be finite with hi > lo, got {data_range!r}")
    return K, tuple(pred.shape[:-3]), C, H, W, lo, hi


def _window(dtype, device):
    d = torch.arange(WIN, dtype=torch.float64, device=device) - (WIN - 1) / 2
    g = torch.exp(-d * d / (2 * SIGMA ** 2))
    return (g / g.sum()).to(dtype)


def _frame_metrics_torch(pred, truth, K, N, C, H, W, lo, hi):
    """The definition in float64 torch ops on any device: (K, N, C, H, W) against (N, C, H, W) -> mse, ssim (K, N) float64."""
    g = _window(torch.float64, pred.device)
    gh, gv = g.view(1, 1, 1, WIN), g.view(1, 1, WIN, 1)
    blur = lambda a: F.conv2d(F.conv2d(a, gh), gv)      # noqa: E731
    x = pred.reshape(K, N * C, H, W)
    y = truth.reshape(N * C, H, W)
    mse = torch.empty(K, N * C, dtype=torch.float64, device=pred.device)
    ssim = torch.empty_like(mse)
    for k in range(K):
        for p0 in range(0, N * C, _CHUNK_PLANES):
            a = ((x[k, p0:p0 + _CHUNK_PLANES].double() - lo) / (hi - lo)).unsqueeze(1)
            b = ((y[p0:p0 + _CHUNK_PLANES].double() - lo) / (hi - lo)).unsqueeze(1)
            mse[k, p0:p0 + _CHUNK_PLANES] = ((a - b) ** 2).mean(dim=(1, 2, 3))
            mx, my = blur(a), blur(b)
            sxx, syy, sxy = blur(a * a) - mx * mx, blur(b * b) - my * my, blur(a * b) - mx * my
            m = (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
            ssim[k, p0:p0 + _CHUNK_PLANES] = m.mean(dim=(1, 2, 3))
    return mse.view(K, N, C).mean(-1), ssim.view(K, N, C).mean(-1)


def frame_metrics(pred, truth, data_range=None):
    """MSE, PSNR and SSIM of every frame of ``pred`` (..., C, H, W) against ``truth``: the same shape, or ``pred`` without its
    leading K (samples) axis - then the one truth serves every sample and is not replicated.  ``uint8`` (0-255) or ``float32``
    with ``data_range=(lo, hi)``, default (-1, 1), the range ``sample_video`` returns.  -> dict of float32 tensors of shape
    ``pred.shape[:-3]`` on the input's device.  Device tensors: one native launch pair; CPU tensors: plain torch.
    ``ValueError`` for mismatched shapes, H or W < 11 and other dtypes, before anything runs."""
    K, lead, C, H, W, lo, hi = _ranges(pred, truth, data_range)
    n_frames = int(np.prod(lead, dtype=np.int64))
    Kk = 1 if K is None else K
    N = n_frames // Kk
    pred, truth = pred.contiguous(), truth.contiguous()
    if pred.is_cuda:
        from . import _native as nat
        with torch.cuda.device(pred.device):
            mse = torch.empty(Kk, N, device=pred.device, dtype=torch.float32)
            ssim = torch.empty_like(mse)
            ws = torch.empty(nat.frame_metrics_workspace(Kk, N, C, H, W), device=pred.device, dtype=torch.float32)
            nat.frame_metrics(pred, truth, 1.0 / (hi - lo), -lo / (hi - lo), Kk, N, C, H, W, mse, ssim, ws)
    else:
        mse, ssim = (v.float() for v in _frame_metrics_torch(pred, truth, Kk, N, C, H, W, lo, hi))
    mse, ssim = mse.view(lead), ssim.view(lead)
    return {"mse": mse, "psnr": -10.0 * torch.log10(mse), "ssim": ssim}


def prediction_metrics(samples, truth, n_obs, best_of="ssim"):
    """The conditional-prediction protocol: K samples (K, B, T, C, H, W) of B test videos (B, T, C, H, W) whose first
    ``n_obs`` frames were observed.  One ``frame_metrics`` call over the predicted frames t >= n_obs, then

      mean_*   curves (T - n_obs,): psnr / ssim / mse of frame t averaged over the K samples and the B videos
      best_*   the same for the best sample of each video, chosen by its mean ``best_of`` ("ssim" or "psnr") over the
               predicted frames (ties: the lowest index)
      *_avg    the curves' means, as floats;  best_index (B,): the chosen sample of each video

    (PSNR is averaged frame by frame, as the protocol does; a frame reproduced exactly makes it inf.)"""
    if best_of not in ("ssim", "psnr"):
        raise ValueError(f"best_of must be 'ssim' or 'psnr', got {best_of!r}")
    if not (torch.is_tensor(samples) and torch.is_tensor(truth)) or samples.dim() != 6 or truth.dim() != 5:
        raise ValueError("samples must be (K, B, T, C, H, W) and truth (B, T, C, H, W)")
    if tuple(samples.shape[1:]) != tuple(truth.shape):
        raise ValueError(f"samples {tuple(samples.shape)} are not K samples of truth {tuple(truth.shape)}")
    K, B, T = samples.shape[:3]
    n_obs = int(n_obs)
    if not 0 <= n_obs < T:
        raise ValueError(f"n_obs = {n_obs} leaves no predicted frame of {T}")
    m = frame_metrics(samples[:, :, n_obs:], truth[:, n_obs:])      # each (K, B, T - n_obs)
    best = m[best_of].mean(dim=2).argmax(dim=0)                      # (B,)
    pick = best.view(1, B, 1).expand(1, B, T - n_obs)
    out = {"n_obs": n_obs, "n_samples": int(K), "n_videos": int(B), "best_of": best_of, "best_index": best}
    for name, v in m.items():
        curves = {"mean": v.mean(dim=(0, 1)), "best": v.gather(0, pick)[0].mean(dim=0)}
        for kind, c in curves.items():
            out[f"{kind}_{name}"] = c
            out[f"{kind}_{name}_avg"] = float(c.mean())
    return out


def _jsonable(d):
    return {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in d.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description="per-frame PSNR / SSIM of K samples against the ground truth, best of K per video")
    ap.add_argument("--samples", required=True, help=".npy of (K, B, T, C, H, W), uint8 (0-255) or float (in --data_range)")
    ap.add_argument("--truth", required=True, help=".npy of (B, T, C, H, W), the same dtype")
    ap.add_argument("--n_obs", type=int, required=True, help="observed frames at the start of each video (not scored)")
    ap.add_argument("--best_of", choices=("ssim", "psnr"), default="ssim")
    ap.add_argument("--out", default=None, help="also write the result as JSON here")
    args = ap.parse_args(argv)
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"

    def load(path):
        a = np.load(path)
        if a.dtype != np.uint8:
            a = a.astype(np.float32)      # float16 / float64 files: the metric works on float32 in [-1, 1]
        return torch.from_numpy(a).to(dev)
    res = _jsonable(prediction_metrics(load(args.samples), load(args.truth), args.n_obs, args.best_of))
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return res


if __name__ == "__main__":
    main()
