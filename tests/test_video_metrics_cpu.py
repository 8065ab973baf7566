"""Video prediction metrics without a GPU (improved_diffusion/video_metrics.py, csrc/video_metrics.hip): the CPU path of
frame_metrics against a float64 evaluation of the definition written here, the closed forms (identical frames, constant
frames), uint8 against float, the best-of-K protocol on a planted case, every refusal, the two C-ABI additions (declared,
bound, refusing bad arguments before any launch) and the command line.

The yardstick (``yardstick``) is Wang et al.'s SSIM with the full 11 x 11 window through torch.nn.functional.conv2d in float64
- independent of the module, which filters separably - and the plain mean squared error; run in float32 it gives the
deviation a straightforward float32 evaluation has, which scales the bounds (``bounds``): every comparison is against the
float64 yardstick at max(floor, 3 x that deviation), floors 1e-4 relative for mse (the project's floor for per-sample losses)
and 1e-5 absolute for ssim (about ten roundings of a [0, 1] quantity divided by C2 = 9e-4)."""
import ctypes
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "latent-flexible-video-diffusion-modeling_amd")
NEW_EXPORTS = ("lfvdm_frame_metrics", "lfvdm_frame_metrics_workspace")
E_SHAPE = 1
MSE_REL, SSIM_ABS = 1e-4, 1e-5
C1, C2 = 0.01 ** 2, 0.03 ** 2
# (K, B, T, C, H, W): one tile with 6 x 6 valid positions; a single valid position; tiles straddled in both directions with
# rows that are no multiple of 4 pixels and K > 1 against a shared truth; the workload's own frame size; and, for the kernel's
# tiles of 16 x 32 positions, 2 x 2 tiles whose last row and column are one position wide
SHAPES = [(1, 2, 3, 3, 16, 16), (1, 1, 1, 1, 11, 11), (2, 1, 2, 3, 45, 37), (1, 1, 2, 4, 64, 64), (1, 1, 1, 2, 27, 43)]
DTYPES = ["float32", "uint8"]
NOISE = (0.004, 0.05, 0.4)


def yardstick(pred, truth, lo, hi, dtype=torch.float64):
    """mse, ssim of shape pred.shape[:-3] from the definition, in ``dtype``, on the CPU.  truth: pred's shape or without its
    leading axis."""
    x = (pred.cpu().to(dtype) - lo) / (hi - lo)
    y = ((truth.cpu().to(dtype) - lo) / (hi - lo)).expand_as(x)
    lead, (C, H, W) = x.shape[:-3], x.shape[-3:]
    x, y = x.reshape(-1, 1, H, W), y.reshape(-1, 1, H, W)
    d = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-d * d / (2 * 1.5 ** 2))
    w = torch.outer(g, g)
    w = (w / w.sum()).to(dtype).view(1, 1, 11, 11)
    mx, my = F.conv2d(x, w), F.conv2d(y, w)
    sxx, syy, sxy = F.conv2d(x * x, w) - mx * mx, F.conv2d(y * y, w) - my * my, F.conv2d(x * y, w) - mx * my
    smap = (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    assert smap.shape[-2:] == (H - 10, W - 10)
    ssim = smap.mean(dim=(1, 2, 3)).view(*lead, C).mean(-1)
    mse = ((x - y) ** 2).mean(dim=(1, 2, 3)).view(*lead, C).mean(-1)
    return mse, ssim


@functools.lru_cache(maxsize=None)
def make_case(shape, dtype):
    """-> pred (K, B, T, C, H, W), truth (B, T, C, H, W), (lo, hi): a smooth image plus noise at three levels (frame by frame),
    float32 in [-1, 1] or uint8; the first frame pair has a constant left half in both images (different constants)."""
    K, B, T, C, H, W = shape
    gen = torch.Generator().manual_seed(1000 * H + W + (7 if dtype == "uint8" else 0))
    yy = torch.linspace(0, 1, H, dtype=torch.float64).view(H, 1)
    xx = torch.linspace(0, 1, W, dtype=torch.float64).view(1, W)
    ph = 6.28 * torch.rand(B, T, C, 1, 1, 2, generator=gen, dtype=torch.float64)
    truth = 0.5 + 0.3 * torch.sin(5.0 * yy + ph[..., 0]) * torch.cos(4.0 * xx + ph[..., 1]) \
        + 0.03 * torch.randn(B, T, C, H, W, generator=gen, dtype=torch.float64)
    level = torch.tensor([NOISE[i % 3] for i in range(K * B * T)], dtype=torch.float64).view(K, B, T, 1, 1, 1)
    pred = truth.unsqueeze(0) + level * torch.randn(K, B, T, C, H, W, generator=gen, dtype=torch.float64)
    truth[0, 0, :, :, :W // 2] = 0.6
    pred[0, 0, 0, :, :, :W // 2] = 0.55
    pred, truth = pred.clamp(0, 1), truth.clamp(0, 1)
    if dtype == "uint8":
        return (255 * pred).round().to(torch.uint8), (255 * truth).round().to(torch.uint8), (0.0, 255.0)
    return (2 * pred - 1).float(), (2 * truth - 1).float(), (-1.0, 1.0)


@functools.lru_cache(maxsize=None)
def reference(shape, dtype):
    """-> (mse64, ssim64, mse bound (relative), ssim bound (absolute)) of make_case(shape, dtype); computed once."""
    pred, truth, (lo, hi) = make_case(shape, dtype)
    m64, s64 = yardstick(pred, truth, lo, hi)
    m32, s32 = yardstick(pred, truth, lo, hi, torch.float32)
    return m64, s64, bounds(m64, s64, m32, s32)


def bounds(m64, s64, m32, s32):
    return (max(MSE_REL, 3 * float((m32.double() / m64 - 1).abs().max())), max(SSIM_ABS, 3 * float((s32.double() - s64).abs().max())))


def compare(tag, got, m64, s64, bnd):
    """Print error / bound for mse (relative) and ssim (absolute), then assert; -> the two ratios."""
    em = float((got["mse"].double().cpu() / m64 - 1).abs().max())
    es = float((got["ssim"].double().cpu() - s64).abs().max())
    print(f"[video metrics {tag}] mse {em:.2e} ({em / bnd[0]:.3f} of bound {bnd[0]:.1e})  ssim {es:.2e} "
          f"({es / bnd[1]:.3f} of bound {bnd[1]:.1e})  ssim range {float(s64.min()):.3f}..{float(s64.max()):.3f}")
    assert got["mse"].shape == m64.shape and got["ssim"].shape == s64.shape
    assert bool(torch.isfinite(got["mse"]).all()) and bool(torch.isfinite(got["ssim"]).all())
    assert em <= bnd[0], (tag, "mse", em, bnd[0])
    assert es <= bnd[1], (tag, "ssim", es, bnd[1])
    return em / bnd[0], es / bnd[1]


def planted_case(dtype=torch.float32):
    """K = 3 samples of B = 4 videos of T = 5 frames: sample plant[b] is the truth plus small noise, the others plus large."""
    gen = torch.Generator().manual_seed(5)
    K, B, T, C, H, W = 3, 4, 5, 3, 16, 20
    truth = (0.8 * torch.rand(B, T, C, H, W, generator=gen) - 0.4)
    truth = F.avg_pool2d(truth.view(-1, 1, H, W), 5, 1, 2).view(B, T, C, H, W) * 3
    plant = torch.tensor([2, 0, 1, 2])
    sd = torch.full((K, B), 0.3)
    sd[plant, torch.arange(B)] = 0.02
    samples = (truth.unsqueeze(0) + sd.view(K, B, 1, 1, 1, 1) * torch.randn(K, B, T, C, H, W, generator=gen)).clamp(-1, 1)
    return samples.to(dtype), truth.clamp(-1, 1).to(dtype), plant


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cpu_path_matches_the_float64_yardstick(shape, dtype):
    from improved_diffusion.video_metrics import frame_metrics
    pred, truth, rng = make_case(shape, dtype)
    m64, s64, bnd = reference(shape, dtype)
    got = frame_metrics(pred, truth, data_range=rng)
    assert got["mse"].shape == pred.shape[:3] and got["mse"].dtype == torch.float32 and sorted(got) == ["mse", "psnr", "ssim"]
    compare(f"cpu {shape} {dtype}", got, m64, s64, bnd)
    assert torch.allclose(got["psnr"].double(), -10 * torch.log10(m64), rtol=0, atol=1e-3)
    # the defaults are the ranges of the two dtypes; a truth with the K axis spelled out is the same thing
    dflt = frame_metrics(pred, truth)
    full = frame_metrics(pred, truth.unsqueeze(0).expand_as(pred))
    for k in got:
        assert torch.equal(dflt[k], got[k]) and torch.equal(full[k], got[k]), k


def test_the_cases_span_the_range_of_ssim():
    every = torch.cat([reference(shape, dtype)[1].flatten() for shape in SHAPES for dtype in DTYPES])
    assert float(every.min()) < 0.2 and float(every.max()) > 0.99 and int(((every > 0.4) & (every < 0.9)).sum()) >= 4


def test_identical_inputs():
    from improved_diffusion.video_metrics import frame_metrics
    for dtype in DTYPES:
        pred, _, _ = make_case(SHAPES[2], dtype)
        got = frame_metrics(pred, pred.clone())
        assert float((got["ssim"] - 1).abs().max()) <= 1e-6
        assert float(got["mse"].abs().max()) == 0.0
        assert bool(torch.isinf(got["psnr"]).all()) and bool((got["psnr"] > 0).all())


def test_constant_frames_have_the_closed_form():
    from improved_diffusion.video_metrics import frame_metrics
    for a, b in ((0.25, 0.75), (0.0, 1.0), (0.5, 0.5), (0.9, 0.1)):
        x, y = torch.full((2, 3, 13, 17), a), torch.full((2, 3, 13, 17), b)
        got = frame_metrics(x, y, data_range=(0.0, 1.0))
        want = (2 * a * b + C1) / (a * a + b * b + C1)
        assert float((got["ssim"].double() - want).abs().max()) <= 1e-6, (a, b)
        assert float((got["mse"].double() - (a - b) ** 2).abs().max()) <= 1e-6 * (a - b) ** 2, (a, b)


def test_uint8_equals_float_with_the_0_255_range():
    from improved_diffusion.video_metrics import frame_metrics
    pred, truth, _ = make_case(SHAPES[2], "uint8")
    a = frame_metrics(pred, truth)
    b = frame_metrics(pred.float(), truth.float(), data_range=(0, 255))
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_prediction_metrics_picks_the_planted_sample():
    from improved_diffusion.video_metrics import frame_metrics, prediction_metrics
    samples, truth, plant = planted_case()
    T = samples.shape[2]
    for n_obs in (2, 0):
        for best_of in ("ssim", "psnr"):
            r = prediction_metrics(samples, truth, n_obs, best_of=best_of)
            assert torch.equal(r["best_index"], plant), (n_obs, best_of)
            m = frame_metrics(samples[:, :, n_obs:], truth[:, n_obs:])
            for name in ("psnr", "ssim", "mse"):
                assert r[f"mean_{name}"].shape == (T - n_obs,) and r[f"best_{name}"].shape == (T - n_obs,)
                assert torch.allclose(r[f"mean_{name}"], m[name].mean(dim=(0, 1)))
                want = torch.stack([m[name][plant[b], b] for b in range(4)]).mean(0)
                assert torch.allclose(r[f"best_{name}"], want)
                assert abs(r[f"best_{name}_avg"] - float(want.mean())) <= 1e-6 * abs(float(want.mean()))
            assert r["best_ssim_avg"] > r["mean_ssim_avg"] and r["best_psnr_avg"] > r["mean_psnr_avg"]
            assert r["best_mse_avg"] < r["mean_mse_avg"]
            assert (r["n_obs"], r["n_samples"], r["n_videos"], r["best_of"]) == (n_obs, 3, 4, best_of)


def test_every_refusal():
    from improved_diffusion.video_metrics import frame_metrics, prediction_metrics
    x = torch.zeros(2, 3, 3, 16, 16)
    bad = [
        (x, torch.zeros(2, 3, 3, 16, 15), {}), (x, torch.zeros(3, 3, 3, 16, 16), {}), (x, torch.zeros(16, 16), {}),
        (torch.zeros(2, 3, 10, 16), torch.zeros(2, 3, 10, 16), {}), (torch.zeros(2, 3, 16, 10), torch.zeros(2, 3, 16, 10), {}),
        (x.double(), x.double(), {}), (x.half(), x.half(), {}), (x.long(), x.long(), {}), (x, x.to(torch.uint8), {}),
        (torch.zeros(16, 16), torch.zeros(16, 16), {}), (x, x, dict(data_range=(1.0, 1.0))), (x, x, dict(data_range=(1.0, -1.0))),
        (x, x, dict(data_range=3.0)), (x.numpy(), x.numpy(), {}),
    ]
    for p, t, kw in bad:
        with pytest.raises(ValueError):
            frame_metrics(p, t, **kw)
    s, t = torch.zeros(2, 1, 4, 1, 12, 12), torch.zeros(1, 4, 1, 12, 12)
    for args, kw in (((s, t, 4), {}), ((s, t, -1), {}), ((s, t, 1), dict(best_of="lpips")), ((s[0], t, 1), {}),
                     ((s, torch.zeros(1, 3, 1, 12, 12), 1), {}), ((torch.zeros(2, 1, 4, 1, 10, 12), torch.zeros(1, 4, 1, 10, 12), 1), {})):
        with pytest.raises(ValueError):
            prediction_metrics(*args, **kw)


def test_new_exports_are_bound_and_declared():
    from improved_diffusion import _native
    hdr = open(os.path.join(ROOT, "include", "lfvdm_hip.h")).read()
    declared = set(re.findall(r"\b(lfvdm_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_EXPORTS:
        assert name in _native.EXPORTS and name in _native._SIGS, name
        assert name in declared, name
    assert len(_native._SIGS["lfvdm_frame_metrics"][0]) == 15 and len(_native._SIGS["lfvdm_frame_metrics_workspace"][0]) == 5
    assert _native._SIGS["lfvdm_frame_metrics_workspace"][1] is ctypes.c_long
    assert re.search(r"#define\s+LFVDM_PIX_F32\s+0\b", hdr) and re.search(r"#define\s+LFVDM_PIX_U8\s+1\b", hdr)
    assert (_native.PIX_F32, _native.PIX_U8) == (0, 1)
    assert callable(_native.frame_metrics) and callable(_native.frame_metrics_workspace)
    src = open(os.path.join(PKG, "csrc", "video_metrics.hip")).read()
    assert "atomicAdd" not in src and "atomic_" not in src, "no float atomics: the reduction order is fixed"
    lib = _native.lib()
    assert all(hasattr(lib, name) for name in NEW_EXPORTS)


def test_entry_refuses_bad_arguments_before_any_launch():
    """No device here: a launch would fail with LFVDM_E_LAUNCH (2), so LFVDM_E_SHAPE (1) shows the refusal came first."""
    from improved_diffusion import _native
    lib = _native.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)      # a non-null pointer; nothing is ever read through it
    ws = lib.lfvdm_frame_metrics_workspace
    # two floats per workgroup of 16 x 32 positions per (k, n, c) plane
    assert ws(1, 6, 3, 16, 16) == 2 * 18 and ws(1, 1, 1, 11, 11) == 2 and ws(2, 2, 3, 45, 37) == 2 * 12 * 3
    assert ws(10, 800, 3, 64, 64) == 2 * 24000 * 8 and ws(1, 1, 1, 26, 42) == 2 and ws(1, 1, 1, 27, 43) == 2 * 4
    assert ws(1, 1, 1, 10, 64) == 0 and ws(1, 1, 1, 64, 10) == 0 and ws(0, 1, 1, 64, 64) == 0 and ws(1, 1, -3, 64, 64) == 0

    def call(pred=p, truth=p, dtype=0, K=2, N=2, C=3, H=45, W=37, mse=p, ssim=p, part=p, short=0):
        need = ws(K, N, C, H, W) if min(K, N, C, H, W) > 0 else 1 << 20
        return lib.lfvdm_frame_metrics(pred, truth, dtype, 0.5, 0.5, K, N, C, H, W, mse, ssim, part, need - short, None)
    for kw in (dict(H=10), dict(W=10), dict(H=10, W=10), dict(short=1), dict(short=5), dict(K=0), dict(N=0), dict(C=0), dict(H=0), dict(W=-1),
               dict(K=-2), dict(dtype=2), dict(dtype=-1), dict(pred=None), dict(truth=None), dict(mse=None), dict(ssim=None),
               dict(part=None), dict(dtype=1, H=10)):
        assert call(**kw) == E_SHAPE, kw


def test_cli_round_trip(tmp_path):
    from improved_diffusion.video_metrics import prediction_metrics
    samples, truth, plant = planted_case()
    np.save(tmp_path / "s.npy", samples.numpy())
    np.save(tmp_path / "t.npy", truth.numpy())
    out = tmp_path / "metrics.json"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "improved_diffusion.video_metrics", "--samples", str(tmp_path / "s.npy"), "--truth",
                        str(tmp_path / "t.npy"), "--n_obs", "2", "--best_of", "psnr", "--out", str(out)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(out.read_text())
    assert json.loads(p.stdout) == res
    want = prediction_metrics(samples, truth, 2, best_of="psnr")
    assert res["best_index"] == plant.tolist() and res["best_of"] == "psnr" and res["n_obs"] == 2
    for k, v in want.items():
        if torch.is_tensor(v) and v.is_floating_point():
            assert len(res[k]) == 3
            np.testing.assert_allclose(res[k], v.numpy(), rtol=2e-4, atol=2e-5)      # the tool may have run on a device
        elif isinstance(v, float):
            assert abs(res[k] - v) <= 2e-4 * abs(v) + 2e-5, k
