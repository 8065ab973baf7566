"""DPM-Solver++(2M) without a GPU: the float64 coefficient tables against an independent unfolded restatement, the solver's
order on an analytic Gaussian-data model whose probability-flow ODE has a closed form (driven by the product's own tables),
the public signatures and the C ABI additions."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
NEW_EXPORTS = ("lfvdm_update_ms_x0", "lfvdm_conv_out_update_ms_x0")


def make_diffusion(resp, schedule="linear", steps=1000):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=steps, noise_schedule=schedule, timestep_respacing=resp, rescale_timesteps=True,
                                        rescale_learned_sigmas=True, diffusion_space_kwargs=dict(PIXEL))


@pytest.mark.parametrize("schedule", ["linear", "cosine"])
@pytest.mark.parametrize("resp", ["", "ddim50", "ddim20", "ddim10"])
def test_tables_match_the_unfolded_solver(schedule, resp):
    """k1 / k2 ARE the eta = 0 DDIM arrays; k3 against -alpha_{t-1} expm1(-h) / (2 r) written out from abar alone (rtol 1e-9:
    the folded k1 = sqrt(abar_prev) - c / sqrt_recipm1 cancels at most about 5 of 16 digits at h >= 1e-5); k3 is 0 at the
    chain's first step and at its last two."""
    diff = make_diffusion(resp, schedule)
    co = diff.dpm_solver_coefficients()
    assert set(co) == {"k1", "k2", "k3"} and all(v.dtype == np.float64 for v in co.values())
    dd = diff.ddim_coefficients(0.0)
    assert np.array_equal(co["k1"], dd["k1"]) and np.array_equal(co["k2"], dd["k2"])
    assert diff.dpm_solver_coefficients() is co, "built once"
    n = diff.num_timesteps
    abar = np.asarray(diff.alphas_cumprod, dtype=np.float64)
    alpha, sigma = np.sqrt(abar), np.sqrt(1.0 - abar)
    lam = np.log(alpha / sigma)
    want = np.zeros(n)
    for t in range(2, n - 1):
        h = lam[t - 1] - lam[t]
        assert h >= 1e-5
        r = (lam[t] - lam[t + 1]) / h
        want[t] = -alpha[t - 1] * np.expm1(-h) / (2.0 * r)
    np.testing.assert_allclose(co["k3"], want, rtol=1e-9, atol=0)
    assert co["k3"][0] == 0.0 and co["k3"][1] == 0.0 and co["k3"][n - 1] == 0.0
    assert np.all(co["k3"][2:n - 1] > 0.0)
    # the first-order step in the solver's own terms: k1 = -alpha_{t-1} expm1(-h), k2 = sigma_{t-1} / sigma_t
    for t in range(1, n):
        h = lam[t - 1] - lam[t]
        np.testing.assert_allclose(co["k1"][t], -alpha[t - 1] * np.expm1(-h), rtol=1e-9)
        np.testing.assert_allclose(co["k2"][t], sigma[t - 1] / sigma[t], rtol=1e-9)


def test_three_step_diffusion_is_first_order_throughout():
    diff = make_diffusion("3")
    assert diff.num_timesteps == 3
    assert np.array_equal(diff.dpm_solver_coefficients()["k3"], np.zeros(3))


def _end_point_error(diff, s, multistep):
    """|chain's end point - the ODE's| from x_T = 1 for data ~ N(0, s^2): x0-hat = alpha s^2 / (alpha^2 s^2 + sigma^2) x,
    exact end point x_T s / sqrt(alpha_T^2 s^2 + sigma_T^2); float64, the product's tables, no clamp."""
    co = diff.dpm_solver_coefficients()
    abar = np.asarray(diff.alphas_cumprod, dtype=np.float64)
    n = diff.num_timesteps
    x, prev = 1.0, None
    for t in range(n - 1, -1, -1):
        a2, s2 = abar[t], 1.0 - abar[t]
        p0 = np.sqrt(a2) * s * s / (a2 * s * s + s2) * x
        nxt = co["k1"][t] * p0 + co["k2"][t] * x
        if multistep and prev is not None:
            nxt += co["k3"][t] * (p0 - prev)
        x, prev = nxt, p0
    exact = s / np.sqrt(abar[n - 1] * s * s + 1.0 - abar[n - 1])
    return abs(x - exact)


@pytest.mark.parametrize("schedule", ["linear", "cosine"])
@pytest.mark.parametrize("s", [0.5, 1.0])
def test_second_order_on_the_analytic_gaussian_model(schedule, s):
    """ddim20: the multistep chain's end-point error is at most half of DDIM's (worst ratio seen: 0.30, linear, s = 0.5)."""
    diff = make_diffusion("ddim20", schedule)
    e1, e2 = _end_point_error(diff, s, False), _end_point_error(diff, s, True)
    print(f"[{schedule} s={s}] DDIM {e1:.3e}  DPM-Solver++(2M) {e2:.3e}  ratio {e2 / e1:.3f}")
    assert e2 <= 0.5 * e1, (schedule, s, e1, e2)


def test_methods_and_signatures():
    from improved_diffusion.gaussian_diffusion import GaussianDiffusion, GraphSampler
    from improved_diffusion.respace import SpacedDiffusion
    step = ["self", "model", "x", "t", "clip_denoised", "denoised_fn", "model_kwargs", "prev_pred_xstart"]
    loop = ["self", "model", "shape", "noise", "clip_denoised", "denoised_fn", "model_kwargs", "device", "progress"]
    want = {"dpm_solver_sample": step, "dpm_solver_sample_loop_progressive": loop,
            "dpm_solver_sample_loop": loop + ["latent_mask", "return_decoded"]}
    defaults = {"clip_denoised": True, "denoised_fn": None, "model_kwargs": None, "prev_pred_xstart": None, "noise": None,
                "device": None, "progress": False, "latent_mask": None, "return_decoded": True}
    for name, params in want.items():
        sig = inspect.signature(getattr(GaussianDiffusion, name))
        assert list(sig.parameters) == params, (name, list(sig.parameters))
        assert "eta" not in sig.parameters
        for p in params:
            if p in defaults:
                assert sig.parameters[p].default is defaults[p], (name, p)
    assert "dpm_solver_sample" in vars(SpacedDiffusion), "the respaced diffusion wraps the model for the per-step method"
    diff = make_diffusion("ddim10")
    assert all(hasattr(diff, n) for n in want) and callable(diff.dpm_solver_tables)
    assert "hist" in inspect.signature(GaussianDiffusion._update_denoised).parameters
    with pytest.raises(ValueError, match="unknown update rule"):
        GraphSampler(diff, None, (2, 20, 4, 16, 16), True, rule=("dpmpp2m", 1))
    import improved_diffusion.gaussian_diffusion as gd
    head = gd.__doc__.split("Out of scope")[0]
    assert "DPM-Solver++(2M)" in head and "has not been measured" in head


def test_spaced_wrapper_sends_the_original_timestep():
    """dpm_solver_sample on a ddim50 diffusion reaches the network through the timestep remap (stride 20: 7 -> 140), on
    the way in; the update behind it needs the device, so the call stops there."""
    import torch
    diff = make_diffusion("ddim50")
    seen = []

    class Stop(Exception):
        pass

    class Net:
        def __call__(self, x_, timesteps=None, **kw):
            seen.append(timesteps.clone())
            raise Stop
    with pytest.raises(Stop):
        diff.dpm_solver_sample(Net(), torch.zeros(2, 1, 1, 2, 2), torch.tensor([7, 0]), model_kwargs={})
    assert seen[0].tolist() == [140.0, 0.0]


def test_new_exports_are_bound_and_declared():
    from improved_diffusion import _native
    hdr = open(os.path.join(ROOT, "include", "lfvdm_hip.h")).read()
    declared = set(re.findall(r"\b(lfvdm_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_EXPORTS:
        assert name in _native.EXPORTS and name in _native._SIGS, name
        assert name in declared, name
    assert len(_native._SIGS["lfvdm_update_ms_x0"][0]) == 16 and len(_native._SIGS["lfvdm_conv_out_update_ms_x0"][0]) == 23
    assert callable(_native.update_ms_x0) and callable(_native.conv_out_update_ms_x0)
    assert "hist may equal pred_xstart" in hdr and "hist == NULL" in hdr, "the header states the aliasing contract"
    # the three general entries keep their signatures
    for name, nargs in zip(("lfvdm_update_x0", "lfvdm_update_rng_x0", "lfvdm_conv_out_update_x0"), (18, 19, 27)):
        assert len(_native._SIGS[name][0]) == nargs, name


def test_built_library_exports_the_multistep_entries():
    import ctypes
    from improved_diffusion import _native
    assert os.path.exists(_native.LIB_PATH), "run `python __graft_entry__.py` (build) first"
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(lib, name) for name in NEW_EXPORTS)


def test_sampling_args():
    from improved_diffusion.video_sampler import default_sampling_args
    a = default_sampling_args(device="cpu")
    assert a.use_dpm_solver is False and a.use_ddim is False
    assert default_sampling_args(device="cpu", use_dpm_solver=True).use_dpm_solver is True
    with pytest.raises(ValueError, match="use_ddim and use_dpm_solver"):
        default_sampling_args(device="cpu", use_ddim=True, use_dpm_solver=True)
