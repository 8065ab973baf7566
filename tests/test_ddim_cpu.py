"""DDIM without a GPU: the float64 coefficient tables against the reference's (tests/golden/ddim_update.npz, written by
tools/make_ddim_golden.py from the reference's own tables), the public signatures, and the C ABI additions."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
NEW_EXPORTS = ("lfvdm_update_x0", "lfvdm_update_rng_x0", "lfvdm_conv_out_update_x0")      # DDIM is LFVDM_RULE_DDIM of these


def make_diffusion(resp):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, rescale_timesteps=True,
                                        rescale_learned_sigmas=True, diffusion_space_kwargs=dict(PIXEL))


@pytest.mark.parametrize("tag,resp", [("d1000", ""), ("ddim50", "ddim50")])
def test_ddim_coefficient_tables_match_the_reference(tag, resp):
    g = np.load(os.path.join(GOLDEN, "ddim_update.npz"))
    diff = make_diffusion(resp)
    assert diff.num_timesteps == int(g[f"{tag}/num_timesteps"])
    for name in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "alphas_cumprod_prev", "alphas_cumprod_next"):
        np.testing.assert_allclose(getattr(diff, name), g[f"{tag}/{name}"], rtol=1e-12, atol=0)
    for eta in (0.0, 0.5, 1.0):
        co = diff.ddim_coefficients(eta)
        assert all(v.dtype == np.float64 for v in co.values())
        for k in ("k1", "k2", "sigma"):
            np.testing.assert_allclose(co[k], g[f"{tag}/eta{eta}/{k}"], rtol=1e-12, atol=0, err_msg=f"{tag} eta {eta} {k}")
    assert np.all(diff.ddim_coefficients(0.0)["sigma"] == 0) and np.all(diff.ddim_coefficients(0.5)["sigma"][1:] > 0)
    # the last step of the chain: abar_prev = 1, so the sample IS pred_xstart, exactly, at every eta
    for eta in (0.0, 0.5, 1.0):
        co = diff.ddim_coefficients(eta)
        assert co["k1"][0] == 1.0 and co["k2"][0] == 0.0 and co["sigma"][0] == 0.0
    rev = diff.ddim_coefficients(0.0, reverse=True)
    for k in ("k1", "k2"):
        np.testing.assert_allclose(rev[k], g[f"{tag}/reverse/{k}"], rtol=1e-12, atol=0, err_msg=f"{tag} reverse {k}")
    assert np.all(rev["sigma"] == 0)
    with pytest.raises(AssertionError):
        diff.ddim_coefficients(0.5, reverse=True)
    assert diff.ddim_coefficients(0.5) is diff.ddim_coefficients(0.5), "built once per (eta, direction)"


def test_ddim_methods_and_signatures():
    from improved_diffusion.gaussian_diffusion import GaussianDiffusion, GraphSampler
    from improved_diffusion.respace import SpacedDiffusion
    step = ["self", "model", "x", "t", "clip_denoised", "denoised_fn", "model_kwargs", "eta"]
    loop = ["self", "model", "shape", "noise", "clip_denoised", "denoised_fn", "model_kwargs", "device", "progress", "eta"]
    want = {"ddim_sample": step, "ddim_reverse_sample": step, "ddim_sample_loop_progressive": loop,
            "ddim_sample_loop": loop + ["latent_mask", "return_decoded"]}
    defaults = {"clip_denoised": True, "denoised_fn": None, "model_kwargs": None, "eta": 0.0, "noise": None, "device": None,
                "progress": False, "latent_mask": None, "return_decoded": True}
    for name, params in want.items():
        assert hasattr(GaussianDiffusion, name), name
        sig = inspect.signature(getattr(GaussianDiffusion, name))
        assert list(sig.parameters)[:len(params)] == params, (name, list(sig.parameters))
        for p in params:
            if p in defaults:
                assert sig.parameters[p].default == defaults[p] or sig.parameters[p].default is defaults[p], (name, p)
    # the respaced diffusion wraps the model for the per-step methods (the loops reach the network through them or
    # through the sampler's remapped timestep table)
    for name in ("ddim_sample", "ddim_reverse_sample"):
        assert name in vars(SpacedDiffusion), name
    assert "rule" in inspect.signature(GraphSampler.__init__).parameters
    assert "rule" in inspect.signature(GaussianDiffusion._graph_sampler).parameters
    diff = make_diffusion("ddim10")
    assert all(hasattr(diff, n) for n in want)
    import improved_diffusion.gaussian_diffusion as gd
    head = gd.__doc__.split("Out of scope")[1]
    assert "DDIM" not in head, "DDIM is no longer out of scope"


def test_new_exports_are_bound_and_declared():
    from improved_diffusion import _native
    hdr = open(os.path.join(ROOT, "include", "lfvdm_hip.h")).read()
    declared = set(re.findall(r"\b(lfvdm_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_EXPORTS:
        assert name in _native.EXPORTS, name
        assert name in declared, name
    assert int(re.search(r"#define LFVDM_RULE_DDIM (\d+)", hdr).group(1)) == _native.RULE_DDIM
    assert "sg == NULL" in hdr and "DETERMINISTIC" in hdr, "the header says how the deterministic rule is selected"


def test_sampling_args_default_to_the_ancestral_chain():
    from improved_diffusion.video_sampler import default_sampling_args
    a = default_sampling_args(device="cpu")
    assert a.use_ddim is False and a.ddim_eta == 0.0
    b = default_sampling_args(device="cpu", use_ddim=True, ddim_eta=0.5)
    assert b.use_ddim is True and b.ddim_eta == 0.5
