"""x0-prediction models (predict_xstart=True) without a GPU: the factory, the mode check, the C ABI additions, the public
signatures and the fixtures' own invariants (tests/golden/xstart_*.npz, written by tools/make_xstart_golden.py)."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
NEW_EXPORTS = ("lfvdm_update_x0", "lfvdm_update_rng_x0", "lfvdm_conv_out_update_x0")
KEPT_EXPORTS = ("lfvdm_conv_out_psample_ok",)
RETIRED_EXPORTS = ("lfvdm_p_sample", "lfvdm_p_sample_rng", "lfvdm_ddim_sample", "lfvdm_ddim_sample_rng", "lfvdm_conv_out_psample",
                   "lfvdm_conv_out_ddim")


def make_diffusion(resp="", **kw):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, rescale_timesteps=True,
                                        rescale_learned_sigmas=True, diffusion_space_kwargs=dict(PIXEL), **kw)


def test_predict_xstart_is_a_native_mode():
    from improved_diffusion.gaussian_diffusion import ModelMeanType
    for resp in ("", "ddim50"):
        diff = make_diffusion(resp, predict_xstart=True)
        assert diff.model_mean_type == ModelMeanType.START_X
        diff._check_native_modes()
        assert diff.predicts_xstart is True
    eps = make_diffusion()
    assert eps.model_mean_type == ModelMeanType.EPSILON and eps.predicts_xstart is False
    eps._check_native_modes()


def test_previous_x_and_learned_sigma_still_raise():
    from improved_diffusion.gaussian_diffusion import ModelMeanType
    diff = make_diffusion(predict_xstart=True)
    diff.model_mean_type = ModelMeanType.PREVIOUS_X
    with pytest.raises(NotImplementedError, match="PREVIOUS_X"):
        diff._check_native_modes()
    for kw in (dict(learn_sigma=True), dict(learn_sigma=True, predict_xstart=True)):
        with pytest.raises(NotImplementedError, match="sigma"):
            make_diffusion(**kw)._check_native_modes()


def test_new_exports_are_bound_and_declared():
    from improved_diffusion import _native
    hdr = open(os.path.join(ROOT, "include", "lfvdm_hip.h")).read()
    declared = set(re.findall(r"\b(lfvdm_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_EXPORTS + KEPT_EXPORTS:
        assert name in _native.EXPORTS, name
        assert name in declared, name
    for name in ("LFVDM_RULE_ANCESTRAL", "LFVDM_RULE_DDIM", "LFVDM_MEAN_EPS", "LFVDM_MEAN_X0"):
        value = int(re.search(rf"#define {name} (\d+)", hdr).group(1))
        assert getattr(_native, name[len("LFVDM_"):]) == value, name
    for name, nargs in zip(NEW_EXPORTS, (18, 19, 27)):
        assert len(_native._SIGS[name][0]) == nargs, name
    for fn in ("update_x0", "update_rng_x0", "conv_out_update_x0"):
        assert callable(getattr(_native, fn))


def test_retired_update_entries_are_gone():
    """One update entry per launch kind: the six entries that each hand-picked one rule x mean type cell are neither
    declared, bound, wrapped nor exported by the built library."""
    import ctypes
    from improved_diffusion import _native
    hdr = open(os.path.join(ROOT, "include", "lfvdm_hip.h")).read()
    declared = set(re.findall(r"\b(lfvdm_[a-z0-9_]+)\s*\(", hdr))
    assert os.path.exists(_native.LIB_PATH), "run `python __graft_entry__.py` (build) first"
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(lib, name) for name in NEW_EXPORTS + KEPT_EXPORTS)
    for name in RETIRED_EXPORTS:
        assert name not in declared, name
        assert name not in _native._SIGS and name not in _native.EXPORTS, name
        assert not hasattr(_native, name[len("lfvdm_"):]), name
        assert not hasattr(lib, name), name


def test_public_signatures_are_unchanged():
    from improved_diffusion.gaussian_diffusion import GaussianDiffusion, GraphSampler
    from improved_diffusion._engine import Plan
    want = {
        "p_mean_variance": ["self", "model", "x", "t", "clip_denoised", "denoised_fn", "model_kwargs", "return_attn_weights"],
        "p_sample": ["self", "model", "x", "t", "clip_denoised", "denoised_fn", "model_kwargs", "return_attn_weights", "noise"],
        "p_sample_loop": ["self", "model", "shape", "noise", "clip_denoised", "denoised_fn", "model_kwargs", "device", "progress",
                          "latent_mask", "return_attn_weights", "return_decoded"],
        "ddim_sample": ["self", "model", "x", "t", "clip_denoised", "denoised_fn", "model_kwargs", "eta", "noise"],
        "ddim_reverse_sample": ["self", "model", "x", "t", "clip_denoised", "denoised_fn", "model_kwargs", "eta"],
        "ddim_sample_loop": ["self", "model", "shape", "noise", "clip_denoised", "denoised_fn", "model_kwargs", "device", "progress",
                             "eta", "latent_mask", "return_decoded"],
        "training_losses": ["self", "model", "x_start", "t", "model_kwargs", "noise", "latent_mask", "eval_mask"],
        "_graph_sampler": ["self", "unet", "shape", "clip_denoised", "rule"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(GaussianDiffusion, name)).parameters) == params, name
    assert list(inspect.signature(GraphSampler.__init__).parameters) == ["self", "diffusion", "unet", "shape", "clip_denoised",
                                                                        "inject_noise", "rule"]
    fuse = inspect.signature(Plan.fuse_head_update).parameters
    assert list(fuse)[:9] == ["self", "t_buf", "tables", "clip", "seed", "noise", "pred", "inject_noise", "ddim"]
    assert fuse["predict_xstart"].default is False
    import improved_diffusion.gaussian_diffusion as gd
    head, tail = gd.__doc__.split("Out of scope")
    assert "predict_xstart" in head and "PREVIOUS_X" in tail and "predict_xstart" not in tail


def test_fixture_invariants():
    """Every update case exercises both sides of the clamp; the stored x0-hat is the clamped model output; the trajectories
    carry the fp32 reference's own deviation for every stored step."""
    g = np.load(os.path.join(GOLDEN, "xstart_update.npz"))
    for tag in ("d1000", "ddim50"):
        nt = int(g[f"{tag}/num_timesteps"])
        seen = set()
        for ti in (0, 1):
            case = f"{tag}/t{ti}"
            assert 0.02 < float(g[f"{case}/clamp_share"]) < 0.6
            seen |= set(g[f"{case}/t"].tolist())
            mo = g[f"{case}/out"].astype(np.float64)
            assert np.array_equal(g[f"{case}/clip1/pred_xstart"], np.clip(mo, -1, 1))
            assert np.array_equal(g[f"{case}/clip0/pred_xstart"], mo)
        assert {0, 1, nt // 2, nt - 1} <= seen
    tr = np.load(os.path.join(GOLDEN, "xstart_traj_cfgB.npz"))
    for leg, n in (("p", 3), ("eta0", 10), ("eta1", 4)):
        for key in ("sample", "pred_xstart"):
            assert tr[f"{leg}/{key}/sub"].shape[0] == n and tr[f"{leg}/ref32_dev/{key}"].shape == (n,)
            assert float(np.abs(tr[f"{leg}/pred_xstart/sub"]).max()) <= 1.0
    w = np.load(os.path.join(GOLDEN, "xstart_window_cfgD.npz"))
    assert w["frame_indices"].shape == (1, 14) and w["top/sample/sub"].shape[0] == 3 and w["bottom/sample/sub"].shape[0] == 2
    t = np.load(os.path.join(GOLDEN, "xstart_train_micro.npz"))
    assert t["loss"].shape == (2,) and np.array_equal(t["loss"], t["mse"]) and len(t["keys"]) == len(t["grad_norm"]) == len(t["grad_head"])
