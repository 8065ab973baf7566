"""Dynamic thresholding of x0-hat, host side (no GPU): the two entries are declared, bound and exported; the plain-torch
reference against a direct ``torch.quantile`` float64 composition; the validation of ``set_dynamic_threshold`` and of the
LFVDM_DYNAMIC_THRESHOLD string; the setting as part of both sampler cache keys."""
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
NAMES = ("lfvdm_dyn_threshold", "lfvdm_dyn_threshold_workspace")


def make_diffusion(resp="ddim10", predict_xstart=False):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, rescale_timesteps=True, rescale_learned_sigmas=True,
                                        predict_xstart=predict_xstart, diffusion_space_kwargs=dict(PIXEL))


def test_entries_are_declared_bound_and_exported():
    import ctypes
    from improved_diffusion import _native as nat
    header = open(os.path.join(ROOT, "include", "lfvdm_hip.h")).read()
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), f"{name} is not declared in lfvdm_hip.h"
        assert name in nat.EXPORTS
        getattr(L, name)
    assert callable(nat.dyn_threshold) and callable(nat.dyn_threshold_workspace)
    assert nat.lib().lfvdm_abi_version() == 9
    n = ctypes.c_size_t(0)
    assert L.lfvdm_dyn_threshold_workspace(ctypes.c_int(3), ctypes.c_int64(1000), ctypes.byref(n)) == 0 and n.value > 0
    assert nat.dyn_threshold_workspace(3, 1000) == n.value == 3 * nat.dyn_threshold_workspace(1, 5)
    for B, inner in ((0, 10), (2, 0), (2, 2 ** 31), (70000, 4)):
        with pytest.raises(RuntimeError, match="invalid shape"):
            nat.dyn_threshold_workspace(B, inner)


def _quantile_composition(p, mask, pct, max_value):
    """The definition spelled with torch.quantile, float64, sample by sample"""
    B, T = p.shape[:2]
    out, scales = torch.empty_like(p, dtype=torch.float64), []
    for b in range(B):
        keep = torch.ones(T, dtype=torch.bool) if mask is None else mask.reshape(B, T)[b] != 0
        v = p[b][keep].double().abs().reshape(-1)
        s = 1.0 if v.numel() == 0 else max(float(torch.quantile(v, pct, interpolation="linear")), 1.0)
        s = s if max_value is None else min(s, max_value)
        scales.append(s)
        out[b] = p[b].double().clamp(-s, s) / s
    return out, torch.tensor(scales, dtype=torch.float64)


@pytest.mark.parametrize("pct", [0.5, 0.995, 1.0])
@pytest.mark.parametrize("max_value", [None, 1.5])
def test_reference_equals_the_quantile_composition(pct, max_value):
    from improved_diffusion.gaussian_diffusion import dynamic_threshold_reference
    g = torch.Generator().manual_seed(5)
    p = 2.5 * torch.randn(4, 5, 3, 6, 7, generator=g)
    mask = torch.tensor([[1, 1, 1, 1, 1], [0, 1, 0, 1, 1], [0, 0, 0, 0, 0], [0, 0, 0.5, 0, 0]]).view(4, 5, 1, 1, 1)
    for m in (None, mask):
        got, s = dynamic_threshold_reference(p, m, pct, max_value, return_scale=True)
        want, ws = _quantile_composition(p, m, pct, max_value)
        assert got.dtype == p.dtype and got.shape == p.shape and s.dtype == torch.float64
        assert torch.allclose(s, ws, rtol=1e-13, atol=0), (s, ws)      # torch.lerp's two branches differ in the last bits
        assert float((got.double() - want).abs().max()) <= 2.0 ** -23, "float32 rounding of values in [-1, 1]"
        assert float(got.abs().max()) <= 1.0
        if m is not None:
            assert float(s[2]) == 1.0, "no selected frame: s = 1"
            assert torch.equal(got[2], p[2].clamp(-1, 1))
        if pct == 1.0 and max_value is None:      # the maximum: nothing is clamped, everything is divided
            b = 0
            assert float(s[b]) == float(p[b].abs().max()) and torch.allclose(got[b].double(), p[b].double() / s[b], rtol=1e-6)
    # an exact integer position
    q =torch.tensor([[[3.0], [-1.0], [2.0], [-5.0], [4.0]]])      # |.| sorted 1 2 3 4 5, pos = 0.5 * 4 = 2
    got, s = dynamic_threshold_reference(q, None, 0.5, None, return_scale=True)
    assert float(s[0]) == 3.0 and torch.equal(got, (q.clamp(-3, 3) / 3))
    d64 = dynamic_threshold_reference(q.double(), None, 0.75, None)
    assert d64.dtype == torch.float64 and torch.equal(d64, q.double().clamp(-4, 4) / 4)


def test_setter_validation_and_the_environment_string(monkeypatch):
    from improved_diffusion.gaussian_diffusion import parse_dynamic_threshold
    from improved_diffusion.video_sampler import resolve_dynamic_threshold, default_sampling_args
    diff = make_diffusion()
    assert diff.dynamic_threshold is None and diff._threshold(True) is None
    diff.set_dynamic_threshold(0.995)
    assert diff.dynamic_threshold == (0.995, None)
    diff.set_dynamic_threshold(1, max_value=1)
    assert diff.dynamic_threshold == (1.0, 1.0)
    diff.set_dynamic_threshold(0.9, max_value=float("inf"))
    assert diff.dynamic_threshold == (0.9, None)
    for kw in (dict(percentile=0.0), dict(percentile=-0.1), dict(percentile=1.0001), dict(percentile=float("nan")),
               dict(percentile="x"), dict(percentile=0.9, max_value=0.99), dict(percentile=0.9, max_value=float("nan")),
               dict(percentile=0.9, max_value="y"), dict(max_value=2.0)):
        with pytest.raises(ValueError, match="dynamic threshold"):
            diff.set_dynamic_threshold(**kw)
        assert diff.dynamic_threshold == (0.9, None), "a refused setting leaves the one in force untouched"
    diff.set_dynamic_threshold()
    assert diff.dynamic_threshold is None
    from improved_diffusion.respace import SpacedDiffusion
    assert isinstance(diff, SpacedDiffusion), "the respaced diffusion inherits the setter"

    assert parse_dynamic_threshold("0.995") == {"percentile": 0.995, "max_value": None}
    assert parse_dynamic_threshold(" 0.995:1.5 ") == {"percentile": 0.995, "max_value": 1.5}
    assert parse_dynamic_threshold("none") == parse_dynamic_threshold("") == {"percentile": None, "max_value": None}
    for bad in ("a", "0.9:b", "0.9:1.5:2", ":", 0.9):
        with pytest.raises(ValueError, match="dynamic threshold"):
            parse_dynamic_threshold(bad)
    with pytest.raises(ValueError, match="dynamic threshold"):
        diff.set_dynamic_threshold(**parse_dynamic_threshold("1.5"))      # the shape passes, the value does not

    monkeypatch.delenv("LFVDM_DYNAMIC_THRESHOLD", raising=False)
    a = default_sampling_args(device="cpu")
    assert a.dynamic_threshold is None and a.dynamic_threshold_max is None and resolve_dynamic_threshold(a) is None
    assert resolve_dynamic_threshold(types.SimpleNamespace()) is None, "args without the attributes: getattr form"
    monkeypatch.setenv("LFVDM_DYNAMIC_THRESHOLD", "0.99:2")
    assert resolve_dynamic_threshold(a) == {"percentile": 0.99, "max_value": 2.0}
    b = default_sampling_args(device="cpu", dynamic_threshold=0.9, dynamic_threshold_max=1.25)
    assert resolve_dynamic_threshold(b) == {"percentile": 0.9, "max_value": 1.25}, "args win over the environment"
    with pytest.raises(ValueError, match="dynamic_threshold_max needs"):
        resolve_dynamic_threshold(types.SimpleNamespace(dynamic_threshold_max=2.0))


def test_setting_is_part_of_both_sampler_cache_keys(monkeypatch):
    """Host only: ``_cached_sampler`` is replaced by a recorder of (cache, key)."""
    diff = make_diffusion()
    seen = []
    monkeypatch.setattr(diff, "_cached_sampler", lambda cache, key, *a, **k: seen.append((cache, key)) or key)
    unet, shape = object(), (2, 4, 3, 8, 8)

    def keys(clip):
        return (diff._graph_sampler(unet, shape, clip, rule=("ddim", 0.0)),
                diff._known_region_sampler(unet, shape, clip, ("ddim", 0.0), True))

    off = keys(True)
    diff.set_dynamic_threshold(0.995)
    on = keys(True)
    diff.set_dynamic_threshold(0.995, max_value=1.5)
    capped = keys(True)
    assert len({off[0], on[0], capped[0]}) == 3 and len({off[1], on[1], capped[1]}) == 3
    assert on[0][:4] == off[0][:4] and on[0][1] == shape and on[0][3] == ("ddim", 0.0), "positions 1 and 3 stay shape and rule"
    assert on[0][-1] == (0.995, None) and on[1][-1] == (0.995, None) and on[1][4] == "known" and off[0][-1] is None
    assert keys(False) == (off[0][:2] + (False,) + off[0][3:], off[1][:2] + (False,) + off[1][3:]), \
        "clip_denoised=False ignores the setting"
    diff.set_dynamic_threshold()
    assert keys(True) == off, "off again: the static samplers' keys"
    assert seen[0][0] is diff._samplers and seen[1][0] is diff._known_samplers


def test_eager_denoised_route_thresholds_with_the_reference_on_the_cpu():
    """``_update_denoised`` (the only route that runs without a GPU): denoised_fn first, then the reference in the clamp's
    place, over the frames of model_kwargs["latent_mask"]; clip_denoised=False: no thresholding, no clamp."""
    from improved_diffusion.gaussian_diffusion import dynamic_threshold_reference
    diff = make_diffusion("ddim10", predict_xstart=True)
    g = torch.Generator().manual_seed(3)
    x, out = torch.randn(2, 3, 1, 4, 4, generator=g), 3.0 * torch.randn(2, 3, 1, 4, 4, generator=g)
    lm = torch.tensor([[0.0, 1.0, 1.0], [1.0, 0.0, 0.0]]).view(2, 3, 1, 1, 1)
    t = torch.tensor([9, 4])
    net = lambda x_, timesteps=None, **kw: (out, None)      # noqa: E731
    fn = lambda v: 0.5 * v                                  # noqa: E731
    static = diff.ddim_sample(net, x, t, model_kwargs={"latent_mask": lm}, denoised_fn=fn)
    assert torch.equal(static["pred_xstart"], (0.5 * out).clamp(-1, 1))
    diff.set_dynamic_threshold(0.9)
    dyn = diff.ddim_sample(net, x, t, model_kwargs={"latent_mask": lm}, denoised_fn=fn)
    want = dynamic_threshold_reference(0.5 * out, lm, 0.9, None)
    assert torch.equal(dyn["pred_xstart"], want) and not torch.equal(want, static["pred_xstart"])
    assert not torch.equal(want, dynamic_threshold_reference(0.5 * out, None, 0.9, None)), "the mask steers the threshold"
    raw = diff.ddim_sample(net, x, t, clip_denoised=False, model_kwargs={"latent_mask": lm}, denoised_fn=fn)
    assert torch.equal(raw["pred_xstart"], 0.5 * out)
