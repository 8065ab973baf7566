"""Known-region sampling without a GPU: the two C-ABI additions (declared, bound, exported, refusing bad shapes before any
launch), the float64 / fp32 tables, every refusal of the loop, the slow path on CPU tensors with a stand-in model, and the
signatures the feature must leave alone."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
NEW_EXPORTS = ("lfvdm_known_blend", "lfvdm_renoise")
SHAPE = (2, 3, 4, 4, 4)
E_SHAPE = 1


def make_diffusion(resp, steps=1000):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=steps, timestep_respacing=resp, rescale_timesteps=True,
                                        rescale_learned_sigmas=True, diffusion_space_kwargs=dict(PIXEL))


def net(x, timesteps=None, **kw):
    """The tiny stand-in model: predicts zero noise."""
    return torch.zeros_like(x), None


def identity(x):
    """A denoised_fn: sends the chain down the slow path, whose update is plain torch and runs on CPU tensors."""
    return x


def run(diff, known, mask, **kw):
    return diff.known_region_sample_loop(net, SHAPE, known, mask, denoised_fn=identity, model_kwargs={}, device="cpu",
                                         return_decoded=False, **kw)


def test_new_exports_are_declared_bound_and_built():
    from improved_diffusion import _native
    hdr = open(os.path.join(ROOT, "include", "lfvdm_hip.h")).read()
    declared = set(re.findall(r"\b(lfvdm_[a-z0-9_]+)\s*\(", hdr))
    assert os.path.exists(_native.LIB_PATH), "run `python __graft_entry__.py` (build) first"
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _native.EXPORTS and name in _native._SIGS, name
        assert hasattr(lib, name), name
    assert len(_native._SIGS["lfvdm_known_blend"][0]) == 14 and len(_native._SIGS["lfvdm_renoise"][0]) == 9
    assert callable(_native.known_blend) and callable(_native.renoise)
    # every export that was there keeps its argument count
    for name, nargs in zip(("lfvdm_update_x0", "lfvdm_update_rng_x0", "lfvdm_conv_out_update_x0", "lfvdm_update_ms_x0",
                            "lfvdm_conv_out_update_ms_x0", "lfvdm_q_sample"), (18, 19, 27, 16, 23, 9)):
        assert len(_native._SIGS[name][0]) == nargs, name
    assert lib.lfvdm_abi_version() == 9


def test_entries_refuse_bad_arguments_before_any_launch():
    """No device here: a launch would fail with LFVDM_E_LAUNCH (2), so LFVDM_E_SHAPE (1) shows the refusal came first."""
    from improved_diffusion import _native
    lib = _native.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)      # a non-null pointer; nothing is ever read through it
    blend = lambda x=p, known=p, mask=p, eps=None, t=p, a=p, s=p, seed=p, B=1, T=2, C=2, HW=4: lib.lfvdm_known_blend(
        x, known, mask, eps, None, t, a, s, seed, B, T, C, HW, None)
    for kw in (dict(x=None), dict(known=None), dict(mask=None), dict(t=None), dict(a=None), dict(s=None),
               dict(seed=None),                       # neither fixed noise nor a seed to draw with
               dict(B=0), dict(B=65536), dict(T=0), dict(C=-1), dict(HW=0),
               dict(T=1, C=1, HW=6), dict(T=3, C=3, HW=3), dict(eps=p, seed=None, T=1, C=2, HW=1)):
        assert blend(**kw) == E_SHAPE, kw
    renoise = lambda x=p, t=p, c=p, d=p, seed=p, B=1, inner=8: lib.lfvdm_renoise(x, None, t, c, d, seed, B, inner, None)
    for kw in (dict(x=None), dict(t=None), dict(c=None), dict(d=None), dict(seed=None), dict(B=0), dict(B=65536), dict(inner=0),
               dict(inner=6), dict(inner=9)):
        assert renoise(**kw) == E_SHAPE, kw


@pytest.mark.parametrize("resp", ["", "ddim50"])
def test_tables_against_float64_numpy(resp):
    diff = make_diffusion(resp)
    # the linear schedule restated (and, respaced, the betas of the kept timesteps' cumulative products)
    betas = np.linspace(1e-4, 0.02, 1000, dtype=np.float64)
    acp = np.cumprod(1.0 - betas)
    if resp:
        kept = np.asarray(diff.timestep_map)
        assert len(kept) == 50
        acp = acp[kept]
        betas = 1.0 - acp / np.append(1.0, acp[:-1])
    prev = np.append(1.0, acp[:-1])
    want = {"a": np.sqrt(prev), "s": np.sqrt(1.0 - prev), "sqrt_1mbeta": np.sqrt(1.0 - betas), "sqrt_beta": np.sqrt(betas)}
    co = diff.known_region_coefficients()
    tb = diff.known_region_tables("cpu")
    assert diff.known_region_tables("cpu") is tb, "uploaded once per device"
    assert set(tb) == set(want)
    for k, w in want.items():
        assert co[k].dtype == np.float64 and tb[k].dtype == torch.float32 and tuple(tb[k].shape) == (diff.num_timesteps,)
        np.testing.assert_allclose(co[k], w, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(tb[k].double().numpy(), w, rtol=2.0 ** -24, atol=0)      # one fp32 rounding
    a, s = tb["a"].double().numpy(), tb["s"].double().numpy()
    assert a[0] == 1.0 and s[0] == 0.0
    assert np.abs(a ** 2 + s ** 2 - 1.0).max() <= 2.0 ** -22
    c, d = tb["sqrt_1mbeta"].double().numpy(), tb["sqrt_beta"].double().numpy()
    assert np.abs(c ** 2 + d ** 2 - 1.0).max() <= 2.0 ** -22


def test_every_refusal():
    diff = make_diffusion("10")
    known, mask = torch.zeros(SHAPE), torch.ones(2, 3, 4, 4)
    bad = [
        (dict(known=torch.zeros(2, 3, 4, 4, 5)), "known has the shape"),
        (dict(mask=torch.ones(2, 3, 4, 5)), "known_mask broadcasts"),
        (dict(mask=torch.ones(2, 3, 4, 4, 4)), "known_mask broadcasts"),
        (dict(noise=torch.zeros(2, 3, 4, 4, 2)), "noise has the shape"),
        (dict(latent_mask=torch.ones(2, 4, 1, 1, 1)), "latent_mask"),
        (dict(mask=mask * 1.5), r"\[0, 1\]"),
        (dict(mask=mask - 1.25), r"\[0, 1\]"),
        (dict(mask=mask * float("nan")), r"\[0, 1\]"),
        (dict(known=known + float("inf")), "non-finite"),
        (dict(known=known * float("nan")), "non-finite"),
        (dict(sampler="heun"), "unknown sampler"),
        (dict(resample_steps=0), "resample_steps"),
        (dict(resample_steps=-2), "resample_steps"),
        (dict(resample_steps=1.5), "resample_steps"),
        (dict(sampler="ddim", resample_steps=2), "resample_steps"),
        (dict(sampler="dpm_solver", resample_steps=2), "resample_steps"),
    ]
    calls = []

    def counting(x, timesteps=None, **kw):
        calls.append(1)
        return net(x)
    for kw, msg in bad:
        kw = dict(kw)
        k, m = kw.pop("known", known), kw.pop("mask", mask)
        with pytest.raises(ValueError, match=msg):
            diff.known_region_sample_loop(counting, SHAPE, k, m, denoised_fn=identity, model_kwargs={}, device="cpu",
                                          return_decoded=False, **kw)
        # the progressive twin refuses when it is called, not at the first next()
        with pytest.raises(ValueError, match=msg):
            diff.known_region_sample_loop_progressive(counting, SHAPE, k, m, denoised_fn=identity, model_kwargs={},
                                                      device="cpu", **kw)
    assert not calls, "refused before the chain runs"


def test_return_decoded_is_refused_before_the_chain():
    from improved_diffusion import script_util as su
    diff = su.create_gaussian_diffusion(steps=1000, timestep_respacing="10", rescale_timesteps=True, rescale_learned_sigmas=True,
                                        diffusion_space_kwargs={"diffusion_space": "latent", "pre_encoded": False,
                                                                "pre_encoded_stats_dict": None})
    diff.vae = None      # whatever the environment configures: nothing to decode with
    assert not diff.can_decode()

    def never(*a, **kw):
        raise AssertionError("the chain ran")
    with pytest.raises(NotImplementedError, match="BEFORE the chain runs"):
        diff.known_region_sample_loop(never, SHAPE, torch.zeros(SHAPE), torch.ones(2, 3, 4, 4), model_kwargs={}, device="cpu")


@pytest.mark.parametrize("sampler,kw", [("ancestral", {}), ("ancestral", {"resample_steps": 3}), ("ddim", {}),
                                        ("ddim", {"eta": 1.0}), ("dpm_solver", {})])
def test_cpu_chain_with_a_full_mask_returns_known(sampler, kw):
    diff = make_diffusion("10")
    torch.manual_seed(1)
    known = torch.randn(SHAPE)
    out = run(diff, known, torch.ones(1, 1, 4, 4), sampler=sampler, **kw)
    assert torch.equal(out, known)


def test_cpu_chain_with_an_empty_mask_is_the_plain_loop():
    diff = make_diffusion("10")
    known = torch.full(SHAPE, 7.0)
    torch.manual_seed(5)
    got = run(diff, known, torch.zeros(2, 3, 4, 4))
    torch.manual_seed(5)
    want, _ = diff.p_sample_loop(net, SHAPE, denoised_fn=identity, model_kwargs={}, device="cpu", return_decoded=False)
    assert torch.equal(got, want)
    # and the latent mask empties a full known mask: frames that are not latent are never blended
    torch.manual_seed(5)
    got = run(diff, known, torch.ones(2, 3, 4, 4), latent_mask=torch.zeros(2, 3, 1, 1, 1))
    assert torch.equal(got, want)


def state_net(x, timesteps=None, **kw):
    """A stand-in whose output depends on the state (``net`` predicts zero noise whatever it is fed, which hides a step that
    was given the wrong state or taken in the wrong order)."""
    return 0.3 * x, None


# sampler= / eta= of the known-region loop, and the plain loop of the same rule with its per-step method and key set
CHAINS = {
    "ancestral": ("ancestral", {}, "p_sample_loop", "p_sample", {"sample", "pred_xstart", "attn"}),
    "ddim_eta0": ("ddim", {"eta": 0.0}, "ddim_sample_loop", "ddim_sample", {"sample", "pred_xstart"}),
    "ddim_eta1": ("ddim", {"eta": 1.0}, "ddim_sample_loop", "ddim_sample", {"sample", "pred_xstart"}),
    "dpm_solver": ("dpm_solver", {}, "dpm_solver_sample_loop", "dpm_solver_sample", {"sample", "pred_xstart"}),
}
CPU_KW = dict(denoised_fn=identity, model_kwargs={}, device="cpu")


def plain_final(diff, loop, kw):
    out = getattr(diff, loop)(state_net, SHAPE, return_decoded=False, **kw, **CPU_KW)
    return out[0] if loop == "p_sample_loop" else out


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_cpu_chain_with_an_empty_mask_is_the_plain_loop_of_every_sampler(chain):
    sampler, kw, loop, _, _ = CHAINS[chain]
    diff = make_diffusion("10")
    known, empty = torch.full(SHAPE, 7.0), torch.zeros(2, 3, 4, 4)
    torch.manual_seed(11)
    want = plain_final(diff, loop, kw)
    assert bool(torch.isfinite(want).all())
    torch.manual_seed(11)
    got = diff.known_region_sample_loop(state_net, SHAPE, known, empty, sampler=sampler, return_decoded=False, **kw, **CPU_KW)
    assert torch.equal(got, want)
    torch.manual_seed(11)
    last = list(diff.known_region_sample_loop_progressive(state_net, SHAPE, known, empty, sampler=sampler, **kw, **CPU_KW))[-1]
    assert torch.equal(last["sample"], want)


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_each_plain_loop_is_its_per_step_method_by_hand(chain):
    """The slow path's contract, whatever drives it: the start noise first, then the public per-step method for
    t = n-1 .. 0 on the sample of the step before, the multistep rule fed the x0-hat of the step before."""
    _, kw, loop, step, keys = CHAINS[chain]
    diff = make_diffusion("10")
    n = diff.num_timesteps
    torch.manual_seed(13)
    x, prev = torch.randn(*SHAPE), None
    for i in range(n - 1, -1, -1):
        t = torch.full((SHAPE[0],), i, dtype=torch.long)
        more = {"prev_pred_xstart": prev} if step == "dpm_solver_sample" else kw
        with torch.no_grad():
            out = getattr(diff, step)(state_net, x, t, clip_denoised=True, denoised_fn=identity, model_kwargs={}, **more)
        x, prev = out["sample"], out["pred_xstart"]
    assert bool(torch.isfinite(x).all())
    torch.manual_seed(13)
    assert torch.equal(plain_final(diff, loop, kw), x)
    torch.manual_seed(13)
    outs = list(getattr(diff, loop + "_progressive")(state_net, SHAPE, **kw, **CPU_KW))
    assert len(outs) == n and all(set(o) == keys for o in outs)
    assert torch.equal(outs[-1]["sample"], x) and torch.equal(outs[-1]["pred_xstart"], prev)


def test_the_chain_driver_and_its_timeout_text_exist_once():
    from improved_diffusion.gaussian_diffusion import GaussianDiffusion
    src = inspect.getsource(GaussianDiffusion)
    assert src.count("the states yielded since the last check are not valid") == 1
    assert not hasattr(GaussianDiffusion, "_known_region_steps") and not hasattr(GaussianDiffusion, "_sample_loop")
    assert inspect.isgeneratorfunction(GaussianDiffusion._chain)


def test_cpu_chain_blends_per_frame_and_per_pixel():
    """Left half known on the frames the latent mask names: exactly known there, the plain chain's values elsewhere are
    NOT reproduced (the model sees the blended state), but stay finite; the forward count under resampling is r (n-1) + 1."""
    diff = make_diffusion("10")
    torch.manual_seed(2)
    known = torch.randn(SHAPE)
    mask = torch.zeros(2, 3, 4, 4)
    mask[..., :2] = 1.0
    lat = torch.tensor([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0]]).view(2, 3, 1, 1, 1)
    calls = []

    def counting(x, timesteps=None, **kw):
        calls.append(1)
        return net(x)
    out = diff.known_region_sample_loop(counting, SHAPE, known, mask, resample_steps=2, denoised_fn=identity, model_kwargs={},
                                        device="cpu", latent_mask=lat, return_decoded=False)
    assert len(calls) == 2 * (diff.num_timesteps - 1) + 1
    on = (mask.unsqueeze(2) * lat).expand(SHAPE) == 1
    assert torch.equal(out[on], known[on]) and bool(torch.isfinite(out).all())
    assert not torch.equal(out[~on], known[~on])


def test_repeat_keys_wrap_like_int64_for_any_repeat_count():
    """Repeat k of a resampled timestep runs under seed + k * stride modulo 2^64.  The Python product leaves the 64-bit range
    at k = 5 and torch refuses a scalar beyond 64 bits (k >= 9 - RePaint's own r is 10): the offset handed to torch is the
    product reduced into the signed range, congruent to it, distinct per k, and the int64 tensor add takes it."""
    from improved_diffusion.gaussian_diffusion import GaussianDiffusion
    S = GaussianDiffusion._REPEAT_SEED_STRIDE
    assert S % 2 == 1, "an odd stride: k -> k * S is injective modulo 2^64"
    ks = list(range(0, 300)) + [1000, 12345, 2 ** 31, 2 ** 40 + 7]
    offs = [GaussianDiffusion._repeat_seed_offset(k) for k in ks]
    assert offs[0] == 0 and len(set(offs)) == len(ks)
    wrap = lambda v: ((v + 2 ** 63) % 2 ** 64) - 2 ** 63
    for seed in (0, 1, 2 ** 63 - 1, 20221201):      # seed.random_() gives [0, 2^63)
        s = torch.tensor([seed], dtype=torch.int64)
        for k, o in zip(ks, offs):
            assert -2 ** 63 <= o < 2 ** 63 and (o - k * S) % 2 ** 64 == 0
            assert int(torch.add(s, o)) == wrap(seed + k * S), (seed, k)
            assert int(s + o) == wrap(seed + k * S)


def test_progressive_yields_one_state_per_timestep():
    diff = make_diffusion("10")
    known = torch.zeros(SHAPE)
    outs = list(diff.known_region_sample_loop_progressive(net, SHAPE, known, torch.ones(2, 3, 4, 4), resample_steps=2,
                                                          denoised_fn=identity, model_kwargs={}, device="cpu"))
    assert len(outs) == diff.num_timesteps and all(set(o) == {"sample", "pred_xstart"} for o in outs)
    assert torch.equal(outs[-1]["sample"], known)


def test_pinned_signatures_are_unchanged():
    from improved_diffusion.gaussian_diffusion import GaussianDiffusion, GraphSampler
    from improved_diffusion.video_sampler import sample_video
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(GaussianDiffusion.__init__) == ["self", "betas", "model_mean_type", "model_var_type", "loss_type",
                                                 "rescale_timesteps", "diffusion_space_kwargs"]
    assert names(GraphSampler.__init__) == ["self", "diffusion", "unet", "shape", "clip_denoised", "inject_noise", "rule"]
    assert names(GaussianDiffusion._graph_sampler) == ["self", "unet", "shape", "clip_denoised", "rule"]
    sv = inspect.signature(sample_video).parameters
    assert list(sv)[:6] == ["args", "model", "diffusion", "batch", "just_get_indices", "verbose"]
    assert sv["just_get_indices"].default is False and sv["verbose"].default is True
    assert list(sv)[6:] == ["known_video", "known_mask"] and sv["known_video"].default is None and sv["known_mask"].default is None
    kr = inspect.signature(GaussianDiffusion.known_region_sample_loop).parameters
    assert list(kr)[:5] == ["self", "model", "shape", "known", "known_mask"]
    assert all(kr[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(kr)[5:])
    assert kr["sampler"].default == "ancestral" and kr["resample_steps"].default == 1 and kr["eta"].default == 0.0
    # the sampler's begin still takes (img, model_kwargs) alone
    assert names(GraphSampler.begin)[:3] == ["self", "img", "model_kwargs"]
    assert all(p.default is None for p in list(inspect.signature(GraphSampler.begin).parameters.values())[3:])


def test_sample_video_refuses_half_a_known_region():
    from improved_diffusion.video_sampler import sample_video, default_sampling_args
    args = default_sampling_args(device="cpu", n_obs=1, max_frames=3)
    batch = torch.zeros(1, 4, 4, 4, 4)
    with pytest.raises(ValueError, match="come together"):
        sample_video(args, net, make_diffusion("10"), batch, known_video=batch)
    with pytest.raises(ValueError, match="known_mask is"):
        sample_video(args, net, make_diffusion("10"), batch, known_video=batch, known_mask=torch.ones(1, 4, 4))
