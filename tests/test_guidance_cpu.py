"""Classifier-free guidance on the observed frames, host side: the parser and the setter, the plain-torch definition
(``guidance_reference``), the per-step methods on CPU tensors with a stub model, and the separation test for the inputs the
GPU op test uses (``make_case`` is shared with tests/test_guidance_gpu.py)."""
import math

import numpy as np
import pytest
import torch

PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
U = 2.0 ** -24            # unit roundoff of fp32
CHUNK = 4096 + 6          # elements one workgroup of lfvdm_cfg_combine sums: a chunk, plus the row's scalar lead and tail
RULES = [("ancestral",), ("ddim", 0.0), ("ddim", 1.0), ("dpmpp2m",)]


def make_diffusion(predict_xstart=False, resp="10"):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, rescale_timesteps=True, rescale_learned_sigmas=True,
                                        predict_xstart=predict_xstart, diffusion_space_kwargs=dict(PIXEL))


def make_case(kind, shape, seed=0):
    """(x, out2) host fp32 for (B, T, F): "gauss" - centred; "offcentre" - every value 1000 + N(0, 1): the x0-hat of an x0
    model (o_c and o_g alike, for every w) then has |mean| / std >= 64 over any selection."""
    B, T, F = shape
    g = torch.Generator().manual_seed(7919 * seed + sum(shape))
    x = 1.3 * torch.randn(B, T, F, generator=g)
    out2 = 0.6 * torch.randn(2 * B, T, F, generator=g)
    if kind == "offcentre":
        x, out2 = x + 1000.0, out2 / 0.6 + 1000.0
    return x.contiguous(), out2.contiguous()


def masks_for(B, T):
    """NULL, all ones, a different subset per sample (never empty), one sample with an empty selection"""
    sub = torch.zeros(B, T)
    for b in range(B):
        sub[b, b % T::2] = 1.0 + b      # any non-zero value selects
    empty = sub.clone()
    empty[B - 1] = 0.0
    return {"null": None, "ones": torch.ones(B, T), "subset": sub, "empty": empty}


def std_bound(v64, nch):
    """Relative bound on s_c / s_g of lfvdm_cfg_combine against the float64 population std of the SAME fp32 values ``v64``
    (given as float64), from the kernel's summation structure.  A workgroup sums at most L = CHUNK values twice in double
    (the sum, then the squared deviations from its own mean): relative error <= L 2^-53 each, and fl(v - mean) is exact
    relative to the difference, so an off-centre mean costs nothing inside a chunk.  The nch records are merged by Chan's
    formula in M = ceil(nch / 64) + 6 steps of eight double operations.  What an off-centre mean does cost: a chunk mean
    carries an absolute error L 2^-53 |mean|, which enters delta = mean_b - mean_a of a merge; the term delta^2 n_a n_b / n
    then moves the variance by at most 4 (|delta| / std)(L 2^-53 |mean| / std), |delta| <= the spread of the values.  The
    root is rounded to fp32 once: 2^-24.  (The bound is taken on the variance and applied to s, whose relative error is half.)"""
    s = float(v64.std(unbiased=False))
    ratio = abs(float(v64.mean())) / s
    spread = float(v64.max() - v64.min()) / s
    merges = math.ceil(nch / 64) + 6
    return U + 2.0 ** -53 * (2 * CHUNK + 8 * merges + 8) * (1.0 + 4.0 * ratio * spread)


# ------------------------------------------------------------------------------------------------ parser, setter, key
def test_parse_guidance():
    from improved_diffusion.gaussian_diffusion import parse_guidance
    assert parse_guidance("2") == {"scale": 2.0, "rescale": 0.0}
    assert parse_guidance(" 2 : 0.7 ") == {"scale": 2.0, "rescale": 0.7}
    assert parse_guidance("") == parse_guidance("none") == {"scale": None, "rescale": 0.0}
    assert parse_guidance("-3:9") == {"scale": -3.0, "rescale": 9.0}, "only the shape is judged: the setter validates"
    for bad in ("a", "2:b", "1:2:3", ":", "2:", 2.0, None):
        with pytest.raises(ValueError):
            parse_guidance(bad)


def test_set_guidance_validates_and_knows_what_off_is():
    from improved_diffusion.gaussian_diffusion import parse_guidance
    d = make_diffusion()
    assert d.guidance is None
    d.set_guidance(2.0, 0.7)
    assert d.guidance == (2.0, 0.7)
    d.set_guidance(0.0)
    assert d.guidance == (0.0, 0.0), "w = 0 is the unconditional model, not off"
    d.set_guidance(1.0, 0.5)
    assert d.guidance == (1.0, 0.5), "a rescale alone is on"
    for off in (dict(scale=None), dict(scale=1), dict(scale=1.0, rescale=0.0), parse_guidance(""), parse_guidance("1:0"),
                parse_guidance("none")):
        d.set_guidance(3.0)
        d.set_guidance(**off)
        assert d.guidance is None, off
    for bad in (dict(scale=-0.1), dict(scale=float("inf")), dict(scale=float("nan")), dict(scale=2, rescale=-0.1),
                dict(scale=2, rescale=1.1), dict(scale=2, rescale=float("nan")), dict(scale="x"), dict(scale=None, rescale=2)):
        d.set_guidance(3.0, 0.25)
        with pytest.raises(ValueError):
            d.set_guidance(**bad)
        assert d.guidance == (3.0, 0.25), "a refused call changes nothing"


def test_sampler_cache_keys(monkeypatch):
    """Without guidance the keys are the tuples they always were; with guidance one more element, last; [1] stays the shape."""
    d = make_diffusion()
    seen = []
    monkeypatch.setattr(type(d), "_cached_sampler", lambda self, cache, key, *a, **kw: seen.append(key) or key)
    unet, shape, rule = object(), (2, 4, 4, 16, 16), ("ddim", 0.0)
    d._graph_sampler(unet, shape, True, rule)
    d._known_region_sampler(unet, shape, True, rule, True)
    assert seen[0] == (id(unet), shape, True, rule, None, None)
    assert seen[1] == (id(unet), shape, True, rule, "known", None)
    d.set_guidance(2.0, 0.5)
    d.set_dynamic_threshold(0.9)
    d._graph_sampler(unet, shape, True, rule)
    d._known_region_sampler(unet, shape, True, rule, True)
    assert seen[2] == (id(unet), shape, True, rule, None, (0.9, None), (2.0, 0.5))
    assert seen[3] == (id(unet), shape, True, rule, "known", (0.9, None), (2.0, 0.5))
    d.set_guidance(1.0)
    d._graph_sampler(unet, shape, True, rule)
    assert seen[4] == seen[0][:5] + ((0.9, None),) and all(k[1] == shape for k in seen)


def test_resolve_guidance(monkeypatch):
    from types import SimpleNamespace
    from improved_diffusion.video_sampler import default_sampling_args, resolve_guidance
    monkeypatch.delenv("LFVDM_GUIDANCE", raising=False)
    a = default_sampling_args()
    assert a.guidance_scale is None and a.guidance_rescale is None and resolve_guidance(a) is None
    assert resolve_guidance(SimpleNamespace()) is None
    assert resolve_guidance(default_sampling_args(guidance_scale=2)) == {"scale": 2, "rescale": 0.0}
    assert resolve_guidance(default_sampling_args(guidance_scale=2, guidance_rescale=0.7)) == {"scale": 2, "rescale": 0.7}
    with pytest.raises(ValueError):
        resolve_guidance(default_sampling_args(guidance_rescale=0.7))
    monkeypatch.setenv("LFVDM_GUIDANCE", "3:0.5")
    assert resolve_guidance(a) == {"scale": 3.0, "rescale": 0.5}
    assert resolve_guidance(default_sampling_args(guidance_scale=2)) == {"scale": 2, "rescale": 0.0}, "args win"
    monkeypatch.setenv("LFVDM_GUIDANCE", "none")
    assert resolve_guidance(a) == {"scale": None, "rescale": 0.0}


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("px", [False, True], ids=["eps", "x0"])
def test_reference_identities_in_float64(px):
    from improved_diffusion.gaussian_diffusion import guidance_reference
    d = make_diffusion(px)
    B, T, F = 3, 5, 37
    x, out2 = (a.double() for a in make_case("gauss", (B, T, F), 1))
    t = torch.tensor([9, 4, 0])
    tb = d.tables("cpu")
    tabs = {} if px else dict(recip=tb["sqrt_recip_alphas_cumprod"].double(), recipm1=tb["sqrt_recipm1_alphas_cumprod"].double())
    plain = lambda o: d._xstart_from_output(x, t, o) if px else (      # noqa: E731
        tabs["recip"][t].view(B, 1, 1) * x - tabs["recipm1"][t].view(B, 1, 1) * o)
    o_c, o_u = out2[:B], out2[B:]
    same = torch.cat([o_c, o_c])
    for w in (0.0, 0.5, 2.0, 7.5):
        for phi in (0.0, 0.7):
            got, st = guidance_reference(x, same, t, w, phi, None, return_stats=True, **tabs)
            assert torch.equal(got, plain(o_c)) or float((got - plain(o_c)).abs().max()) <= 1e-13, "o_u == o_c: the plain x0-hat"
            assert phi == 0.0 or float((st[:, 2] - 1.0).abs().max()) <= 1e-13
    assert torch.equal(guidance_reference(x, out2, t, 0.0, **tabs), plain(o_u)), "w = 0: the unconditional x0-hat"
    assert torch.equal(guidance_reference(x, out2, t, 1.0, **tabs), plain(o_u + 1.0 * (o_c - o_u)))
    masks = masks_for(B, T)
    for name in ("null", "ones", "subset"):
        m = masks[name]
        got, st = guidance_reference(x, out2, t, 3.0, 1.0, m, return_stats=True, **tabs)
        for b in range(B):
            keep = torch.ones(T, dtype=torch.bool) if m is None else m[b] != 0
            s_sel = got[b][keep].std(unbiased=False)
            assert abs(float(s_sel) - float(st[b, 0])) <= 1e-12 * float(st[b, 0]), "phi = 1: the selected std is s_c"
            assert abs(float(plain(o_c)[b][keep].std(unbiased=False)) - float(st[b, 0])) <= 1e-12 * float(st[b, 0])
    got, st = guidance_reference(x, out2, t, 3.0, 0.7, masks["empty"], return_stats=True, **tabs)
    assert st[B - 1].tolist() == [0.0, 0.0, 1.0], "an empty selection: f = 1"
    assert torch.equal(got[B - 1], guidance_reference(x, out2, t, 3.0, **tabs)[B - 1])
    assert float(st[0, 2]) != 1.0
    assert guidance_reference(x.float(), out2.float(), t, 3.0, 0.7).dtype == torch.float32
    with pytest.raises(ValueError):
        guidance_reference(x, out2[:B], t, 3.0)


# ------------------------------------------------------------------------------------------------ the per-step methods
class Stub:
    def __init__(self, B, shape, seed=3):
        self.calls = []
        self.out = 0.5 * torch.randn((2 * B,) + tuple(shape[1:]), generator=torch.Generator().manual_seed(seed))

    def __call__(self, x, timesteps=None, **kw):
        self.calls.append((x, timesteps, kw))
        return self.out[:x.shape[0]], None

    def parameters(self):
        return iter([torch.zeros(1)])


def _window(shape, seed=5):
    B, T = shape[:2]
    g = torch.Generator().manual_seed(seed)
    obs = torch.tensor([[1.0, 0, 0, 0], [1, 1, 0, 0]]).view(B, T, 1, 1, 1)
    lat = torch.tensor([[0.0, 1, 1, 1], [0, 0, 1, 0]]).view(B, T, 1, 1, 1)
    mk = dict(frame_indices=torch.tensor([[0, 1, 2, 3], [5, 9, 12, 40]]), obs_mask=obs, latent_mask=lat,
              x0=torch.randn(shape, generator=g))
    return torch.randn(shape, generator=g), mk


@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("px", [False, True], ids=["eps", "x0"])
@pytest.mark.parametrize("rule", RULES, ids=lambda r: "-".join(map(str, r)))
def test_eager_step_on_cpu_tensors(rule, px, phi):
    """One model call on the doubled batch, built as the issue says; the result is ``_update_denoised`` driven by
    ``guidance_reference``; the stats are kept."""
    from improved_diffusion.gaussian_diffusion import guidance_reference
    shape = (2, 4, 3, 4, 4)
    B = shape[0]
    d = make_diffusion(px)
    d.set_guidance(3.0, phi)
    x, mk = _window(shape)
    t = torch.tensor([7, 3])
    g = torch.Generator().manual_seed(11)
    noise, hist = torch.randn(shape, generator=g), 0.3 * torch.randn(shape, generator=g)
    net = Stub(B, shape)
    if rule[0] == "ancestral":
        got = d.p_sample(net, x, t, model_kwargs=mk, noise=noise)
    elif rule[0] == "ddim":
        got = d.ddim_sample(net, x, t, model_kwargs=mk, eta=rule[1], noise=noise)
    else:
        got = d.dpm_solver_sample(net, x, t, model_kwargs=mk, prev_pred_xstart=hist)
    assert len(net.calls) == 1, "ONE model call"
    x2, ts2, kw2 = net.calls[0]
    assert x2.shape[0] == 2 * B and torch.equal(x2[:B], x) and torch.equal(x2[B:], x)
    assert ts2.shape == (2 * B,) and torch.equal(ts2[:B], ts2[B:])
    assert torch.equal(kw2["obs_mask"][:B], mk["obs_mask"]) and not bool(kw2["obs_mask"][B:].any())
    for k in ("frame_indices", "latent_mask", "x0"):
        assert torch.equal(kw2[k][:B], mk[k]) and torch.equal(kw2[k][B:], mk[k]), k
    tb = d.tables("cpu")
    tabs = {} if px else dict(recip=tb["sqrt_recip_alphas_cumprod"], recipm1=tb["sqrt_recipm1_alphas_cumprod"])
    xhat, st = guidance_reference(x, net.out, t, 3.0, phi, mk["latent_mask"], return_stats=True, **tabs)
    assert torch.equal(d.last_guidance_stats, st.float())
    # an x0 model's output from here on: _update_denoised of an x0-prediction twin of this diffusion
    twin = make_diffusion(True)
    s, p, _ = twin._update_denoised(x, xhat, t, noise, True, lambda v: v, rule, hist=hist if rule[0] == "dpmpp2m" else None,
                                    latent_mask=mk["latent_mask"])
    assert torch.allclose(got["pred_xstart"], p, rtol=0, atol=1e-6) and torch.allclose(got["sample"], s, rtol=0, atol=1e-6)
    assert float(got["pred_xstart"].abs().max()) <= 1.0


def test_setter_is_inert_for_training_and_the_bound(monkeypatch):
    """``training_losses`` and ``_vb_terms_bpd`` on CPU tensors with a stub model, guidance set and unset: the model is called
    with the very same B rows, timesteps and kwargs (compared bit for bit).  Their loss kernels are device launches, so the
    stub ends the call there; the results themselves are compared bitwise on the device by tests/test_guidance_gpu.py."""
    from improved_diffusion import _native as nat
    d0, d1 = make_diffusion(), make_diffusion()
    d1.set_guidance(4.0, 0.7)
    shape = (2, 4, 3, 4, 4)
    x, mk = _window(shape)
    t = torch.tensor([7, 3])
    noise = torch.randn(shape, generator=torch.Generator().manual_seed(2))

    def q_sample(x0, nz, tt, sa, sb, out):      # lfvdm_q_sample's statement in torch: the one launch in front of the model
        out.copy_(sa[tt].view(-1, 1, 1, 1, 1) * x0 + sb[tt].view(-1, 1, 1, 1, 1) * nz)
    monkeypatch.setattr(nat, "q_sample", q_sample)

    class Reached(Exception):
        pass

    seen = []

    def net(x_, timesteps=None, **kw):
        seen.append((x_.clone(), timesteps.clone(), {k: v.clone() for k, v in kw.items() if torch.is_tensor(v)}))
        raise Reached
    for d in (d0, d1):
        with pytest.raises(Reached):
            d.training_losses(net, x, t, model_kwargs=mk, noise=noise, latent_mask=mk["latent_mask"])
        with pytest.raises(Reached):
            d._vb_terms_bpd(net, x, d.q_sample(x, t, noise), t, model_kwargs=mk)
    assert len(seen) == 4
    for a, b in ((seen[0], seen[2]), (seen[1], seen[3])):
        assert a[0].shape[0] == 2 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2].keys() == b[2].keys()
        assert all(torch.equal(a[2][k], b[2][k]) for k in a[2]) and torch.equal(a[2]["obs_mask"], mk["obs_mask"])


def test_a_broadcast_obs_mask_is_expanded_before_it_is_zeroed():
    """``obs_mask`` with one row for all B samples: the doubled batch still has B conditional and B unconditional rows."""
    from improved_diffusion.gaussian_diffusion import GaussianDiffusion
    shape = (2, 4, 3, 4, 4)
    x, mk = _window(shape)
    kw = GaussianDiffusion._doubled_kwargs(dict(mk, obs_mask=mk["obs_mask"][:1]), 2)
    assert kw["obs_mask"].shape[0] == 4 and not bool(kw["obs_mask"][2:].any())
    assert torch.equal(kw["obs_mask"][0], mk["obs_mask"][0]) and torch.equal(kw["obs_mask"][1], mk["obs_mask"][0])
    for bad in (mk["obs_mask"][:1].expand(3, 4, 1, 1, 1), 1.0):
        with pytest.raises(ValueError):
            GaussianDiffusion._doubled_kwargs(dict(mk, obs_mask=bad), 2)
    with pytest.raises(ValueError):
        GaussianDiffusion._doubled_kwargs({k: v for k, v in mk.items() if k != "obs_mask"}, 2)


def test_reverse_ode_and_losses_do_not_double_the_batch_on_cpu():
    """What can be checked without a device: with guidance set, ``ddim_reverse_sample`` refuses nothing new and calls the
    model on B rows (it fails later, at the native update, exactly as it does without guidance)."""
    d = make_diffusion()
    d.set_guidance(4.0)
    shape = (2, 4, 3, 4, 4)
    x, mk = _window(shape)
    net = Stub(2, shape)
    with pytest.raises(RuntimeError, match="device"):
        d.ddim_reverse_sample(net, x, torch.tensor([7, 3]), model_kwargs=mk)
    assert len(net.calls) == 1 and net.calls[0][0].shape[0] == 2


# ------------------------------------------------------------------------------------------------ separation
def test_a_one_pass_fp32_variance_misses_the_kernels_bound_on_the_offcentre_case():
    """The GPU op test holds s_c / s_g to ``std_bound``.  On the off-centre case an fp32 E[v^2] - mean^2 misses that bound by
    more than 10 x; on the centred case it would have passed - so the off-centre case is what tells the two apart."""
    from improved_diffusion.gaussian_diffusion import guidance_reference
    shape = (2, 20, 1024)
    B, T, F = shape
    nch = math.ceil(T * F / 4 / 1024)
    t = torch.tensor([9, 4])
    for kind, want_miss in (("offcentre", True), ("gauss", False)):
        x, out2 = make_case(kind, shape)
        for w in (0.0, 2.0, 7.5):
            # x0-hat(o_g) of an x0 model in fp32 statements: the definition's float32 model (phi = 0: f = 1)
            v = guidance_reference(x, out2, t, w, 0.0, dtype=torch.float32)
            assert v.dtype == torch.float32
            for b in range(B):
                v64 = v[b].double().reshape(-1)
                s64 = float(v64.std(unbiased=False))
                ratio = abs(float(v64.mean())) / s64
                one_pass = (v[b] * v[b]).mean() - v[b].mean() * v[b].mean()
                s32 = float(one_pass.clamp(min=0).sqrt())
                miss = abs(s32 - s64) / s64 / std_bound(v64, nch)
                print(f"[separation {kind} w={w} b={b}] |mean|/std {ratio:.1f}  one-pass fp32 misses the bound by {miss:.3g} x")
                if want_miss:
                    assert ratio >= 64 and miss >= 10, (ratio, miss)
                    assert std_bound(v64, nch) <= 4 * U, "and the bound stays a few roundings"
                else:
                    assert miss < 10
