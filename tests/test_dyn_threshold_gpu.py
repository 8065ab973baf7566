"""Dynamic thresholding of x0-hat on the MI355X.  The op (lfvdm_dyn_threshold) against torch on host copies of the same fp32
values - order statistics and xhat bitwise, s within four roundings of the float64 interpolation - on inputs chosen to break
a radix select; then the replayed and the eager steps of every rule on the micro model.

Two figures of the float64 step test go into DESIGN.md section 6: the kernel's error and the fp32 model's.

Where a test compares a replayed step with the public per-step methods BITWISE, the per-step method is handed the network
output of that very step (``plan.out``) through a stub model: the sampler's autotuned private plan and the eager model call are
two fp32 evaluations of the network, which the existing sampler tests grant 2e-4; what is pinned here is everything behind
the network output - threshold launches, the MEAN_X0 re-entry, noise and buffer wiring."""
import functools
import math

import numpy as np
import pytest
import torch

from test_oracle_golden import load_case
from test_forward_gpu import build_native

pytestmark = pytest.mark.gpu

PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
U = 2.0 ** -23
SHAPES = [(2, 3, 4), (3, 5, 37), (2, 20, 1024), (1, 5, 49152)]
PCTS = [0.25, 0.5, 0.995, 1.0]      # 0.25 and 0.5 of n_sel - 1 = 184 (3 x 5 x 37, no mask): pos an exact integer; 1.0 always
KINDS = ["gauss", "equal", "zeros", "lastdigit", "subnormal", "ties"]
RULES = [("ancestral",), ("ddim", 0.0), ("ddim", 1.0), ("dpmpp2m",)]


def make_diffusion(predict_xstart=False, resp="10"):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, rescale_timesteps=True, rescale_learned_sigmas=True,
                                        predict_xstart=predict_xstart, diffusion_space_kwargs=dict(PIXEL))


# ------------------------------------------------------------------------------------------------ the op
def make_input(kind, shape, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + sum(shape))
    n = int(np.prod(shape))
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    if kind == "gauss":
        v = 2.5 * torch.randn(n, generator=g)
    elif kind == "equal":
        v = 1.7 * sign
    elif kind == "zeros":      # half exact zeros, of both signs
        v = torch.where(torch.rand(n, generator=g) < 0.5, 0.0 * sign, 2.5 * torch.randn(n, generator=g))
    elif kind == "lastdigit":      # |.| patterns that agree in the top 22 bits: 1.5 + j 2^-23, j < 1024
        bits = 0x3FC00000 + torch.randint(0, 1024, (n,), generator=g, dtype=torch.int32)
        v = bits.view(torch.float32) * sign
    elif kind == "subnormal":      # subnormal patterns, the smallest normals, and values around 1e-38
        bits = torch.randint(0, 1 << 24, (n,), generator=g, dtype=torch.int32)
        v = torch.where(torch.rand(n, generator=g) < 0.7, bits.view(torch.float32), 1e-38 * torch.randn(n, generator=g)) * sign
    else:      # 70 % of the elements ARE the quantile value: count(<= v_lo) straddles k + 1 at every percentile above 0.15
        v = torch.where(torch.rand(n, generator=g) < 0.7, 2.0 * sign, 0.5 * torch.randn(n, generator=g))
    return v.reshape(shape).contiguous()


def masks_for(B, T):
    """NULL, all ones, a different subset per sample (never empty), one sample with an empty selection"""
    sub = torch.zeros(B, T)
    for b in range(B):
        sub[b, b % T::2] = 1.0 + b      # any non-zero value selects
    empty = sub.clone()
    empty[B - 1] = 0.0
    return {"null": None, "ones": torch.ones(B, T), "subset": sub, "empty": empty}


class Op:
    """One workspace per shape, zero-filled ONCE: every call of a test reuses it"""

    def __init__(self, shape):
        from improved_diffusion import _native as nat
        self.nat, self.shape = nat, shape
        B, T, F = shape
        self.ws = torch.zeros(nat.dyn_threshold_workspace(B, T * F), dtype=torch.uint8, device="cuda")
        self.t = torch.zeros(B, dtype=torch.int64, device="cuda")

    def __call__(self, out, mask, pct, max_value=None, x=None, t=None, recip=None, recipm1=None, mean=None, fma=False, ws=None):
        nat = self.nat
        xhat = torch.full_like(out, float("nan"))
        stats = torch.full((out.shape[0], 3), float("nan"), device="cuda")
        nat.dyn_threshold(out if x is None else x, out, self.t if t is None else t, recip, recipm1,
                          nat.MEAN_X0 if mean is None else mean, fma, mask, pct, max_value, xhat, stats, self.ws if ws is None else ws)
        return xhat, stats


def check_against_host(p0, mask, pct, max_value, xhat, stats):
    """p0: host fp32 (B, T, F); the assertions of the op's contract"""
    B, T, F = p0.shape
    xhat, stats = xhat.cpu(), stats.cpu()
    assert bool(torch.isfinite(xhat).all()) and bool(torch.isfinite(stats).all()), "outputs were pre-filled with NaN"
    for b in range(B):
        keep = torch.ones(T, dtype=torch.bool) if mask is None else mask[b] != 0
        v = p0[b][keep].abs().reshape(-1).sort().values
        n = v.numel()
        v_lo, v_hi, s = stats[b]
        if n == 0:
            assert (float(v_lo), float(v_hi), float(s)) == (0.0, 0.0, 1.0)
        else:
            pos = pct * (n - 1)
            k = min(int(math.floor(pos)), n - 1)
            want_lo, want_hi = v[k], v[min(k + 1, n - 1)]
            assert v_lo.view(torch.int32) == want_lo.view(torch.int32), (b, n, k, float(v_lo), float(want_lo))
            assert v_hi.view(torch.int32) == want_hi.view(torch.int32), (b, n, k, float(v_hi), float(want_hi))
            q64 = float(want_lo) + (float(want_hi) - float(want_lo)) * (pos - k)
            s64 = max(q64, 1.0) if max_value is None else min(max(q64, 1.0), max_value)
            assert abs(float(s) - s64) <= 4 * U * max(float(want_hi), 1.0), (b, float(s), s64)
            if pos == k:
                assert float(s) == s64, "an integer position: no interpolation"
        want = torch.minimum(torch.maximum(p0[b], -s), s) / s
        assert torch.equal(xhat[b].view(torch.int32), want.view(torch.int32)), (b, float((xhat[b] - want).abs().max()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_x0_mode_against_host_sort(shape, kind):
    B, T, F = shape
    op = Op(shape)
    p0 = make_input(kind, shape)
    out = p0.cuda()
    exact = 0
    for name, mask in masks_for(B, T).items():
        m = None if mask is None else mask.cuda()
        for pct in PCTS:
            xhat, stats = op(out, m, pct)
            check_against_host(p0, mask, pct, None, xhat, stats)
            n = T * F if mask is None else int((mask[0] != 0).sum()) * F
            exact += n > 0 and pct * (n - 1) == math.floor(pct * (n - 1)) and pct < 1.0
    assert exact or shape != (3, 5, 37), "0.25 / 0.5 of 184 are exact integer positions"
    if kind == "gauss":      # the cap, and aliasing xhat with model_out
        xhat, stats = op(out, None, 0.995, max_value=1.25)
        check_against_host(p0, None, 0.995, 1.25, xhat, stats)
        assert float(stats[:, 2].max()) == 1.25
        buf, st = out.clone(), torch.full((B, 3), float("nan"), device="cuda")
        op.nat.dyn_threshold(buf, buf, op.t, None, None, op.nat.MEAN_X0, False, None, 0.995, 1.25, buf, st, op.ws)
        assert torch.equal(buf, xhat) and torch.equal(st, stats)


@pytest.mark.parametrize("fma", [False, True], ids=["two_products", "fma"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_eps_mode_has_the_bits_of_the_update_cells(shape, fma):
    """MEAN_EPS: p0 is the pred_xstart lfvdm_update_x0(clip = 0) writes for the same inputs - under the ancestral rule
    (x0hat_fma = 0) and under the deterministic DDIM rule (x0hat_fma = 1) - so the order statistics and xhat are compared
    bitwise for this mean type too."""
    from improved_diffusion import _native as nat
    B, T, F = shape
    diff = make_diffusion()
    tb, dd = diff.tables("cuda"), diff.ddim_tables("cuda", 0.0)
    r, rm1 = tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"]
    x, eps = make_input("gauss", shape, 1).cuda(), (0.4 * make_input("gauss", shape, 2)).cuda()
    t = torch.tensor([9, 4, 0][:B], device="cuda")
    sample, pred = torch.empty_like(x), torch.full_like(x, float("nan"))
    if fma:
        nat.update_x0(x, eps, None, t, r, rm1, dd["k1"], dd["k2"], None, nat.RULE_DDIM, nat.MEAN_EPS, False, sample, pred)
    else:
        nat.update_x0(x, eps, x, t, r, rm1, tb["posterior_mean_coef1"], tb["posterior_mean_coef2"], tb["model_log_variance"],
                      nat.RULE_ANCESTRAL, nat.MEAN_EPS, False, sample, pred)
    p0 = pred.cpu()
    assert float(p0.abs().max()) > 1.0
    op = Op(shape)
    for name, mask in masks_for(B, T).items():
        m = None if mask is None else mask.cuda()
        for pct in (0.5, 0.995):
            xhat, stats = op(eps, m, pct, x=x, t=t, recip=r, recipm1=rm1, mean=nat.MEAN_EPS, fma=fma)
            check_against_host(p0, mask, pct, None, xhat, stats)


def test_op_is_reproducible_and_hands_its_workspace_back():
    shape = (2, 20, 1024)
    op = Op(shape)
    out = make_input("ties", shape).cuda()
    mask = masks_for(2, 20)["subset"].cuda()
    a = op(out, mask, 0.6)
    b = op(out, mask, 0.6)                      # the same workspace, not re-zeroed
    fresh = torch.zeros_like(op.ws)
    c = op(out, mask, 0.6, ws=fresh)
    other = op(make_input("gauss", shape).cuda(), None, 0.995)      # other data in between
    d = op(out, mask, 0.6)
    for got in (b, c, d):
        assert torch.equal(got[0].view(torch.int32), a[0].view(torch.int32)) and torch.equal(got[1], a[1])
    assert not torch.equal(other[0], a[0])


def test_refusals_launch_nothing():
    from improved_diffusion import _native as nat
    shape = (2, 3, 4)
    op = Op(shape)
    diff = make_diffusion()
    tb = diff.tables("cuda")
    r, rm1 = tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"]
    out = make_input("gauss", shape).cuda()
    xhat, stats = torch.full_like(out, float("nan")), torch.full((2, 3), float("nan"), device="cuda")
    bad = [dict(mean=5), dict(mean=-1), dict(mean=nat.MEAN_EPS), dict(mean=nat.MEAN_EPS, recip=r), dict(pct=0.0), dict(pct=-0.5),
           dict(pct=1.5), dict(pct=float("nan")), dict(max_value=0.5), dict(max_value=float("nan"))]
    for kw in bad:
        kw = dict(dict(mean=nat.MEAN_X0, recip=None, recipm1=None, pct=0.9, max_value=None), **kw)
        with pytest.raises(RuntimeError, match="invalid shape"):
            nat.dyn_threshold(out, out, op.t, kw["recip"], kw["recipm1"], kw["mean"], False, None, kw["pct"], kw["max_value"], xhat,
                              stats, op.ws)
    L, p = nat.lib(), nat.ptr
    args = [p(out), p(out), p(op.t, torch.int64), None, None, nat.MEAN_X0, 0, None, 2, 3, 4, 0.9, float("inf"), p(xhat), p(stats),
            p(op.ws, torch.uint8), nat.stream()]
    for i in (0, 1, 2, 13, 14, 15):      # a required pointer missing
        a = list(args)
        a[i] = None
        assert L.lfvdm_dyn_threshold(*a) == 1
    for i, v in ((8, 0), (8, 70000), (9, 0), (10, 0), (10, 2 ** 31)):      # B, T, frame_inner out of range
        a = list(args)
        a[i] = v
        assert L.lfvdm_dyn_threshold(*a) == 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(xhat).all()) and bool(torch.isnan(stats).all()) and not bool(op.ws.any())
    assert L.lfvdm_dyn_threshold(*args) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xhat).all())


# ------------------------------------------------------------------------------------------------ steps and chains
@functools.lru_cache(maxsize=None)
def micro():
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd).eval()
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    return model, d, mk, tuple(inp["x"].shape)


def progressive(diff, rule, model, shape, noise, mk):
    if rule[0] == "ancestral":
        gen = diff.p_sample_loop_progressive(model, shape, noise=noise, clip_denoised=True, model_kwargs=mk)
    elif rule[0] == "ddim":
        gen = diff.ddim_sample_loop_progressive(model, shape, noise=noise, clip_denoised=True, model_kwargs=mk, eta=rule[1])
    else:
        gen = diff.dpm_solver_sample_loop_progressive(model, shape, noise=noise, clip_denoised=True, model_kwargs=mk)
    return [(o["sample"], o["pred_xstart"]) for o in gen]


@pytest.mark.parametrize("px", [False, True], ids=["eps", "x0"])
@pytest.mark.parametrize("rule", RULES, ids=lambda r: "-".join(map(str, r)))
def test_cap_of_one_is_the_static_clip_chain_with_a_two_launch_head(rule, px, monkeypatch):
    """set_dynamic_threshold(0.995, max_value=1.0) forces s = 1: ten replayed steps with in-kernel noise under one seed are
    bitwise the static-clip chain captured with LFVDM_FUSED_HEAD=0 - the un-fused head, the MEAN_X0 re-entry, the rounding
    of x0-hat per rule and the buffer wiring.  Fresh diffusion objects: the environment is read at capture."""
    model, d, mk, shape = micro()
    monkeypatch.setenv("LFVDM_FUSED_HEAD", "0")
    static, dyn = make_diffusion(px), make_diffusion(px)
    dyn.set_dynamic_threshold(0.995, max_value=1.0)
    torch.manual_seed(4)
    want = progressive(static, rule, model, shape, d["x"].clone(), mk)
    torch.manual_seed(4)
    got = progressive(dyn, rule, model, shape, d["x"].clone(), mk)
    assert len(want) == len(got) == 10
    for j, ((ws, wp), (gs, gp)) in enumerate(zip(want, got)):
        assert torch.equal(gp, wp), (j, float((gp - wp).abs().max()))
        assert torch.equal(gs, ws), (j, float((gs - ws).abs().max()))
    (ss,), (sd,) = static._samplers.values(), dyn._samplers.values()
    assert not ss.plan.head_fused and not sd.plan.head_fused and sd.threshold == (0.995, 1.0) and ss.threshold is None
    assert len(sd.plan.steps) == len(ss.plan.steps) and sd.extra_launches == ss.extra_launches + 4
    assert float(sd.dyn_stats[:, 2].min()) == 1.0 == float(sd.dyn_stats[:, 2].max())


def _stub(out):
    return lambda x_, timesteps=None, **kw: (out, None)      # noqa: E731


@pytest.mark.parametrize("px", [False, True], ids=["eps", "x0"])
@pytest.mark.parametrize("rule", RULES, ids=lambda r: "-".join(map(str, r)))
def test_replayed_chain_is_the_eager_public_step_bitwise(rule, px):
    """max_value=None, injected noise, ten replayed steps; after each, the public per-step method on the state the step
    started from and the network output it saw (module docstring) gives the same sample and pred_xstart to the last bit,
    and (v_lo, v_hi, s) agree.  s >= 1 at every step and > 1 at the first step of an epsilon model."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    model, d, mk, shape = micro()
    diff = make_diffusion(px)
    diff.set_dynamic_threshold(0.995)
    s = GraphSampler(diff, model, shape, True, inject_noise=True, rule=rule)
    s.begin(d["x"].clone(), mk)
    assert not s.plan.head_fused
    g = torch.Generator().manual_seed(9)
    prev, moved = None, 0
    for j, i in enumerate(range(9, -1, -1)):
        noise = torch.randn(shape, generator=g).cuda()
        s.noise.copy_(noise)
        before = s.plan.x_in.clone()
        out = s.step(i)
        net = _stub(s.plan.out.clone())
        t = torch.full((shape[0],), i, device="cuda", dtype=torch.long)
        with torch.no_grad():
            if rule[0] == "ancestral":
                ref = diff.p_sample(net, before, t, clip_denoised=True, model_kwargs=mk, noise=noise)
            elif rule[0] == "ddim":
                ref = diff.ddim_sample(net, before, t, clip_denoised=True, model_kwargs=mk, eta=rule[1], noise=noise)
            else:
                ref = diff.dpm_solver_sample(net, before, t, clip_denoised=True, model_kwargs=mk, prev_pred_xstart=prev)
        assert torch.equal(out["pred_xstart"], ref["pred_xstart"]), (j, float((out["pred_xstart"] - ref["pred_xstart"]).abs().max()))
        assert torch.equal(out["sample"], ref["sample"]), (j, float((out["sample"] - ref["sample"]).abs().max()))
        assert torch.equal(s.dyn_stats, diff.last_threshold_stats)
        sc = s.dyn_stats[:, 2].cpu()
        print(f"[dyn {rule} {'x0' if px else 'eps'}] step {j} (t={i}): s = {sc.tolist()}")
        assert bool((sc >= 1.0).all())
        moved += int(bool((sc > 1.0).any()))
        if j == 0 and not px:
            assert bool((sc > 1.0).all()), "x0-hat of an epsilon model is large at the top of the chain: the path is exercised"
        assert float(out["pred_xstart"].abs().max()) <= 1.0
        prev = out["pred_xstart"].clone()
    assert moved or px
    # the window's latent frames steer the threshold, the observed ones do not: the mask was uploaded by begin()
    assert torch.equal(s.frame_mask, d["latent_mask"].reshape(s.frame_mask.shape))
    assert bool((s.frame_mask == 0).any()) and bool((s.frame_mask != 0).any())


@pytest.mark.parametrize("px", [False, True], ids=["eps", "x0"])
@pytest.mark.parametrize("rule", RULES, ids=lambda r: "-".join(map(str, r)))
def test_one_step_against_float64(rule, px):
    """One native step per rule (lfvdm_dyn_threshold + the MEAN_X0 update) against ``_update_denoised`` driven by
    ``dynamic_threshold_reference`` on float64 copies of the same inputs.  Bound, the convention of DESIGN.md section 6: 4 x the
    error of the same statements evaluated in torch float32 against that float64 result.  Both figures are printed."""
    from improved_diffusion.gaussian_diffusion import dynamic_threshold_reference, _bshape
    diff = make_diffusion(px)
    diff.set_dynamic_threshold(0.995)
    shape = (2, 4, 4, 16, 16)
    x = make_input("gauss", shape, 3).mul(0.4).cuda()
    out = make_input("gauss", shape, 4).mul(1.2 if px else 0.4).cuda()
    hist = make_input("gauss", shape, 5).mul(0.3).cuda()
    noise = make_input("gauss", shape, 6).mul(0.4).cuda()
    lm = torch.tensor([[0.0, 1, 1, 1], [0, 0, 1, 1]], device="cuda").view(2, 4, 1, 1, 1)
    t = torch.tensor([7, 3], device="cuda")
    net, mk = _stub(out), {"latent_mask": lm}
    with torch.no_grad():
        if rule[0] == "ancestral":
            got = diff.p_sample(net, x, t, model_kwargs=mk, noise=noise)
        elif rule[0] == "ddim":
            got = diff.ddim_sample(net, x, t, model_kwargs=mk, eta=rule[1], noise=noise)
        else:
            got = diff.dpm_solver_sample(net, x, t, model_kwargs=mk, prev_pred_xstart=hist)
    assert float(diff.last_threshold_stats[:, 2].min()) > 1.0
    h64 = hist.double() if rule[0] == "dpmpp2m" else None
    s64, p64, _ = diff._update_denoised(x.double(), out.double(), t, noise.double(), True, lambda v: v, rule, hist=h64,
                                        latent_mask=lm)

    def fp32_model():
        """the statements of _update_denoised, every one in float32"""
        pred = dynamic_threshold_reference(diff._xstart_from_output(x, t, out), lm, 0.995, None, dtype=torch.float32)
        _, _, c1, c2, sg, R, _ = diff._update_args(x.device, rule)
        mean = _bshape(c1[t], 5) * pred + _bshape(c2[t], 5) * x
        if rule[0] == "dpmpp2m":
            k3 = _bshape(sg[t], 5)
            return torch.where(k3 != 0, mean + k3 * (pred - hist), mean), pred
        if sg is None:
            return mean, pred
        sigma = torch.exp(0.5 * sg[t]) if rule[0] == "ancestral" else sg[t]
        return mean + _bshape((t != 0).float() * sigma, 5) * noise, pred
    s32, p32 = fp32_model()
    for name, g_, m32, r64 in (("sample", got["sample"], s32, s64), ("pred_xstart", got["pred_xstart"], p32, p64)):
        ek, em = float((g_.double() - r64).abs().max()), float((m32.double() - r64).abs().max())
        print(f"[dyn fp64 {rule} {'x0' if px else 'eps'}] {name}: kernel {ek:.3e}  fp32 model {em:.3e}  bound {4 * em:.3e}")
        assert ek <= 4 * em, (name, ek, em)


@pytest.mark.parametrize("name,rule", [("ancestral", ("ancestral",)), ("ddim", ("ddim", 0.0)), ("dpm_solver", ("dpmpp2m",))])
def test_known_region_sampling_with_thresholding(name, rule):
    model, d, mk, shape = micro()
    B, T, _, H, W = shape
    lat = d["latent_mask"]
    on = (lat > 0).expand(shape)
    known = (0.8 * torch.randn(shape, generator=torch.Generator().manual_seed(17))).cuda()
    diff = make_diffusion()
    diff.set_dynamic_threshold(0.995)
    kr = lambda m: diff.known_region_sample_loop(model, shape, known, m, sampler=name, clip_denoised=True, model_kwargs=mk,      # noqa: E731
                                                 latent_mask=lat, return_decoded=False)
    torch.manual_seed(5)
    full = kr(torch.ones(1, 1, 1, 1, device="cuda"))
    assert torch.equal(full[on], known[on]) and bool(torch.isfinite(full).all())
    torch.manual_seed(4)
    none = kr(torch.zeros(B, T, H, W, device="cuda"))
    torch.manual_seed(4)
    plain = progressive(diff, rule, model, shape, None, mk)[-1][0]
    assert torch.equal(none, plain), "an empty known mask: the plain dynamic chain of the same seed"
    (ps,), (ks,) = diff._samplers.values(), diff._known_samplers.values()
    assert ps.threshold == ks.threshold == (0.995, None)
    assert len(ks.plan.steps) + ks.extra_launches == len(ps.plan.steps) + ps.extra_launches + 1, "the blend stays last, and counted"
    static = make_diffusion()
    torch.manual_seed(4)
    assert not torch.equal(progressive(static, rule, model, shape, None, mk)[-1][0], plain), "thresholding moved the result"


def test_off_after_on_is_the_static_sampler():
    """Thresholding off after having been on, same diffusion object: the sampler built BEFORE the setting was ever touched
    is found again - same object, same graphs, same launch count - and gives the same bytes."""
    model, d, mk, shape = micro()
    rule = ("ddim", 1.0)
    diff = make_diffusion()
    torch.manual_seed(2)
    before = progressive(diff, rule, model, shape, d["x"].clone(), mk)[-1][0]
    (s0,) = diff._samplers.values()
    launches, graph = len(s0.plan.steps) + s0.extra_launches, id(s0.graph)
    diff.set_dynamic_threshold(0.9)
    torch.manual_seed(2)
    on = progressive(diff, rule, model, shape, d["x"].clone(), mk)[-1][0]
    assert len(diff._samplers) == 2 and not torch.equal(on, before)
    s1 = next(s for s in diff._samplers.values() if s is not s0)
    assert s1.threshold == (0.9, None) and s0.threshold is None
    assert len(s1.plan.steps) + s1.extra_launches == launches + 4 + int(s0.plan.head_fused)
    diff.set_dynamic_threshold()
    torch.manual_seed(2)
    after = progressive(diff, rule, model, shape, d["x"].clone(), mk)[-1][0]
    assert list(diff._samplers.values())[-1] is s0 and len(diff._samplers) == 2
    assert len(s0.plan.steps) + s0.extra_launches == launches and id(s0.graph) == graph
    assert torch.equal(after, before)
    fresh = make_diffusion()
    torch.manual_seed(2)
    assert torch.equal(progressive(fresh, rule, model, shape, d["x"].clone(), mk)[-1][0], before)
