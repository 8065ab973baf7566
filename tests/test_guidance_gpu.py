"""Classifier-free guidance on the observed frames on the MI355X.  The op (lfvdm_cfg_combine) against host copies of the same
fp32 values - xhat bitwise, s_c / s_g within ``std_bound`` of float64 (tests/test_guidance_cpu.py: the derivation), f within the
rounding of its operations - then the replayed and the eager steps of every rule on the micro model.

Two figures of the float64 step test go into DESIGN.md section 6: the kernel's error and the fp32 model's.

Where a test compares a replayed step with the public per-step methods BITWISE, the per-step method is handed the network
output of that very step (``plan.out``, all 2B rows) through a stub model, as tests/test_dyn_threshold_gpu.py does."""
import functools
import math

import pytest
import torch

from test_oracle_golden import load_case
from test_forward_gpu import build_native
from test_guidance_cpu import RULES, U, make_case, make_diffusion, masks_for, std_bound

pytestmark = pytest.mark.gpu

# the shapes of the threshold tests (a vector tail, more than one chunk per sample, B = 1), then two whose rows start off the
# 16-byte grid while B * inner is a multiple of 4: scalar leads of 0..3 elements, and a second chunk of a single quad
SHAPES = [(2, 3, 4), (3, 5, 37), (2, 20, 1024), (1, 5, 49152), (4, 3, 5), (4, 1, 4103)]
WS = [0.0, 0.5, 2.0, 7.5]
PHIS = [0.3, 0.7, 1.0]
ids = lambda s: "x".join(map(str, s))      # noqa: E731


def bits(a):
    return a.contiguous().view(torch.int32)


class Op:
    def __init__(self, shape, eps):
        from improved_diffusion import _native as nat
        self.nat, self.shape, self.eps = nat, shape, eps
        B, T, F = shape
        diff = make_diffusion()
        self.tb, self.dd = diff.tables("cuda"), diff.ddim_tables("cuda", 0.0)
        self.r, self.rm1 = self.tb["sqrt_recip_alphas_cumprod"], self.tb["sqrt_recipm1_alphas_cumprod"]
        self.t = torch.tensor([9, 4, 0, 6][:B], device="cuda")
        self.nch = max(1, math.ceil((T * F // 4) / 1024))
        # a DIRTY workspace: never zero-filled
        self.ws = torch.full((nat.cfg_workspace(B, T * F),), 0xA5, dtype=torch.uint8, device="cuda")

    def __call__(self, x, out2, mask, w, phi, fma=False, ws=None):
        nat = self.nat
        xhat = torch.full_like(x, float("nan"))
        stats = torch.full((x.shape[0], 3), float("nan"), device="cuda")
        nat.cfg_combine(x, out2, self.t, self.r if self.eps else None, self.rm1 if self.eps else None,
                        nat.MEAN_EPS if self.eps else nat.MEAN_X0, fma, mask, w, phi, xhat, stats, self.ws if ws is None else ws)
        return xhat, stats

    def x0hat(self, x, o, fma):
        """x0-hat of ``o`` (device fp32) as the update cell of that rounding writes it (clip = 0): the ancestral cell rounds
        both products, the deterministic DDIM cell evaluates one fma."""
        nat, tb, dd = self.nat, self.tb, self.dd
        if not self.eps:
            return o.clone()
        sample, pred = torch.empty_like(x), torch.full_like(x, float("nan"))
        if fma:
            nat.update_x0(x, o, None, self.t, self.r, self.rm1, dd["k1"], dd["k2"], None, nat.RULE_DDIM, nat.MEAN_EPS, False,
                          sample, pred)
        else:
            nat.update_x0(x, o, x, self.t, self.r, self.rm1, tb["posterior_mean_coef1"], tb["posterior_mean_coef2"],
                          tb["model_log_variance"], nat.RULE_ANCESTRAL, nat.MEAN_EPS, False, sample, pred)
        return pred


def guided_host(out2, w):
    """o_g = o_u + w (o_c - o_u) on the host: three fp32 statements in the kernel's order"""
    B = out2.shape[0] // 2
    o_c, o_u = out2[:B], out2[B:]
    d = o_c - o_u
    m = torch.tensor(w, dtype=torch.float32) * d
    return o_u + m


@pytest.mark.parametrize("eps", [True, False], ids=["eps", "x0"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_op_without_rescale_is_the_fp32_statements_bitwise(shape, eps):
    B, T, F = shape
    op = Op(shape, eps)
    xh, out2h = make_case("gauss", shape)
    x, out2 = xh.cuda(), out2h.cuda()
    for w in WS:
        o_g = guided_host(out2h, w)
        for fma in ((False, True) if eps else (False,)):
            want = op.x0hat(x, o_g.cuda(), fma)
            if eps and not fma:      # and the two-product form once more, entirely on the host
                tb = op.t.cpu()
                host = op.r.cpu()[tb].view(B, 1, 1) * xh - op.rm1.cpu()[tb].view(B, 1, 1) * o_g
                assert torch.equal(bits(host), bits(want.cpu()))
            for name, mask in masks_for(B, T).items():
                xhat, stats = op(x, out2, None if mask is None else mask.cuda(), w, 0.0, fma)
                assert torch.equal(bits(xhat), bits(want)), (w, fma, name, float((xhat - want).abs().max()))
                assert stats.cpu().tolist() == [[0.0, 0.0, 1.0]] * B
    # without a workspace at all
    xhat, stats = torch.full_like(x, float("nan")), torch.full((B, 3), float("nan"), device="cuda")
    op.nat.cfg_combine(x, out2, op.t, op.r, op.rm1, op.nat.MEAN_EPS if eps else op.nat.MEAN_X0, False, None, 2.0, 0.0, xhat, stats)
    assert torch.equal(bits(xhat), bits(op.x0hat(x, guided_host(out2h, 2.0).cuda(), False)))


@pytest.mark.parametrize("fma", [False, True], ids=["two_products", "fma"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_op_with_equal_halves_has_the_bits_of_the_update_cells(shape, fma):
    """o_u == o_c: o_g is o_c for every w, and xhat is the pred_xstart lfvdm_update_x0(clip = 0) writes for the same inputs
    - under the ancestral rule (x0hat_fma = 0) and under the deterministic DDIM rule (x0hat_fma = 1)."""
    B, T, F = shape
    op = Op(shape, True)
    xh, out2h = make_case("gauss", shape, 1)
    x, o = xh.cuda(), out2h[:B].cuda()
    p0 = op.x0hat(x, o, fma)
    assert float(p0.abs().max()) > 1.0
    for w in WS:
        xhat, stats = op(x, torch.cat([o, o]), None, w, 0.0, fma)
        assert torch.equal(bits(xhat), bits(p0)), w
        # with a rescale s_c and s_g are the same float, and f is 1 to the rounding of phi s / s + (1 - phi)
        xhat, stats = op(x, torch.cat([o, o]), None, w, 0.7, fma)
        assert torch.equal(stats[:, 0], stats[:, 1]) and float((stats[:, 2] - 1.0).abs().max()) <= 2 * U


@pytest.mark.parametrize("kind", ["gauss", "offcentre"])
@pytest.mark.parametrize("eps", [True, False], ids=["eps", "x0"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_op_with_rescale(shape, eps, kind):
    """s_c, s_g against the float64 std of the same fp32 values within ``std_bound``; f within the rounding of its
    operations (product, division, 1 - phi, sum: each 2^-24 relative); xhat = x0hat_g f with the kernel's own f, bitwise.
    "offcentre" is the case of the CPU separation test."""
    B, T, F = shape
    op = Op(shape, eps)
    xh, out2h = make_case(kind, shape)
    x, out2 = xh.cuda(), out2h.cuda()
    fmas = (False, True) if eps else (False,)
    worst = 0.0
    for fma in fmas:
        h_c = op.x0hat(x, out2[:B], fma).cpu()
        for w in WS:
            h_g = op.x0hat(x, guided_host(out2h, w).cuda(), fma).cpu()
            for name, mask in masks_for(B, T).items():
                for phi in PHIS:
                    xhat, stats = op(x, out2, None if mask is None else mask.cuda(), w, phi, fma)
                    xhat, stats = xhat.cpu(), stats.cpu()
                    assert bool(torch.isfinite(xhat).all()) and bool(torch.isfinite(stats).all()), "outputs were NaN-filled"
                    phi32 = float(torch.tensor(phi, dtype=torch.float32))
                    for b in range(B):
                        keep = torch.ones(T, dtype=torch.bool) if mask is None else mask[b] != 0
                        s_c, s_g, f = (float(v) for v in stats[b])
                        if not bool(keep.any()):
                            assert (s_c, s_g, f) == (0.0, 0.0, 1.0)
                        else:
                            for got, v in ((s_c, h_c[b][keep]), (s_g, h_g[b][keep])):
                                v64 = v.double().reshape(-1)
                                s64 = float(v64.std(unbiased=False))
                                bound = std_bound(v64, op.nch) if s64 > 0 else 0.0
                                assert abs(got - s64) <= bound * s64, (name, w, phi, b, got, s64, bound)
                                worst = max(worst, abs(got - s64) / s64 / bound if s64 > 0 else 0.0)
                            if s_g == 0.0:
                                assert f == 1.0
                            else:
                                q = phi32 * s_c / s_g
                                f64 = q + (1.0 - phi32)
                                assert abs(f - f64) <= U * (2 * q + (1.0 - phi32) + f64) * 1.01, (f, f64)
                        want = h_g[b] * stats[b, 2]
                        assert torch.equal(bits(xhat[b]), bits(want)), (name, w, phi, b)
    print(f"[cfg std {kind} {shape} {'eps' if eps else 'x0'}] worst |s - s64| / s64 = {worst:.3f} of the bound")


def test_op_is_reproducible_whatever_the_workspace_holds():
    shape = (2, 20, 1024)
    op = Op(shape, True)
    xh, out2h = make_case("offcentre", shape)
    x, out2 = xh.cuda(), out2h.cuda()
    mask = masks_for(2, 20)["subset"].cuda()
    a = op(x, out2, mask, 2.0, 0.7)
    b = op(x, out2, mask, 2.0, 0.7)
    c = op(x, out2, mask, 2.0, 0.7, ws=torch.zeros_like(op.ws))
    other = op(*(v.cuda() for v in make_case("gauss", shape)), None, 7.5, 1.0)
    d = op(x, out2, mask, 2.0, 0.7)
    for got in (b, c, d):
        assert torch.equal(bits(got[0]), bits(a[0])) and torch.equal(bits(got[1]), bits(a[1]))
    assert not torch.equal(other[0], a[0])


def test_refusals_launch_nothing():
    from improved_diffusion import _native as nat
    shape = (2, 3, 4)
    op = Op(shape, True)
    xh, out2h = make_case("gauss", shape)
    x, out2 = xh.cuda(), out2h.cuda()
    xhat, stats = torch.full_like(x, float("nan")), torch.full((2, 3), float("nan"), device="cuda")
    L, p = nat.lib(), nat.ptr
    args = [p(x), p(out2), p(op.t, torch.int64), p(op.r), p(op.rm1), nat.MEAN_EPS, 0, None, 2.0, 0.5, p(xhat), p(stats),
            p(op.ws, torch.uint8), 2, 3, 4, nat.stream()]
    bad = [(i, None) for i in (0, 1, 2, 3, 4, 10, 11, 12)]                               # a required pointer missing
    bad += [(5, 5), (5, -1)]                                                             # an unknown mean type
    bad += [(8, -0.5), (8, float("inf")), (8, float("nan")), (9, -0.1), (9, 1.5), (9, float("nan"))]      # scale, rescale
    bad += [(13, 0), (13, -2), (13, 40000), (14, 0), (15, 0), (15, 2 ** 31)]             # B, T, frame_inner
    for i, v in bad:
        a = list(args)
        a[i] = v
        assert L.lfvdm_cfg_combine(*a) == 1, (i, v)
    n = __import__("ctypes").c_size_t(7)
    assert L.lfvdm_cfg_workspace(0, 12, n) == 1 and L.lfvdm_cfg_workspace(2, 0, n) == 1 and L.lfvdm_cfg_workspace(2, 12, None) == 1
    with pytest.raises(RuntimeError, match="invalid shape"):
        nat.cfg_combine(x, out2, op.t, op.r, op.rm1, nat.MEAN_EPS, False, None, 2.0, 0.5, xhat, stats, None)
    torch.cuda.synchronize()
    assert bool(torch.isnan(xhat).all()) and bool(torch.isnan(stats).all()) and bool((op.ws == 0xA5).all())
    assert L.lfvdm_cfg_combine(*args) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xhat).all()) and bool(torch.isfinite(stats).all())


# ------------------------------------------------------------------------------------------------ steps and chains
@functools.lru_cache(maxsize=None)
def micro():
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd).eval()
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    return model, d, mk, tuple(inp["x"].shape)


def _stub(out):
    return lambda x_, timesteps=None, **kw: (out, None)      # noqa: E731


def _eager(diff, rule, net, x, t, mk, noise, prev):
    with torch.no_grad():
        if rule[0] == "ancestral":
            return diff.p_sample(net, x, t, clip_denoised=True, model_kwargs=mk, noise=noise)
        if rule[0] == "ddim":
            return diff.ddim_sample(net, x, t, clip_denoised=True, model_kwargs=mk, eta=rule[1], noise=noise)
        return diff.dpm_solver_sample(net, x, t, clip_denoised=True, model_kwargs=mk, prev_pred_xstart=prev)


def _wiring(rule, px, phi=0.0, threshold=None):
    from improved_diffusion.gaussian_diffusion import GraphSampler
    model, d, mk, shape = micro()
    B, T = shape[:2]
    diff = make_diffusion(px)
    diff.set_guidance(3.0, phi)
    if threshold is not None:
        diff.set_dynamic_threshold(threshold)
    s = GraphSampler(diff, model, shape, True, inject_noise=True, rule=rule)
    s.begin(d["x"].clone(), mk)
    assert not s.plan.head_fused and s.plan.B == 2 * B and s.t_buf.shape == (B,) and s.guidance == (3.0, phi)
    obs = s.plan.obs.view(2 * B, T)
    assert torch.equal(obs[:B], d["obs_mask"].view(B, T)) and not bool(obs[B:].any()) and bool(obs[:B].any())
    g = torch.Generator().manual_seed(9)
    prev = None
    for j, i in enumerate(range(9, -1, -1)):
        noise = torch.randn(shape, generator=g).cuda()
        s.noise.copy_(noise)
        assert torch.equal(s.plan.x_in[B:], s.plan.x_in[:B])
        before = s.plan.x_in[:B].clone()
        out = s.step(i)
        assert out["sample"].shape == shape and s.plan.out.shape[0] == 2 * B
        t = torch.full((B,), i, device="cuda", dtype=torch.long)
        ref = _eager(diff, rule, _stub(s.plan.out.clone()), before, t, mk, noise, prev)
        assert torch.equal(out["pred_xstart"], ref["pred_xstart"]), (j, float((out["pred_xstart"] - ref["pred_xstart"]).abs().max()))
        assert torch.equal(out["sample"], ref["sample"]), (j, float((out["sample"] - ref["sample"]).abs().max()))
        assert torch.equal(s.cfg_stats, diff.last_guidance_stats)
        if threshold is not None:
            assert torch.equal(s.dyn_stats, diff.last_threshold_stats)
        assert torch.equal(s.plan.x_in[B:], s.plan.x_in[:B]), "the new state is mirrored into the second half"
        assert bool((s.clock == max(i, 0)).all())
        prev = out["pred_xstart"].clone()
    return s


@pytest.mark.parametrize("px", [False, True], ids=["eps", "x0"])
@pytest.mark.parametrize("rule", RULES, ids=lambda r: "-".join(map(str, r)))
def test_replayed_chain_is_the_eager_public_step_bitwise(rule, px):
    s = _wiring(rule, px)
    assert s.cfg_stats.cpu().tolist() == [[0.0, 0.0, 1.0]] * 2


def test_replayed_chain_with_rescale_and_with_the_threshold_on_top():
    s = _wiring(("ddim", 1.0), False, phi=0.7)
    assert bool((s.cfg_stats[:, 2] != 1.0).all()) and bool((s.cfg_stats[:, :2] > 0).all())
    s = _wiring(("ancestral",), False, threshold=0.995)
    assert s.threshold == (0.995, None) and bool((s.dyn_stats[:, 2] >= 1.0).all())


def test_known_region_sampler_blend_resample_and_mirror():
    from improved_diffusion.gaussian_diffusion import GraphSampler, _Known
    model, d, mk, shape = micro()
    B, T, _, H, W = shape
    diff = make_diffusion()
    diff.set_guidance(3.0)
    known = (0.8 * torch.randn(shape, generator=torch.Generator().manual_seed(17))).cuda()
    mask = (torch.rand(B, T, H, W, generator=torch.Generator().manual_seed(18)) < 0.5).float().cuda()
    mask = mask * d["latent_mask"].view(B, T, 1, 1)
    s = GraphSampler(diff, model, shape, True, inject_noise=True, rule=("ancestral",))
    s.enable_known_region(False)
    s.begin(d["x"].clone(), mk, known=known, known_mask=mask)
    g = torch.Generator().manual_seed(3)
    kn = _Known(known, mask, False, 2)
    for i in (9, 8, 0):
        noise = torch.randn(shape, generator=g).cuda()
        s.noise.copy_(noise)
        before = s.plan.x_in[:B].clone()
        out = s.step(i)
        t = torch.full((B,), i, device="cuda", dtype=torch.long)
        ref = _eager(diff, ("ancestral",), _stub(s.plan.out.clone()), before, t, mk, noise, None)
        want = diff._put_known_back(ref["sample"], kn, None, t, None, s.seed, False)
        assert torch.equal(out["sample"], want), i
        assert torch.equal(s.plan.x_in[B:], s.plan.x_in[:B])
        if i:
            s.renoise()
            want = diff._put_known_back(ref["sample"], kn, None, t, None, s.seed, True)
            assert torch.equal(s.plan.x_in[:B], want) and torch.equal(s.plan.x_in[B:], want), "re-noised and mirrored"
    # the public loop: where the mask is 1 the sample is the known video
    on = (d["latent_mask"] > 0).expand(shape)
    torch.manual_seed(5)
    full = diff.known_region_sample_loop(model, shape, known, torch.ones(1, 1, 1, 1, device="cuda"), sampler="ancestral",
                                         resample_steps=2, model_kwargs=mk, latent_mask=d["latent_mask"], return_decoded=False)
    assert torch.equal(full[on], known[on]) and bool(torch.isfinite(full).all())
    (ks,) = diff._known_samplers.values()
    assert ks.guidance == (3.0, 0.0) and ks.plan.B == 2 * B


@pytest.mark.parametrize("px", [False, True], ids=["eps", "x0"])
@pytest.mark.parametrize("rule", RULES, ids=lambda r: "-".join(map(str, r)))
def test_one_step_against_float64(rule, px):
    """One native step per rule (lfvdm_cfg_combine + the MEAN_X0 update with the static clamp) against ``_update_denoised``
    driven by ``guidance_reference`` on float64 copies of the same inputs.  Bound, the convention of DESIGN.md section 6: 4 x the
    error of the same statements evaluated in torch float32 against that float64 result.  Both figures are printed."""
    from improved_diffusion.gaussian_diffusion import guidance_reference, _bshape
    w, phi = 3.0, 0.7
    diff = make_diffusion(px)
    diff.set_guidance(w, phi)
    shape = (2, 4, 4, 16, 16)
    g = torch.Generator().manual_seed(31)
    x = (0.5 * torch.randn(shape, generator=g)).cuda()
    out2 = ((0.3 if px else 0.4) * torch.randn((4,) + shape[1:], generator=g)).cuda()
    hist = (0.3 * torch.randn(shape, generator=g)).cuda()
    noise = torch.randn(shape, generator=g).cuda()
    lm = torch.tensor([[0.0, 1, 1, 1], [0, 0, 1, 1]], device="cuda").view(2, 4, 1, 1, 1)
    t = torch.tensor([7, 3], device="cuda")
    mk = {"latent_mask": lm, "obs_mask": 1.0 - lm}
    got = _eager(diff, rule, _stub(out2), x, t, mk, noise, hist)
    h64 = hist.double() if rule[0] == "dpmpp2m" else None
    s64, p64, _ = diff._update_denoised(x.double(), out2.double(), t, noise.double(), True, None, rule, hist=h64, latent_mask=lm,
                                        guided=True)
    assert s64.dtype == torch.float64 and float(p64.abs().max()) <= 1.0 and float(p64.abs().min()) < 1.0

    def fp32_model():
        """the statements of _update_denoised under guidance, every one in float32"""
        recip, recipm1, c1, c2, sg, R, _ = diff._update_args(x.device, rule)
        pred = guidance_reference(x, out2, t, w, phi, lm, recip, recipm1, diff._x0hat_fma(diff._update_args(x.device, rule)),
                                  dtype=torch.float32).clamp(-1, 1)
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
        print(f"[cfg fp64 {rule} {'x0' if px else 'eps'}] {name}: kernel {ek:.3e}  fp32 model {em:.3e}  bound {4 * em:.3e}")
        assert ek <= 4 * em, (name, ek, em)


def test_the_second_half_is_the_unconditional_forward():
    from improved_diffusion.gaussian_diffusion import GraphSampler
    model, d, mk, shape = micro()
    B = shape[0]
    diff = make_diffusion()
    diff.set_guidance(2.0)
    s = GraphSampler(diff, model, shape, True, inject_noise=True, rule=("ddim", 0.0))
    s.begin(d["x"].clone(), mk)
    s.step(9)
    t = torch.full((B,), 9, device="cuda", dtype=torch.long)
    net = diff._wrap_model(model)
    with torch.no_grad():
        uncond, _ = net(d["x"], t, return_attn_weights=False, **dict(mk, obs_mask=torch.zeros_like(mk["obs_mask"])))
        cond, _ = net(d["x"], t, return_attn_weights=False, **mk)
    eu = float((s.plan.out[B:] - uncond).abs().max())
    ec = float((s.plan.out[:B] - cond).abs().max())
    apart = float((s.plan.out[B:] - s.plan.out[:B]).abs().max())
    print(f"[cfg forward] unconditional half vs eager {eu:.2e}, conditional half vs eager {ec:.2e}, the halves differ by {apart:.2e}")
    assert eu <= 2e-4 and ec <= 2e-4 and apart > 2e-4


def test_guided_chain_without_timestep_tables(monkeypatch):
    """A 2B plan asks the table budget for twice as much; where it does not fit, the plan runs the per-step embedding and RPE
    launches - on a chain longer than the R ring too - and the samples are bitwise those of the tabulated plan."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    model, d, mk, shape = micro()
    res = []
    for gb in ("12", "0.000001"):
        monkeypatch.setenv("LFVDM_TIME_TABLE_GB", gb)
        diff = make_diffusion(resp="250")
        diff.set_guidance(2.0, 0.5)
        s = GraphSampler(diff, model, shape, True, rule=("ddim", 0.0))
        s.begin(d["x"].clone(), mk)
        assert bool(s.plan.time_steps) == (gb == "12"), s.plan.time_table_fallback
        res.append(s.run(249, 12)["sample"].clone())
        del s
    assert bool(torch.isfinite(res[0]).all()) and torch.equal(res[0], res[1])


def _final(diff, rule, model, shape, noise, mk):
    if rule[0] == "ancestral":
        return diff.p_sample_loop(model, shape, noise=noise, model_kwargs=mk, return_decoded=False)[0]
    if rule[0] == "ddim":
        return diff.ddim_sample_loop(model, shape, noise=noise, model_kwargs=mk, eta=rule[1], return_decoded=False)
    return diff.dpm_solver_sample_loop(model, shape, noise=noise, model_kwargs=mk, return_decoded=False)


def test_off_after_on_is_the_static_sampler():
    model, d, mk, shape = micro()
    rule = ("ancestral",)
    diff = make_diffusion()
    torch.manual_seed(2)
    before = _final(diff, rule, model, shape, d["x"].clone(), mk)
    (s0,) = diff._samplers.values()
    launches, graph, fused = len(s0.plan.steps) + s0.extra_launches, id(s0.graph), s0.plan.head_fused
    diff.set_guidance(2.0)
    torch.manual_seed(2)
    on = _final(diff, rule, model, shape, d["x"].clone(), mk)
    assert len(diff._samplers) == 2 and not torch.equal(on, before) and on.shape == before.shape
    s1 = next(s for s in diff._samplers.values() if s is not s0)
    assert s1.guidance == (2.0, 0.0) and s0.guidance is None and s1.plan.B == 2 * s0.plan.B
    assert s1.extra_launches == s0.extra_launches + 2 + int(fused), "the combine and the mirror (and the un-fused update)"
    for off in (None, 1.0):
        diff.set_guidance(off)
        torch.manual_seed(2)
        after = _final(diff, rule, model, shape, d["x"].clone(), mk)
        assert list(diff._samplers.values())[-1] is s0 and len(diff._samplers) == 2
        assert len(s0.plan.steps) + s0.extra_launches == launches and id(s0.graph) == graph and s0.plan.head_fused == fused
        assert torch.equal(after, before)
    fresh = make_diffusion()
    torch.manual_seed(2)
    assert torch.equal(_final(fresh, rule, model, shape, d["x"].clone(), mk), before)


def test_training_loss_and_bound_terms_ignore_the_setting():
    model, d, mk, shape = micro()
    d0, d1 = make_diffusion(), make_diffusion()
    d1.set_guidance(4.0, 0.7)
    t = torch.tensor([7, 3], device="cuda")
    noise = torch.randn(shape, generator=torch.Generator().manual_seed(2)).cuda()
    res = []
    with torch.no_grad():
        for diff in (d0, d1):
            a = diff.training_losses(model, d["x0"], t, model_kwargs=mk, noise=noise, latent_mask=d["latent_mask"])
            b = diff._vb_terms_bpd(model, d["x0"], diff.q_sample(d["x0"], t, noise), t, model_kwargs=mk)
            c = diff.ddim_reverse_sample(model, d["x"], t, model_kwargs=mk)
            res.append({**{"l_" + k: v for k, v in a.items()}, **{"b_" + k: b[k] for k in ("output", "pred_xstart")},
                        **{"r_" + k: v for k, v in c.items()}})
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k


def test_public_loops_and_sample_video():
    from improved_diffusion.video_sampler import default_sampling_args, sample_video
    model, d, mk, shape = micro()
    diff = make_diffusion()
    diff.set_guidance(2.0, 0.5)
    for rule in (("ancestral",), ("ddim", 0.0), ("dpmpp2m",)):
        res = []
        for _ in range(2):
            torch.manual_seed(8)
            res.append(_final(diff, rule, model, shape, None, mk))
        assert res[0].shape == shape and bool(torch.isfinite(res[0]).all()) and torch.equal(res[0], res[1]), rule
    diff2 = make_diffusion()
    Tv, n_obs = 10, 2
    batch = (0.8 * torch.randn(2, Tv, 4, 16, 16, generator=torch.Generator().manual_seed(4))).cuda()
    args = default_sampling_args(sampling_scheme="autoreg", n_obs=n_obs, max_frames=6, max_latent_frames=4, device="cuda",
                                 guidance_scale=2)
    res = []
    for _ in range(2):
        torch.manual_seed(21)
        out, used = sample_video(args, model, diff2, batch, verbose=False)
        res.append(out)
    assert len(used) >= 2 and diff2.guidance == (2.0, 0.0)
    assert res[0].shape == batch.shape and bool(torch.isfinite(res[0]).all()) and torch.equal(res[0], res[1])
    assert torch.equal(res[0][:, :n_obs], batch[:, :n_obs]) and all(k[-1] == (2.0, 0.0) for k in diff2._samplers)
