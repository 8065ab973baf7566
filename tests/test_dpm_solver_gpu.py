"""DPM-Solver++(2M) on the MI355X: the two multistep entries through the C ABI against a float64 evaluation of the folded
formula (tables of GaussianDiffusion.dpm_solver_coefficients), their bitwise relation to the deterministic DDIM cell, the
replayed and the eager chain at cfg B for an epsilon and an x0 model, sample_video and the denoised_fn route.  The reference
has no such sampler: the yardsticks are the formula in float64 and the project's own DDIM step."""
import functools

import numpy as np
import pytest
import torch

from oracle import recipe
from test_oracle_golden import load_case
from test_forward_gpu import build_native

pytestmark = pytest.mark.gpu

PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
ATOL = 2e-4     # what tests/test_ddim_gpu.py and tests/test_sampler_gpu.py grant an update against float64
DENSE, RAGGED = (6, 2, 4, 8, 8), (6, 1, 3, 5, 7)      # inner 512; inner 105: no multiple of 4, the stand-alone entry's tail


def make_diffusion(resp, predict_xstart=False):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, rescale_timesteps=True, rescale_learned_sigmas=True,
                                        predict_xstart=predict_xstart, diffusion_space_kwargs=dict(PIXEL))


@functools.lru_cache(maxsize=None)
def cfgB():
    cfg, sd, inp = load_case("cfgB")
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    return model, d, mk, tuple(inp["x"].shape)


# ------------------------------------------------------------------------------------------------ the update kernels
def _rows(diff):
    """t = 0, 1 (k3 = 0 by decision), 2 (the largest k3), the middle, n - 2 (the first second-order step), n - 1 (no history)"""
    n = diff.num_timesteps
    return np.array([0, 1, 2, n // 2, n - 2, n - 1])


@functools.lru_cache(maxsize=None)
def _op_inputs(shape):
    """x, model output, history: gaussianish, the history at the scale of an x0-hat"""
    n = int(np.prod(shape))
    return tuple(np.float32(sc * recipe.gaussianish(f"dpm/op/{shape[-1]}/{k}", n)).reshape(shape)
                 for k, sc in (("x", 1.0), ("out", 1.0), ("hist", 0.7)))


def _formula(dt, diff, tv, x, out, hist, eps_mode, clip):
    """sample, x0-hat of the folded rule in dtype ``dt`` (float32: tables rounded first, as the device holds them)"""
    co = diff.dpm_solver_coefficients()
    f = lambda a: np.asarray(a)[tv].astype(dt).reshape((-1,) + (1,) * (x.ndim - 1))      # noqa: E731
    x, out = x.astype(dt), out.astype(dt)
    p0 = f(diff.sqrt_recip_alphas_cumprod) * x - f(diff.sqrt_recipm1_alphas_cumprod) * out if eps_mode else out
    if clip:
        p0 = np.clip(p0, -1, 1)
    s = f(co["k1"]) * p0 + f(co["k2"]) * x
    if hist is not None:
        k3 = f(co["k3"])
        s = np.where(k3 != 0, s + k3 * (p0 - np.nan_to_num(hist.astype(dt))), s)
    return s, p0


def _tabs(diff, eps_mode):
    from improved_diffusion import _native as nat
    tb, co = diff.tables("cuda"), diff.dpm_solver_tables("cuda")
    r, rm1 = (tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"]) if eps_mode else (None, None)
    return r, rm1, co["k1"], co["k2"], co["k3"], (nat.MEAN_EPS if eps_mode else nat.MEAN_X0)


def _ms(x, out, hist, t, tabs, clip, sample=None, pred=None):
    from improved_diffusion import _native as nat
    r, rm1, k1, k2, k3, M = tabs
    sample = torch.full_like(x, float("nan")) if sample is None else sample
    pred = torch.full_like(x, float("nan")) if pred is None else pred
    nat.update_ms_x0(x, out, hist, t, r, rm1, k1, k2, k3, M, clip, sample, pred)
    return sample, pred


def _ddim_det(x, out, t, tabs, clip):
    from improved_diffusion import _native as nat
    r, rm1, k1, k2, _, M = tabs
    sample, pred = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    nat.update_x0(x, out, None, t, r, rm1, k1, k2, None, nat.RULE_DDIM, M, clip, sample, pred)
    return sample, pred


@pytest.mark.parametrize("shape", [DENSE, RAGGED], ids=["inner512", "inner105"])
@pytest.mark.parametrize("eps_mode", [True, False], ids=["eps", "x0"])
def test_update_entry_against_float64_and_the_ddim_cell(shape, eps_mode):
    """lfvdm_update_ms_x0 on ddim50, clip on and off.  The float32 numpy evaluation of the same formula has to be within
    ATOL / 3 of float64 (so ATOL bounds the kernel, not the conditioning of the inputs: x0-hat = r x - rm1 eps has r = 130 at
    t = n - 1); sample and x0-hat against float64 at ATOL; rows with k3 = 0 bitwise the deterministic DDIM cell with a NaN
    history; hist aliasing pred and x aliasing sample bitwise the out-of-place call; hist = None bitwise DDIM in every row."""
    diff = make_diffusion("ddim50")
    tv = _rows(diff)
    k3 = diff.dpm_solver_coefficients()["k3"][tv]
    first = np.flatnonzero(k3 == 0)
    assert first.tolist() == [0, 1, 5] and np.all(k3[[2, 3, 4]] > 0)
    xn, on, hn = _op_inputs(shape)
    x, out, hist = (torch.from_numpy(a).cuda() for a in (xn, on, hn))
    t = torch.from_numpy(tv).cuda()
    tabs = _tabs(diff, eps_mode)
    nan_hist = hist.clone()
    nan_hist[torch.from_numpy(first).cuda()] = float("nan")
    for clip in (0, 1):
        s64, p64 = _formula(np.float64, diff, tv, xn, on, hn, eps_mode, clip)
        s32, p32 = _formula(np.float32, diff, tv, xn, on, hn, eps_mode, clip)
        e32 = max(float(np.abs(s32 - s64).max()), float(np.abs(p32 - p64).max()))
        assert e32 <= ATOL / 3, e32
        if clip:
            share = float((np.abs(p64) >= 1).mean())
            assert 0.02 < share < 0.98, share
        sample, pred = _ms(x, out, hist, t, tabs, clip)
        torch.cuda.synchronize()
        es = float(np.abs(sample.double().cpu().numpy() - s64).max())
        ep = float(np.abs(pred.double().cpu().numpy() - p64).max())
        print(f"[ms op {'eps' if eps_mode else 'x0'} inner={x[0].numel()} clip={clip}] sample {es:.2e} pred_xstart {ep:.2e} "
              f"(fp32 numpy {e32:.2e}; worst {max(es, ep) / ATOL:.3f} of bound)")
        assert es <= ATOL and ep <= ATOL
        ds, dp = _ddim_det(x, out, t, tabs, clip)
        sn, pn = _ms(x, out, nan_hist, t, tabs, clip)
        assert torch.equal(sn, sample) and torch.equal(pn, pred), "a row with k3 = 0 never reads its history"
        for b in first.tolist():
            assert torch.equal(sample[b], ds[b]) and torch.equal(pred[b], dp[b]), f"row {b}: the deterministic DDIM cell"
        for b in (2, 3, 4):
            assert not torch.equal(sample[b], ds[b]) and torch.equal(pred[b], dp[b])
        xin, hp = x.clone(), hist.clone()
        _ms(xin, out, hp, t, tabs, clip, sample=xin, pred=hp)
        assert torch.equal(xin, sample) and torch.equal(hp, pred), "in place: hist is pred, x is sample"
        s0, p0 = _ms(x, out, None, t, tabs, clip)
        assert torch.equal(s0, ds) and torch.equal(p0, dp), "no history: first order in every row"


def test_bad_mean_type_or_missing_tables_are_refused():
    from improved_diffusion import _native as nat
    diff = make_diffusion("ddim50")
    x = torch.zeros(2, 1, 4, 4, 4, device="cuda")
    t = torch.zeros(2, dtype=torch.int64, device="cuda")
    r, rm1, k1, k2, k3, _ = _tabs(diff, True)
    for bad in (5, -1):
        with pytest.raises(RuntimeError, match="invalid shape"):
            nat.update_ms_x0(x, x, x, t, r, rm1, k1, k2, k3, bad, True, torch.empty_like(x))
    with pytest.raises(RuntimeError, match="invalid shape"):        # epsilon needs its two tables
        nat.update_ms_x0(x, x, x, t, None, None, k1, k2, k3, nat.MEAN_EPS, True, torch.empty_like(x))
    with pytest.raises(RuntimeError, match="invalid shape"):        # k3 is required even where no history is given
        nat.update_ms_x0(x, x, None, t, r, rm1, k1, k2, None, nat.MEAN_EPS, True, torch.empty_like(x))
    act = torch.zeros(2 * 1 * 4 * 4, 64, device="cuda")
    wp, bias = torch.zeros(4, 9, 64, device="cuda"), torch.zeros(4, device="cuda")
    with pytest.raises(RuntimeError, match="invalid shape"):
        nat.conv_out_update_ms_x0(act, wp, bias, None, x, x, t, r, rm1, k1, k2, k3, 5, True, torch.empty_like(x))
    with pytest.raises(RuntimeError, match="invalid shape"):
        nat.conv_out_update_ms_x0(act, wp, bias, None, x, x, t, None, None, k1, k2, k3, nat.MEAN_EPS, True, torch.empty_like(x))


def _one_hot_head(out, C=64):
    """Channels-last rows and packed filters [Cout][9][C] whose 3x3 convolution IS ``out`` (centre tap, channel co -> co)."""
    B, T, Co, H, W = out.shape
    act = torch.zeros(B * T * H * W, C, device="cuda")
    act[:, :Co] = out.permute(0, 1, 3, 4, 2).reshape(-1, Co)
    wp = torch.zeros(Co, 9, C, device="cuda")
    for co in range(Co):
        wp[co, 4, co] = 1.0
    return act, wp, torch.zeros(Co, device="cuda")


def _fused(head, x, hist, t, tabs, clip, sample=None, pred=None):
    from improved_diffusion import _native as nat
    r, rm1, k1, k2, k3, M = tabs
    act, wp, bias = head
    assert nat.lib().lfvdm_conv_out_psample_ok(x.shape[0] * x.shape[1], x.shape[3], x.shape[4], act.shape[1], x.shape[2]) == 0
    conv = torch.full_like(x, float("nan"))
    sample = torch.full_like(x, float("nan")) if sample is None else sample
    pred = torch.full_like(x, float("nan")) if pred is None else pred
    nat.conv_out_update_ms_x0(act, wp, bias, conv, x, hist, t, r, rm1, k1, k2, k3, M, clip, sample, pred)
    return sample, pred, conv


@pytest.mark.parametrize("eps_mode", [False, True], ids=["x0", "eps"])
def test_fused_head_on_a_dense_activation(eps_mode):
    """lfvdm_conv_out_update_ms_x0 on a dense synthetic activation (C = 64, all nine taps, a bias), as
    test_xstart_gpu.test_fused_head_on_a_dense_activation: its convolution output against a float64 convolution at ATOL, and
    sample / x0-hat against the float64 update.  x0 mode: the update OF the float64 convolution.  Epsilon mode multiplies
    the convolution's own fp32 summation error (576 terms) by sqrt_recipm1 = 130 at t = n - 1, which is the conditioning of
    x0-hat and not the update's error: there the float64 update is that of the convolution output the kernel reports."""
    diff = make_diffusion("ddim50")
    tv = _rows(diff)
    xn, _, hn = _op_inputs(DENSE)
    x, hist = torch.from_numpy(xn).cuda(), torch.from_numpy(hn).cuda()
    t = torch.from_numpy(tv).cuda()
    B, T, Co, H, W = DENSE
    C = 64
    act = torch.from_numpy(recipe.gaussianish("dpm/head/act", B * T * H * W * C).reshape(B * T * H * W, C).astype(np.float32))
    wp = torch.from_numpy((recipe.gaussianish("dpm/head/w", Co * 9 * C) / 24.0).reshape(Co, 9, C).astype(np.float32))
    bias = torch.from_numpy((0.1 * recipe.gaussianish("dpm/head/b", Co)).astype(np.float32))
    w64 = wp.double().view(Co, 3, 3, C).permute(0, 3, 1, 2)
    a64 = act.double().view(B * T, H, W, C).permute(0, 3, 1, 2)
    e64 = torch.nn.functional.conv2d(a64, w64, bias.double(), padding=1).view(B, T, Co, H, W).numpy()
    assert 0.02 < float((np.abs(e64) > 1).mean()) < 0.6
    tabs = _tabs(diff, eps_mode)
    head = (act.cuda(), wp.cuda(), bias.cuda())
    for clip in (0, 1):
        sample, pred, conv = _fused(head, x, hist, t, tabs, clip)
        torch.cuda.synchronize()
        cv = conv.double().cpu().numpy()
        s64, p64 = _formula(np.float64, diff, tv, xn, cv if eps_mode else e64, hn, eps_mode, clip)
        ec = float(np.abs(cv - e64).max())
        es = float(np.abs(sample.double().cpu().numpy() - s64).max())
        ep = float(np.abs(pred.double().cpu().numpy() - p64).max())
        print(f"[ms dense head {'eps' if eps_mode else 'x0'} clip={clip}] conv {ec:.2e} sample {es:.2e} pred_xstart {ep:.2e} "
              f"(worst {max(ec, es, ep) / ATOL:.3f} of bound)")
        assert max(ec, es, ep) <= ATOL


@pytest.mark.parametrize("eps_mode", [False, True], ids=["x0", "eps"])
def test_fused_head_with_a_one_hot_head_is_the_stand_alone_entry(eps_mode):
    from improved_diffusion import _native as nat
    diff = make_diffusion("ddim50")
    tv = _rows(diff)
    x, out, hist = (torch.from_numpy(a).cuda() for a in _op_inputs(DENSE))
    t = torch.from_numpy(tv).cuda()
    tabs = _tabs(diff, eps_mode)
    head = _one_hot_head(out)
    for clip in (0, 1):
        want_s, want_p = _ms(x, out, hist, t, tabs, clip)
        sample, pred, conv = _fused(head, x, hist, t, tabs, clip)
        assert torch.equal(conv, out), "the convolution's own output is the given model output"
        assert torch.equal(sample, want_s) and torch.equal(pred, want_p)
        xin, hp = x.clone(), hist.clone()
        _fused(head, xin, hp, t, tabs, clip, sample=xin, pred=hp)
        assert torch.equal(xin, want_s) and torch.equal(hp, want_p), "in place, as the sampler launches it"
        s0, p0, _ = _fused(head, x, None, t, tabs, clip)
        r, rm1, k1, k2, _, M = tabs
        ds, dp = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        nat.conv_out_update_x0(head[0], head[1], head[2], None, x, None, None, t, r, rm1, k1, k2, None, nat.RULE_DDIM, M, clip, ds,
                               None, dp)
        assert torch.equal(s0, ds) and torch.equal(p0, dp), "no history: the fused launch's deterministic DDIM cell"


# ------------------------------------------------------------------------------------------------ chains at cfg B
def _eager(diff, model, x0, mk, shape, rule):
    """The eager per-step chain -> [(x, sample, pred_xstart, previous pred_xstart)]"""
    x, prev, steps = x0.clone(), None, []
    with torch.no_grad():
        for i in range(diff.num_timesteps - 1, -1, -1):
            t = torch.full((shape[0],), i, device="cuda", dtype=torch.long)
            if rule == "dpm":
                out = diff.dpm_solver_sample(model, x, t, clip_denoised=True, model_kwargs=mk, prev_pred_xstart=prev)
            else:
                out = diff.ddim_sample(model, x, t, clip_denoised=True, model_kwargs=mk, eta=0.0)
            steps.append((x, out["sample"], out["pred_xstart"], prev))
            x, prev = out["sample"], out["pred_xstart"]
    return steps


@pytest.mark.parametrize("px", [False, True], ids=["eps", "x0"])
def test_replayed_and_eager_ddim10_chains(px, monkeypatch):
    """dpm_solver_sample_loop_progressive (captured graph) against the eager dpm_solver_sample chain: at most ATOL (j + 1) at
    step j, the rule of test_ddim_gpu._bounds (x0-hat of an epsilon model carries sqrt_recip_alphas_cumprod[t] on top, as
    there), the DDIM chains' figure printed next to it; every eager step against the float64 recombination of its own x,
    pred_xstart and previous pred_xstart at ATOL; the first step bitwise DDIM's; the last sample is the last x0-hat; the
    final-only loop repeats bitwise, also with one step per graph.

    The first step of the REPLAYED chain of an x0 model is compared with DDIM's to the last bit of the sample instead: there
    both updates ride in the head launch, whose deterministic DDIM x0 cell was compiled to fma(c1, p0, c2 x) where every
    other deterministic cell, and every multistep cell, has fma(c2, x, c1 p0) (csrc/diffusion_ops.hip, multistep_mean) -
    one rounding of a value of magnitude <= 4, i.e. at most 2^-22 = 2.4e-7 apart; x0-hat is bitwise in every case."""
    model, d, mk, shape = cfgB()
    diff = make_diffusion("ddim10", px)
    n = diff.num_timesteps
    co = diff.dpm_solver_coefficients()
    rep = [(o["sample"], o["pred_xstart"]) for o in
           diff.dpm_solver_sample_loop_progressive(model, shape, noise=d["x"].clone(), clip_denoised=True, model_kwargs=mk)]
    rep_ddim = [(o["sample"], o["pred_xstart"]) for o in
                diff.ddim_sample_loop_progressive(model, shape, noise=d["x"].clone(), clip_denoised=True, model_kwargs=mk)]
    eag, eag_ddim = _eager(diff, model, d["x"], mk, shape, "dpm"), _eager(diff, model, d["x"], mk, shape, "ddim")
    assert len(rep) == len(eag) == n == 10
    worst = 0.0
    for j, i in enumerate(range(n - 1, -1, -1)):
        x, sample, pred, prev = eag[j]
        s64 = co["k1"][i] * pred.double() + co["k2"][i] * x.double()
        if prev is not None:
            s64 = s64 + co["k3"][i] * (pred.double() - prev.double())
        e64 = float((sample.double() - s64).abs().max())
        amp = 1.0 if px else float(diff.sqrt_recip_alphas_cumprod[i])
        ds, dp = float((rep[j][0] - sample).abs().max()), float((rep[j][1] - pred).abs().max())
        dds = float((rep_ddim[j][0] - eag_ddim[j][1]).abs().max())
        print(f"[dpmpp2m ddim10 {'x0' if px else 'eps'}] step {j} (t={i}): eager vs float64 recombination {e64:.2e}; replayed vs "
              f"eager sample {ds:.2e} (DDIM {dds:.2e}) pred_xstart {dp:.2e} / amp {amp:.1f} (bound {ATOL * (j + 1):.1e})")
        worst = max(worst, e64 / ATOL, ds / (ATOL * (j + 1)), dp / (ATOL * (j + 1) * amp))
        assert e64 <= ATOL, (j, e64)
        assert ds <= ATOL * (j + 1), (j, ds)
        assert dp <= ATOL * (j + 1) * amp, (j, dp)
    print(f"[dpmpp2m ddim10 {'x0' if px else 'eps'}] worst share of a bound {worst:.3f}")
    assert torch.equal(rep[0][1], rep_ddim[0][1]), "no history at t = n - 1"
    d0 = float((rep[0][0] - rep_ddim[0][0]).abs().max())
    print(f"[dpmpp2m ddim10 {'x0' if px else 'eps'}] replayed first step vs DDIM's: {d0:.2e}")
    if px:
        assert float(rep_ddim[0][0].abs().max()) <= 4.0 and d0 <= 2.0 ** -22
    else:
        assert d0 == 0.0 and torch.equal(rep[0][0], rep_ddim[0][0])
    assert torch.equal(eag[0][1], eag_ddim[0][1]) and torch.equal(eag[0][2], eag_ddim[0][2])
    assert torch.equal(rep[-1][0], rep[-1][1]) and torch.equal(eag[-1][1], eag[-1][2]), "t = 0: k1 = 1, k2 = k3 = 0"
    assert not torch.equal(rep[-1][0], rep_ddim[-1][0]) and torch.isfinite(rep[-1][0]).all()
    assert float((rep[-1][0] - rep_ddim[-1][0]).abs().max()) > 10 * ATOL, "the second-order term moves the result"
    loop = lambda df: df.dpm_solver_sample_loop(model, shape, noise=d["x"].clone(), clip_denoised=True, model_kwargs=mk,      # noqa: E731
                                                return_decoded=False)
    a, b = loop(diff), loop(diff)
    assert torch.equal(a, b) and torch.equal(a, rep[-1][0]), "run() with K steps per launch == 10 single replays, repeatably"
    assert sorted(k[3] for k in diff._samplers) == [("ddim", 0.0), ("dpmpp2m",)]
    monkeypatch.setenv("LFVDM_STEPS_PER_GRAPH", "1")
    single = make_diffusion("ddim10", px)
    c = loop(single)
    (s,) = single._samplers.values()
    assert s.K == 1 and s.multistep and torch.equal(a, c)


@pytest.mark.parametrize("fused", ["1", "0"])
def test_launches_per_step_equal_ddim(fused, monkeypatch):
    """The step stays clock + forward + at most one update launch: head_fused, extra_launches and the plan's launch count
    are those of the ("ddim", 0.0) sampler, with the update in the head launch and (LFVDM_FUSED_HEAD=0) as its own."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    monkeypatch.setenv("LFVDM_FUSED_HEAD", fused)
    model, d, mk, shape = cfgB()
    got = {}
    for px in (False, True):
        for rule in (("ddim", 0.0), ("dpmpp2m",)):
            s = GraphSampler(make_diffusion("ddim10", px), model, shape, True, rule=rule)
            s.begin(d["x"].clone(), mk)
            got[(px, rule)] = (s.plan.head_fused, s.extra_launches, len(s.plan.steps))
        print(f"[launches fused={fused} x0={px}] ddim {got[(px, ('ddim', 0.0))]}  dpmpp2m {got[(px, ('dpmpp2m',))]}")
        assert got[(px, ("dpmpp2m",))] == got[(px, ("ddim", 0.0))]
        assert got[(px, ("dpmpp2m",))][0] == (fused == "1")


def test_out_of_order_step_is_refused():
    from improved_diffusion.gaussian_diffusion import GraphSampler
    model, d, mk, shape = cfgB()
    diff = make_diffusion("ddim10")
    s = GraphSampler(diff, model, shape, True, rule=("dpmpp2m",))
    s.begin(d["x"].clone(), mk)
    assert float(s.pred.abs().max()) == 0.0, "begin() zeroes the history"
    first = s.step(9)["sample"].clone()
    s.step(8)
    with pytest.raises(ValueError, match="consecutive timesteps"):
        s.step(5)
    with pytest.raises(ValueError, match="consecutive timesteps"):
        s.run(3, 2)
    s.begin(d["x"].clone(), mk)
    assert torch.equal(s.step(9)["sample"], first), "n - 1 starts a chain over"


# ------------------------------------------------------------------------------------------------ long video, host route
def test_sample_video_with_the_multistep_sampler():
    from improved_diffusion.video_sampler import default_sampling_args, sample_video
    model, _, _, _ = cfgB()
    diff = make_diffusion("ddim25")
    Tv, n_obs = 30, 4
    batch = torch.from_numpy((0.8 * recipe.gaussianish("ddim/video", 2 * Tv * 4 * 16 * 16)).reshape(2, Tv, 4, 16, 16)
                             .astype(np.float32)).cuda()
    kw = dict(sampling_scheme="autoreg", n_obs=n_obs, max_frames=10, max_latent_frames=5, device="cuda")
    res = []
    for a in (dict(use_dpm_solver=True), dict(use_dpm_solver=True), dict(use_ddim=True)):
        torch.manual_seed(21)
        res.append(sample_video(default_sampling_args(**kw, **a), model, diff, batch, verbose=False)[0])
    assert torch.equal(res[0][:, :n_obs], batch[:, :n_obs]), "the observed frames are untouched"
    assert torch.isfinite(res[0]).all() and not torch.equal(res[0][:, n_obs:], batch[:, n_obs:])
    assert torch.equal(res[0], res[1]), "seed-reproducible"
    assert not torch.equal(res[0], res[2]), "not the DDIM result"
    assert {k[3] for k in diff._samplers} == {("dpmpp2m",), ("ddim", 0.0)}
    from types import SimpleNamespace
    both = SimpleNamespace(**{**vars(default_sampling_args(**kw)), "use_ddim": True, "use_dpm_solver": True})
    with pytest.raises(ValueError, match="use_ddim and use_dpm_solver"):
        sample_video(both, model, diff, batch, verbose=False)


@pytest.mark.parametrize("px", [False, True], ids=["eps", "x0"])
def test_denoised_fn_route(px):
    """denoised_fn = identity goes through the elementwise host route: within ATOL of the fused kernel, with and without a
    history."""
    diff = make_diffusion("ddim50", px)
    tv = _rows(diff)
    x, out, hist = (torch.from_numpy(a).cuda() for a in _op_inputs(DENSE))
    t = torch.from_numpy(tv).cuda()
    net = lambda x_, timesteps=None, **kw: (out, None)      # noqa: E731
    for h in (hist, None):
        a = diff.dpm_solver_sample(net, x, t, model_kwargs={}, prev_pred_xstart=h)
        b = diff.dpm_solver_sample(net, x, t, model_kwargs={}, prev_pred_xstart=h, denoised_fn=lambda v: v)
        assert set(a) == set(b) == {"sample", "pred_xstart"}
        es = float((a["sample"] - b["sample"]).abs().max())
        ep = float((a["pred_xstart"] - b["pred_xstart"]).abs().max())
        print(f"[ms denoised_fn {'x0' if px else 'eps'} hist={h is not None}] sample {es:.2e} pred_xstart {ep:.2e} "
              f"(worst {max(es, ep) / ATOL:.3f} of bound)")
        assert max(es, ep) <= ATOL
