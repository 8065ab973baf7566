"""x0-prediction models (predict_xstart=True, ModelMeanType.START_X) on the MI355X against the reference built with that
flag (tests/golden/xstart_*.npz, written by tools/make_xstart_golden.py from the reference's own methods in float64): the
MEAN_X0 instantiations of the three update kernels through the C ABI, replayed and eager chains, p_mean_variance, the
denoised_fn route, training_losses and the captured micro-step, sample_video.  Every comparison prints error / bound."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import recipe
from conftest import GOLDEN
from test_oracle_golden import compare_to_fixture, load_case
from test_forward_gpu import build_native

pytestmark = pytest.mark.gpu

PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
ETAS = (0.0, 0.5, 1.0)
ATOL = 2e-4     # what tests/test_ddim_gpu.py and tests/test_sampler_gpu.py grant an update against a float64 fixture


def make_diffusion(resp="", predict_xstart=True):
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


def _fix(g, prefix, j):
    gj = {k: g[f"{prefix}/{k}"][j] for k in ("sub", "frame_sum", "frame_norm")}
    gj["stride"] = g[f"{prefix}/stride"]
    return gj


def _bound(g, leg, key, j):
    """max(2e-4 per step taken, three times the fp32 reference's own deviation from the float64 trajectory): the rule of
    tests/test_ddim_gpu.py::_bounds; x0-hat carries no sqrt_recip_alphas_cumprod factor in this mode."""
    return max(ATOL * (j + 1), 3.0 * float(g[f"{leg}/ref32_dev/{key}"][j]))


# ------------------------------------------------------------------------------------------------ the update kernels
def _one_hot_head(out, C=64):
    """Channels-last rows and packed filters [Cout][9][C] whose 3x3 convolution IS ``out`` (centre tap, channel co -> co)."""
    B, T, Co, H, W = out.shape
    act = torch.zeros(B * T * H * W, C, device="cuda")
    act[:, :Co] = out.permute(0, 1, 3, 4, 2).reshape(-1, Co)
    wp = torch.zeros(Co, 9, C, device="cuda")
    for co in range(Co):
        wp[co, 4, co] = 1.0
    return act, wp, torch.zeros(Co, device="cuda")


def _tables(diff, mode):
    """-> c1, c2, sg, rule of the update ``mode``: "p" | eta | "reverse"."""
    from improved_diffusion import _native as nat
    if mode == "p":
        tb = diff.tables("cuda")
        return tb["posterior_mean_coef1"], tb["posterior_mean_coef2"], tb["model_log_variance"], nat.RULE_ANCESTRAL
    co = diff.ddim_tables("cuda", 0.0 if mode == "reverse" else mode, mode == "reverse")
    return co["k1"], co["k2"], co["sigma"], nat.RULE_DDIM


def _run_x0(kind, x, out, z, t, tabs, clip, seed=None, inplace=False, head=None):
    """One MEAN_X0 update through the C ABI with NULL sqrt_recip / sqrt_recipm1.  kind: given | rng | fused.
    -> sample, pred, mean (ancestral only), noise used, the convolution's output"""
    from improved_diffusion import _native as nat
    c1, c2, sg, rule = tabs
    det = sg is None
    xin = x.clone()
    sample = xin if inplace else torch.full_like(x, float("nan"))
    pred = torch.full_like(x, float("nan"))
    mean = torch.full_like(x, float("nan")) if rule == nat.RULE_ANCESTRAL else None
    zo = torch.full_like(x, float("nan"))
    if kind == "given":
        nat.update_x0(xin, out, None if det else z, t, None, None, c1, c2, sg, rule, nat.MEAN_X0, clip, sample, pred, mean)
        return sample, pred, mean, z, None
    if kind == "rng":
        nat.update_rng_x0(xin, out, None if det else zo, t, None, None, c1, c2, sg, rule, nat.MEAN_X0, clip, sample,
                          None if det else seed, pred, mean)
        return sample, pred, mean, zo, None
    act, wp, bias = head if head is not None else _one_hot_head(out)
    assert nat.lib().lfvdm_conv_out_psample_ok(x.shape[0] * x.shape[1], x.shape[3], x.shape[4], act.shape[1], x.shape[2]) == 0
    conv = torch.full_like(x, float("nan"))
    given = seed is None and not det
    nat.conv_out_update_x0(act, wp, bias, conv, xin, z if given else None, None if given or det else zo, t, None, None, c1, c2,
                           sg, rule, nat.MEAN_X0, clip, sample, None if det else seed, pred, mean)
    return sample, pred, mean, (z if given else zo), conv


MODES = ("p",) + ETAS + ("reverse",)


@pytest.mark.parametrize("tag,resp", [("d1000", ""), ("ddim50", "ddim50")])
def test_update_kernels_match_the_reference(tag, resp):
    """p_sample / p_mean_variance, ddim_sample at eta 0 / 0.5 / 1 and ddim_reverse_sample of the reference built with
    predict_xstart=True; clamp on and off; t = 0, 1, middle, last: every new entry with given noise, kernel noise, and the
    deterministic instantiation (NULL noise and seed), out of place and in place, all with NULL sqrt_recip pointers.
    atol 2e-4 on sample, mean and x0-hat.  Kernels that draw their own noise are compared after replacing the fixture's z
    by theirs with the reference's float64 sigma (sample + sigma (z_kernel - z_fixture))."""
    g = np.load(os.path.join(GOLDEN, "xstart_update.npz"))
    diff = make_diffusion(resp)
    seed = torch.tensor([20240607], dtype=torch.int64, device="cuda")
    worst = {}
    for case in (f"{tag}/t0", f"{tag}/t1"):
        assert 0.02 < float(g[f"{case}/clamp_share"]) < 0.6, "the clamp bites in a real share of the elements, not in all"
        tv = g[f"{case}/t"]
        x, out, z = (torch.from_numpy(g[f"{case}/{k}"]).cuda() for k in ("x", "out", "z"))
        t = torch.from_numpy(tv).cuda()
        B = x.shape[0]
        nz = torch.from_numpy((tv != 0).astype(np.float64)).view(B, 1, 1, 1, 1)
        for clip in (0, 1):
            want_pred = torch.from_numpy(g[f"{case}/clip{clip}/pred_xstart"])
            for mode in MODES:
                tabs = _tables(diff, mode)
                det = tabs[2] is None
                assert det == (mode in (0.0, "reverse"))
                name = mode if isinstance(mode, str) else f"eta{mode}"
                want = torch.from_numpy(g[f"{case}/clip{clip}/{name}/sample"])
                want_mean = torch.from_numpy(g[f"{case}/clip{clip}/p/mean"]) if mode == "p" else None
                sig = None if det else torch.from_numpy(g[f"{tag}/{name}/sigma"][tv]).view(B, 1, 1, 1, 1)
                for kind, sd in (("given", None), ("rng", seed), ("fused", None), ("fused", seed)):
                    if det and kind == "fused" and sd is not None:
                        continue        # deterministic: there is no seed to hand over
                    for inplace in (False, True):
                        sample, pred, mean, zk, conv = _run_x0(kind, x, out, z, t, tabs, clip, sd, inplace)
                        torch.cuda.synchronize()
                        exp = want if det else want + nz * sig * (zk.double().cpu() - z.double().cpu())
                        if conv is not None:
                            assert torch.equal(conv, out), "the convolution's own output is the fixture's model output"
                        es = float((sample.double().cpu() - exp).abs().max())
                        ep = float((pred.double().cpu() - want_pred).abs().max())
                        em = float((mean.double().cpu() - want_mean).abs().max()) if want_mean is not None else 0.0
                        key = (kind, "seed" if sd is not None else "z", name, "inplace" if inplace else "out")
                        worst[key] = tuple(max(a, b) for a, b in zip(worst.get(key, (0.0, 0.0, 0.0)), (es, ep, em)))
                        assert es <= ATOL and ep <= ATOL and em <= ATOL, (case, clip, key, es, ep, em)
    for key, (es, ep, em) in sorted(worst.items(), key=str):
        print(f"[{tag}] {key}: sample {es:.2e} ({es / ATOL:.3f} of bound)  pred_xstart {ep:.2e} ({ep / ATOL:.3f})  "
              f"mean {em:.2e} ({em / ATOL:.3f})")


@pytest.mark.parametrize("mode", MODES)
def test_fused_head_on_a_dense_activation(mode):
    """lfvdm_conv_out_update_x0 on a dense synthetic activation (C = 64, all nine taps, a bias): its convolution output
    against a float64 convolution, and sample / x0-hat / mean against the float64 update OF that convolution (the folded
    form, which tools/make_xstart_golden.py pins to the reference's rule at 1e-12).  atol 2e-4."""
    g = np.load(os.path.join(GOLDEN, "xstart_update.npz"))
    diff = make_diffusion("ddim50")
    case = "ddim50/t1"
    tv = g[f"{case}/t"]
    x, z = (torch.from_numpy(g[f"{case}/{k}"]).cuda() for k in ("x", "z"))
    t = torch.from_numpy(tv).cuda()
    B, T, Co, H, W = x.shape
    C = 64
    act = torch.from_numpy(recipe.gaussianish("xstart/head/act", B * T * H * W * C).reshape(B * T * H * W, C).astype(np.float32))
    wp = torch.from_numpy((recipe.gaussianish("xstart/head/w", Co * 9 * C) / 24.0).reshape(Co, 9, C).astype(np.float32))
    bias = torch.from_numpy((0.1 * recipe.gaussianish("xstart/head/b", Co)).astype(np.float32))
    w64 = wp.double().view(Co, 3, 3, C).permute(0, 3, 1, 2)
    a64 = act.double().view(B * T, H, W, C).permute(0, 3, 1, 2)
    e64 = torch.nn.functional.conv2d(a64, w64, bias.double(), padding=1).view(B, T, Co, H, W)
    share = float((e64.abs() > 1).double().mean())
    assert 0.02 < share < 0.6, share
    tabs = _tables(diff, mode)
    det = tabs[2] is None
    if mode == "p":
        c1, c2 = diff.posterior_mean_coef1, diff.posterior_mean_coef2
        sg = np.exp(0.5 * diff._fixed_var_tables()[1])
    else:
        co = diff.ddim_coefficients(0.0 if mode == "reverse" else mode, mode == "reverse")
        c1, c2, sg = co["k1"], co["k2"], co["sigma"]
    v = lambda a: torch.from_numpy(a[tv]).view(B, 1, 1, 1, 1)      # noqa: E731
    nz = torch.from_numpy((tv != 0).astype(np.float64)).view(B, 1, 1, 1, 1)
    seed = torch.tensor([77], dtype=torch.int64, device="cuda")
    for clip in (0, 1):
        p64 = e64.clamp(-1, 1) if clip else e64
        m64 = v(c1) * p64 + v(c2) * x.double().cpu()
        for sd in ((None,) if det else (None, seed)):
            sample, pred, mean, zk, conv = _run_x0("fused", x, None, z, t, tabs, clip, sd, False,
                                                   head=(act.cuda(), wp.cuda(), bias.cuda()))
            torch.cuda.synchronize()
            exp = m64 if det else m64 + nz * v(sg) * zk.double().cpu()
            ec = float((conv.double().cpu() - e64).abs().max())
            es = float((sample.double().cpu() - exp).abs().max())
            ep = float((pred.double().cpu() - p64).abs().max())
            em = float((mean.double().cpu() - m64).abs().max()) if mean is not None else 0.0
            print(f"[dense head {mode} clip={clip} {'seed' if sd is not None else 'given'}] clamp share {share:.2f}; conv {ec:.2e} "
                  f"sample {es:.2e} pred_xstart {ep:.2e} mean {em:.2e} (worst {max(ec, es, ep, em) / ATOL:.3f} of bound)")
            assert max(ec, es, ep, em) <= ATOL


def test_unknown_rule_or_mean_type_is_refused():
    from improved_diffusion import _native as nat
    diff = make_diffusion("ddim50")
    x = torch.zeros(2, 1, 4, 4, 4, device="cuda")
    t = torch.zeros(2, dtype=torch.int64, device="cuda")
    c1, c2, sg, rule = _tables(diff, "p")
    for bad in (dict(rule=7), dict(mean_type=5), dict(rule=-1)):
        kw = dict(rule=rule, mean_type=nat.MEAN_X0)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="invalid shape"):
            nat.update_x0(x, x, x, t, None, None, c1, c2, sg, kw["rule"], kw["mean_type"], True, torch.empty_like(x))
    with pytest.raises(RuntimeError, match="invalid shape"):        # epsilon needs its two tables
        nat.update_x0(x, x, x, t, None, None, c1, c2, sg, rule, nat.MEAN_EPS, True, torch.empty_like(x))
    with pytest.raises(RuntimeError, match="invalid shape"):        # the ancestral rule needs its log-variance table
        nat.update_x0(x, x, x, t, None, None, c1, c2, None, rule, nat.MEAN_X0, True, torch.empty_like(x))


def test_noise_stream_is_the_epsilon_mode_stream():
    """Equal (seed, t, shape): noise_out of the x0 entries is bitwise what the MEAN_EPS ancestral lfvdm_update_rng_x0 writes;
    and in every rule x mean type cell the given-noise entry, fed the noise the RNG entry reported, reproduces that entry's
    sample and x0-hat bitwise (t holds 0 - where the noise is not applied - and nonzero steps)."""
    from improved_diffusion import _native as nat
    g = np.load(os.path.join(GOLDEN, "xstart_update.npz"))
    diff = make_diffusion("ddim50")
    case = "ddim50/t0"
    x, out = (torch.from_numpy(g[f"{case}/{k}"]).cuda() for k in ("x", "out"))
    tv = g[f"{case}/t"]
    assert (tv == 0).any() and (tv != 0).any()
    t = torch.from_numpy(tv).cuda()
    tb = diff.tables("cuda")
    r, rm1 = tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"]
    for seed_value in (5, -77):
        seed = torch.tensor([seed_value], dtype=torch.int64, device="cuda")
        z_eps, s_eps, p_eps = torch.zeros_like(x), torch.empty_like(x), torch.empty_like(x)
        nat.update_rng_x0(x, out, z_eps, t, r, rm1, tb["posterior_mean_coef1"], tb["posterior_mean_coef2"],
                          tb["model_log_variance"], nat.RULE_ANCESTRAL, nat.MEAN_EPS, True, s_eps, seed, p_eps)
        assert float(z_eps.std()) > 0.5
        for mode in ("p", 0.5, 1.0):
            tabs = _tables(diff, mode)
            _, _, _, z_rng, _ = _run_x0("rng", x, out, None, t, tabs, True, seed)
            _, _, _, z_fused, _ = _run_x0("fused", x, out, None, t, tabs, True, seed)
            torch.cuda.synchronize()
            assert torch.equal(z_rng, z_eps) and torch.equal(z_fused, z_eps), mode
        for mode in ("p", 1.0):
            c1, c2, sg, rule = _tables(diff, mode)
            for mean_type, rr, rr1 in ((nat.MEAN_EPS, r, rm1), (nat.MEAN_X0, None, None)):
                z1, s1, p1, s2, p2 = (torch.full_like(x, float("nan")) for _ in range(5))
                nat.update_rng_x0(x, out, z1, t, rr, rr1, c1, c2, sg, rule, mean_type, True, s1, seed, p1)
                nat.update_x0(x, out, z1, t, rr, rr1, c1, c2, sg, rule, mean_type, True, s2, p2)
                torch.cuda.synchronize()
                assert torch.isfinite(s1).all() and torch.isfinite(p1).all(), (mode, mean_type)
                assert torch.equal(z1, z_eps) and torch.equal(s2, s1) and torch.equal(p2, p1), (mode, mean_type)


# ------------------------------------------------------------------------------------------------ trajectories
CONFIGS = {"default": {}, "two_launch_head": {"LFVDM_FUSED_HEAD": "0"}, "no_level_chains": {"LFVDM_LEVEL_CHAIN": "0"},
           "one_step_per_graph": {"LFVDM_STEPS_PER_GRAPH": "1"}}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_replayed_and_eager_ancestral_steps_follow_the_reference(config, monkeypatch):
    """Three p_sample steps from t = 999 at cfg B with the fixture's noise: the replayed step (GraphSampler, inject_noise)
    and the eager p_sample against the reference, and against each other within the same bound."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    for k, v in CONFIGS[config].items():
        monkeypatch.setenv(k, v)
    g = np.load(os.path.join(GOLDEN, "xstart_traj_cfgB.npz"))
    model, d, mk, shape = cfgB()
    diff = make_diffusion("")
    s = GraphSampler(diff, model, shape, True, inject_noise=True)
    s.begin(d["x"].clone(), mk)
    assert s.x0_mode and s.plan.head_fused == (config != "two_launch_head")
    assert bool(s.plan.chains) == (config != "no_level_chains")
    x = d["x"].clone()
    for j, i in enumerate((999, 998, 997)):
        noise = torch.from_numpy(recipe.gaussianish(f"xstartB/p/noise{j}", d["x"].numel()).reshape(shape).astype(np.float32)).cuda()
        s.noise.copy_(noise)
        out = s.step(i)
        bs, bp = _bound(g, "p", "sample", j), _bound(g, "p", "pred_xstart", j)
        es = compare_to_fixture(out["sample"], _fix(g, "p/sample", j), atol=bs, rtol=0.0)
        ep = compare_to_fixture(out["pred_xstart"], _fix(g, "p/pred_xstart", j), atol=bp, rtol=0.0)
        with torch.no_grad():
            t = torch.full((shape[0],), i, device="cuda", dtype=torch.long)
            eo = diff.p_sample(model, x, t, clip_denoised=True, model_kwargs=mk, noise=noise)
        x = eo["sample"]
        ee = compare_to_fixture(x, _fix(g, "p/sample", j), atol=bs, rtol=0.0)
        eq = compare_to_fixture(eo["pred_xstart"], _fix(g, "p/pred_xstart", j), atol=bp, rtol=0.0)
        dr, dq = float((x - out["sample"]).abs().max()), float((eo["pred_xstart"] - out["pred_xstart"]).abs().max())
        print(f"[p {config}] step {j} (t={i}): replayed sample {es:.2e} ({es / bs:.3f} of bound) pred_xstart {ep:.2e} ({ep / bp:.3f}); "
              f"eager sample {ee:.2e} ({ee / bs:.3f}) pred_xstart {eq:.2e} ({eq / bp:.3f}); replayed vs eager {dr:.2e} ({dr / bs:.3f}) "
              f"{dq:.2e} ({dq / bp:.3f})")
        assert dr <= bs and dq <= bp, (j, dr, dq)
        assert float(out["pred_xstart"].abs().max()) <= 1.0


@pytest.mark.parametrize("config", list(CONFIGS))
def test_replayed_ddim10_chain_follows_the_reference(config, monkeypatch):
    """ddim_sample_loop_progressive (captured graph) at cfg B on ddim10, eta = 0: all 10 steps against the reference; the
    eager per-step chain within the same bound of the replayed one; ddim_sample_loop (K steps per launch) returns the last
    state, twice bitwise the same."""
    for k, v in CONFIGS[config].items():
        monkeypatch.setenv(k, v)
    g = np.load(os.path.join(GOLDEN, "xstart_traj_cfgB.npz"))
    model, d, mk, shape = cfgB()
    diff = make_diffusion("ddim10")
    assert np.array_equal(np.array(diff.timestep_map), g["timestep_map"])
    x = d["x"].clone()
    last = None
    for j, out in enumerate(diff.ddim_sample_loop_progressive(model, shape, noise=d["x"].clone(), clip_denoised=True,
                                                              model_kwargs=mk, eta=0.0)):
        i = 9 - j
        bs, bp = _bound(g, "eta0", "sample", j), _bound(g, "eta0", "pred_xstart", j)
        es = compare_to_fixture(out["sample"], _fix(g, "eta0/sample", j), atol=bs, rtol=0.0)
        ep = compare_to_fixture(out["pred_xstart"], _fix(g, "eta0/pred_xstart", j), atol=bp, rtol=0.0)
        with torch.no_grad():
            t = torch.full((shape[0],), i, device="cuda", dtype=torch.long)
            eo = diff.ddim_sample(model, x, t, clip_denoised=True, model_kwargs=mk, eta=0.0)
        x = eo["sample"]
        ee = compare_to_fixture(x, _fix(g, "eta0/sample", j), atol=bs, rtol=0.0)
        dr, dq = float((x - out["sample"]).abs().max()), float((eo["pred_xstart"] - out["pred_xstart"]).abs().max())
        print(f"[ddim10 {config}] step {j} (t={i}): replayed sample {es:.2e} ({es / bs:.3f} of bound) pred_xstart {ep:.2e} "
              f"({ep / bp:.3f}); eager sample {ee:.2e} ({ee / bs:.3f}); replayed vs eager {dr:.2e} ({dr / bs:.3f}) {dq:.2e} ({dq / bp:.3f})")
        assert dr <= bs and dq <= bp, (j, dr, dq)
        last = out["sample"]
    assert j == 9 and torch.equal(last, out["pred_xstart"]), "t = 0 of the chain: k1 = 1, k2 = 0"
    (key, s), = diff._samplers.items()
    assert key[3] == ("ddim", 0.0) and s.x0_mode and s.plan.head_fused == (config != "two_launch_head")
    assert s.K == (1 if config == "one_step_per_graph" else 8)
    finals = [diff.ddim_sample_loop(model, shape, noise=d["x"].clone(), clip_denoised=True, model_kwargs=mk, eta=0.0,
                                    return_decoded=False) for _ in range(2)]
    assert torch.equal(finals[0], finals[1]) and torch.equal(finals[0], last), "the replayed chain is bitwise repeatable"


@pytest.mark.parametrize("fused", ["1", "0"])
def test_replayed_eta1_chain_with_injected_noise(fused, monkeypatch):
    """eta = 1 with the fixture's per-step noise, four steps from the top of ddim10, replayed and eager; with kernel noise a
    seeded chain repeats bitwise and another seed gives another video."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    monkeypatch.setenv("LFVDM_FUSED_HEAD", fused)
    g = np.load(os.path.join(GOLDEN, "xstart_traj_cfgB.npz"))
    model, d, mk, shape = cfgB()
    diff = make_diffusion("ddim10")
    s = GraphSampler(diff, model, shape, True, inject_noise=True, rule=("ddim", 1.0))
    s.begin(d["x"].clone(), mk)
    assert s.plan.head_fused == (fused == "1")
    x = d["x"].clone()
    for j, i in enumerate(range(9, 5, -1)):
        noise = torch.from_numpy(recipe.gaussianish(f"xstartB/eta1/noise{j}", d["x"].numel()).reshape(shape).astype(np.float32)).cuda()
        s.noise.copy_(noise)
        out = s.step(i)
        bs, bp = _bound(g, "eta1", "sample", j), _bound(g, "eta1", "pred_xstart", j)
        es = compare_to_fixture(out["sample"], _fix(g, "eta1/sample", j), atol=bs, rtol=0.0)
        ep = compare_to_fixture(out["pred_xstart"], _fix(g, "eta1/pred_xstart", j), atol=bp, rtol=0.0)
        with torch.no_grad():
            t = torch.full((shape[0],), i, device="cuda", dtype=torch.long)
            x = diff.ddim_sample(model, x, t, clip_denoised=True, model_kwargs=mk, eta=1.0, noise=noise)["sample"]
        ee = compare_to_fixture(x, _fix(g, "eta1/sample", j), atol=bs, rtol=0.0)
        dr = float((x - out["sample"]).abs().max())
        print(f"[ddim10 eta=1 fused={fused}] step {j} (t={i}): replayed sample {es:.2e} ({es / bs:.3f} of bound) pred_xstart "
              f"{ep:.2e} ({ep / bp:.3f}); eager sample {ee:.2e} ({ee / bs:.3f}); replayed vs eager {dr:.2e} ({dr / bs:.3f})")
        assert dr <= bs
    res = []
    for sd in (3, 3, 4):
        torch.manual_seed(sd)
        res.append(diff.ddim_sample_loop(model, shape, noise=d["x"].clone(), model_kwargs=mk, eta=1.0, return_decoded=False))
    assert torch.equal(res[0], res[1]) and not torch.equal(res[0], res[2]) and torch.isfinite(res[0]).all()


@pytest.mark.parametrize("fused", ["1", "0"])
def test_cfgD_window_follows_the_reference(fused, monkeypatch):
    """The K = 14 window of the long-video configuration (batch 1, 250-step respacing): the first three and the last two
    p_sample steps with recorded noise, replayed, against the reference."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    monkeypatch.setenv("LFVDM_FUSED_HEAD", fused)
    g = np.load(os.path.join(GOLDEN, "xstart_window_cfgD.npz"))
    model, _, _, _ = cfgB()
    K = 14
    inp = {k: torch.from_numpy(v) for k, v in recipe.make_inputs(f"cfgD_w{K}", 1, K, 4, 16, 16).items()}
    n_obs = int(g["n_obs"])
    obs = torch.zeros(1, K, 1, 1, 1)
    obs[:, :n_obs] = 1.0
    mk = dict(frame_indices=torch.from_numpy(g["frame_indices"]).cuda(), obs_mask=obs.cuda(), latent_mask=(1 - obs).cuda(),
              x0=inp["x0"].cuda())
    shape = tuple(inp["x"].shape)
    diff = make_diffusion("250")
    s = GraphSampler(diff, model, shape, True, inject_noise=True)
    for leg, steps, x in (("top", (249, 248, 247), inp["x"].clone()), ("bottom", (1, 0), 0.5 * inp["x"] + 0.5 * inp["x0"])):
        s.begin(x.cuda(), mk)
        assert s.plan.time_steps == 250 and s.plan.head_fused == (fused == "1")
        for j, i in enumerate(steps):
            noise = torch.from_numpy(recipe.gaussianish(f"xstartD/{leg}/noise{j}", inp["x"].numel()).reshape(shape).astype(np.float32))
            s.noise.copy_(noise.cuda())
            out = s.step(i)
            bs, bp = _bound(g, leg, "sample", j), _bound(g, leg, "pred_xstart", j)
            es = compare_to_fixture(out["sample"], _fix(g, f"{leg}/sample", j), atol=bs, rtol=0.0)
            ep = compare_to_fixture(out["pred_xstart"], _fix(g, f"{leg}/pred_xstart", j), atol=bp, rtol=0.0)
            print(f"[cfgD window K=14 fused={fused}] {leg} step {j} (i={i}): sample {es:.2e} ({es / bs:.3f} of bound) pred_xstart "
                  f"{ep:.2e} ({ep / bp:.3f})")


def test_launch_count_equals_the_epsilon_sampler():
    from improved_diffusion.gaussian_diffusion import GraphSampler
    model, d, mk, shape = cfgB()
    counts = {}
    for px in (False, True):
        for rule in (("ancestral",), ("ddim", 0.0), ("ddim", 1.0)):
            s = GraphSampler(make_diffusion("ddim10", predict_xstart=px), model, shape, True, rule=rule)
            s.begin(d["x"].clone(), mk)
            counts[(px, rule)] = (len(s.plan.steps), s.extra_launches)
    for rule in (("ancestral",), ("ddim", 0.0), ("ddim", 1.0)):
        print(f"[launches {rule}] epsilon {counts[(False, rule)]}  x0 {counts[(True, rule)]}  (plan launches, extra launches)")
        assert counts[(True, rule)] == counts[(False, rule)]


def test_epsilon_chain_is_untouched_by_an_x0_chain_in_between():
    """Two diffusion objects on one model and shape: the epsilon chain after an x0 chain is bitwise the epsilon chain
    before it, for the ancestral and the DDIM rule."""
    model, d, mk, shape = cfgB()
    eps, x0d = make_diffusion("ddim10", predict_xstart=False), make_diffusion("ddim10")

    def chains(diff):
        torch.manual_seed(11)
        a = diff.p_sample_loop(model, shape, noise=d["x"].clone(), clip_denoised=True, model_kwargs=mk, return_decoded=False)[0]
        b = diff.ddim_sample_loop(model, shape, noise=d["x"].clone(), clip_denoised=True, model_kwargs=mk, eta=0.5,
                                  return_decoded=False)
        return a, b
    a0, b0 = chains(eps)
    xa, xb = chains(x0d)
    a1, b1 = chains(eps)
    fa, fb = chains(make_diffusion("ddim10", predict_xstart=False))
    assert torch.equal(a0, a1) and torch.equal(b0, b1) and torch.equal(a0, fa) and torch.equal(b0, fb)
    assert not torch.equal(xa, a0) and not torch.equal(xb, b0) and torch.isfinite(xa).all() and torch.isfinite(xb).all()
    assert len(eps._samplers) == 2 and len(x0d._samplers) == 2
    assert all(s.x0_mode for s in x0d._samplers.values()) and not any(s.x0_mode for s in eps._samplers.values())


# ------------------------------------------------------------------------------------------------ host routes
def test_denoised_fn_route():
    """denoised_fn = clamp to 0.5: x0-hat is at most 0.5 and equals clamp(denoised_fn(model output)) element by element;
    the sample is the posterior mean / folded DDIM rule of that x0-hat."""
    g = np.load(os.path.join(GOLDEN, "xstart_update.npz"))
    diff = make_diffusion("ddim50")
    case = "ddim50/t1"
    tv = g[f"{case}/t"]
    x, out, z = (torch.from_numpy(g[f"{case}/{k}"]).cuda() for k in ("x", "out", "z"))
    t = torch.from_numpy(tv).cuda()
    B = x.shape[0]
    net = lambda x_, timesteps=None, **kw: (out, None)      # noqa: E731
    fn = lambda v: v.clamp(max=0.5)      # noqa: E731
    want = out.clamp(max=0.5).clamp(-1, 1)
    v64 = lambda a: torch.from_numpy(a[tv]).view(B, 1, 1, 1, 1)      # noqa: E731
    nz = torch.from_numpy((tv != 0).astype(np.float64)).view(B, 1, 1, 1, 1)
    r = diff.p_sample(net, x, t, denoised_fn=fn, model_kwargs={}, noise=z)
    m = diff.p_mean_variance(net, x, t, denoised_fn=fn, model_kwargs={})
    e = diff.ddim_sample(net, x, t, denoised_fn=fn, model_kwargs={}, eta=1.0, noise=z)
    co = diff.ddim_coefficients(1.0)
    mean64 = v64(diff.posterior_mean_coef1) * want.double().cpu() + v64(diff.posterior_mean_coef2) * x.double().cpu()
    exp_p = mean64 + nz * v64(np.exp(0.5 * diff._fixed_var_tables()[1])) * z.double().cpu()
    exp_d = v64(co["k1"]) * want.double().cpu() + v64(co["k2"]) * x.double().cpu() + nz * v64(co["sigma"]) * z.double().cpu()
    for name, res in (("p_sample", r), ("p_mean_variance", m), ("ddim_sample", e)):
        assert float(res["pred_xstart"].max()) <= 0.5 and torch.equal(res["pred_xstart"], want), name
    errs = dict(p=float((r["sample"].double().cpu() - exp_p).abs().max()), mean=float((m["mean"].double().cpu() - mean64).abs().max()),
                ddim=float((e["sample"].double().cpu() - exp_d).abs().max()))
    print(f"[denoised_fn] {errs} (worst {max(errs.values()) / ATOL:.3f} of bound)")
    assert max(errs.values()) <= ATOL


def test_p_mean_variance():
    """mean and pred_xstart from the one noise-free kernel pass against the reference's p_mean_variance; variance and
    log_variance are the fixed-sigma tables, as in the epsilon mode."""
    g = np.load(os.path.join(GOLDEN, "xstart_update.npz"))
    for tag, resp in (("d1000", ""), ("ddim50", "ddim50")):
        diff, eps = make_diffusion(resp), make_diffusion(resp, predict_xstart=False)
        for ti in (0, 1):
            case = f"{tag}/t{ti}"
            x, out = (torch.from_numpy(g[f"{case}/{k}"]).cuda() for k in ("x", "out"))
            t = torch.from_numpy(g[f"{case}/t"]).cuda()
            net = lambda x_, timesteps=None, **kw: (out, None)      # noqa: E731
            for clip in (0, 1):
                m = diff.p_mean_variance(net, x, t, clip_denoised=bool(clip), model_kwargs={})
                me = eps.p_mean_variance(net, x, t, clip_denoised=bool(clip), model_kwargs={})
                em = float((m["mean"].double().cpu() - torch.from_numpy(g[f"{case}/clip{clip}/p/mean"])).abs().max())
                ep = float((m["pred_xstart"].double().cpu() - torch.from_numpy(g[f"{case}/clip{clip}/pred_xstart"])).abs().max())
                print(f"[p_mean_variance {case} clip={clip}] mean {em:.2e} ({em / ATOL:.3f} of bound) pred_xstart {ep:.2e} ({ep / ATOL:.3f})")
                assert em <= ATOL and ep <= ATOL
                assert m["variance"].shape == x.shape and m["log_variance"].shape == x.shape
                assert torch.equal(m["variance"], me["variance"]) and torch.equal(m["log_variance"], me["log_variance"])
                np.testing.assert_allclose(m["variance"][:, 0, 0, 0, 0].cpu().numpy(), g[f"{case}/clip{clip}/p/variance"], rtol=1e-6)
                np.testing.assert_allclose(m["log_variance"][:, 0, 0, 0, 0].cpu().numpy(), g[f"{case}/clip{clip}/p/log_variance"],
                                           rtol=1e-6)


# ------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("inplace", [False, True], ids=["autograd", "inplace"])
def test_training_losses_match_the_reference(inplace):
    """training_losses -> (loss * weights).mean().backward() at the micro configuration against the reference built with
    predict_xstart=True (the target is x_start), both gradient delivery modes.  Losses rtol 1e-4; gradients at the bounds
    of tests/test_backward_gpu.py for this shape: |d| <= 2e-3 (max|g_ref| of the tensor + 1e-3 max|g_ref| of the model) on
    the stored leading elements, per-tensor norms within 3e-3 (norm + 1e-3 gmax sqrt(n))."""
    g = np.load(os.path.join(GOLDEN, "xstart_train_micro.npz"))
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd).train()
    model.native_grad_accumulation = inplace
    d = {k: v.cuda() for k, v in inp.items()}
    diff = make_diffusion("")
    noise = torch.from_numpy(recipe.gaussianish("xstartTrain/noise", inp["x0"].numel()).reshape(inp["x0"].shape).astype(np.float32)).cuda()
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    terms = diff.training_losses(model, d["x0"], torch.from_numpy(g["t"]).cuda(), model_kwargs=mk, noise=noise,
                                 latent_mask=1 - d["obs_mask"], eval_mask=d["latent_mask"])
    (terms["loss"] * torch.ones(2, device="cuda")).mean().backward()
    torch.cuda.synchronize()
    for k in ("mse", "eval-mse", "loss"):
        rel = float(np.abs(terms[k].detach().cpu().numpy() / g[k] - 1).max())
        print(f"[train micro {'inplace' if inplace else 'autograd'}] {k}: {terms[k].detach().cpu().numpy()} rel {rel:.2e} ({rel / 1e-4:.3f} of bound)")
        np.testing.assert_allclose(terms[k].detach().cpu().numpy(), g[k], rtol=1e-4)
    gmax = float(g["gmax"])
    keys = [str(k) for k in g["keys"]]
    worst, worst_n = (0.0, None), (0.0, None)
    for i, (k, p) in enumerate(model.named_parameters()):
        assert k == keys[i] and p.grad is not None, k
        n = min(16, p.numel())
        err = float(np.abs(p.grad.flatten()[:n].double().cpu().numpy() - g["grad_head"][i][:n]).max()) / \
            (float(g["grad_absmax"][i]) + 1e-3 * gmax)
        en = abs(float(p.grad.double().norm()) - float(g["grad_norm"][i])) / \
            (float(g["grad_norm"][i]) + 1e-3 * gmax * np.sqrt(p.numel()))
        worst, worst_n = max(worst, (err, k)), max(worst_n, (en, k))
    print(f"[train micro {'inplace' if inplace else 'autograd'}] worst relative gradient error {worst[0]:.2e} ({worst[0] / 2e-3:.3f} of "
          f"bound, {worst[1]}); worst norm deviation {worst_n[0]:.2e} ({worst_n[0] / 3e-3:.3f} of bound, {worst_n[1]}); the fp32 "
          f"reference itself: {float(g['ref32_dev_grad']):.2e}")
    assert worst[0] < 2e-3 and worst_n[0] < 3e-3, (worst, worst_n)


def test_captured_micro_step_replays_the_eager_step(monkeypatch):
    """TrainLoop with a predict_xstart diffusion, LFVDM_DETERMINISTIC=1: the same micro-batch with the same noise four
    times - two eager warm-up steps, the capture, one more replay.  The replay's losses and gradient arena against the eager
    step's at the rule tests/test_train_gpu.py uses for a repeated first step (2e-5 of the largest gradient), and replay
    against replay bitwise (the forward pass runs the same kernels in the same order either way: the losses may differ by
    1e-6 relative at most); then four optimizer steps through forward_backward - two eager, two replayed - stay finite."""
    from test_train_gpu import make_loop
    monkeypatch.setenv("LFVDM_DETERMINISTIC", "1")
    g = np.load(os.path.join(GOLDEN, "xstart_train_micro.npz"))
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd).train()
    loop = make_loop(model, max_frames=inp["x0"].shape[1])
    loop.diffusion = make_diffusion("")
    d = {k: v.cuda() for k, v in inp.items()}
    noise = torch.from_numpy(recipe.gaussianish("xstartTrain/noise", inp["x0"].numel()).reshape(inp["x0"].shape).astype(np.float32)).cuda()
    orig = loop.diffusion.training_losses
    loop.diffusion.training_losses = lambda *a, **k: orig(*a, noise=noise, **k)
    inputs = (d["x0"], d["frame_indices"], d["obs_mask"], d["latent_mask"], torch.from_numpy(g["t"]).cuda(), torch.ones(2, device="cuda"))
    runs = []
    for n in range(4):
        loop.arena.zero_grad()
        weighted, raw = loop._graphed_micro_step(inputs)
        loop.exchange.micro_step_done()
        torch.cuda.synchronize()
        runs.append((raw.clone(), weighted["eval-mse"].clone(), loop.arena.g.clone()))
        assert (loop._graph_state.get("graph") is not None) == (n >= 2)
    np.testing.assert_allclose(runs[0][0].cpu().numpy(), g["loss"], rtol=1e-4)      # pad_with_random_frames: mask = 1 - obs_mask
    np.testing.assert_allclose(runs[0][1].cpu().numpy(), g["eval-mse"], rtol=1e-4)
    scale = float(runs[0][2].abs().max())
    dg_, dl = float((runs[2][2] - runs[0][2]).abs().max()), float((runs[2][0] - runs[0][0]).abs().max())
    print(f"[captured micro-step] replay vs eager: gradients {dg_:.2e} ({dg_ / (2e-5 * scale):.3f} of bound), losses {dl:.2e}; "
          f"eager vs eager {float((runs[1][2] - runs[0][2]).abs().max()):.2e}")
    assert scale > 0 and dg_ < 2e-5 * scale and dl <= 1e-6 * float(runs[0][0].abs().max())
    assert torch.equal(runs[2][2], runs[3][2]) and torch.equal(runs[2][0], runs[3][0]), "the replay is bitwise repeatable"
    # the loop itself (device batch preparation, loss-aware logging): two eager optimizer steps, then two replayed ones
    loop.diffusion.training_losses = orig
    p0 = loop.arena.p.clone()
    for n in range(4):
        loop.forward_backward()
        loop.optimize_normal()
        loop.step += 1
        assert (loop._graph_state.get("graph") is not None) == (n >= 2)
    loop._flush_loss_log()
    torch.cuda.synchronize()
    assert torch.isfinite(loop.arena.p).all() and torch.isfinite(loop.arena.g).all() and not torch.equal(loop.arena.p, p0)


# ------------------------------------------------------------------------------------------------ long video
@pytest.mark.parametrize("use_ddim", [False, True], ids=["ancestral", "ddim"])
def test_sample_video_with_an_x0_model(use_ddim):
    from improved_diffusion.video_sampler import default_sampling_args, sample_video
    model, _, _, _ = cfgB()
    diff = make_diffusion("ddim25")
    Tv, n_obs = 30, 4
    batch = torch.from_numpy((0.8 * recipe.gaussianish("xstart/video", 2 * Tv * 4 * 16 * 16)).reshape(2, Tv, 4, 16, 16)
                             .astype(np.float32)).cuda()
    args = default_sampling_args(sampling_scheme="autoreg", n_obs=n_obs, max_frames=10, max_latent_frames=5, device="cuda",
                                 use_ddim=use_ddim, ddim_eta=0.0)
    res = []
    for sd in (21, 21, 22):
        torch.manual_seed(sd)
        res.append(sample_video(args, model, diff, batch, verbose=False)[0])
    assert torch.equal(res[0][:, :n_obs], batch[:, :n_obs]), "the observed frames are untouched"
    assert torch.isfinite(res[0]).all() and float(res[0][:, n_obs:].abs().max()) <= 1.0
    assert not torch.equal(res[0][:, n_obs:], batch[:, n_obs:])
    assert torch.equal(res[0], res[1]), "seed-reproducible"
    assert not torch.equal(res[0], res[2])
    assert all(s.x0_mode and (k[3][0] == "ddim") == use_ddim for k, s in diff._samplers.items())
