"""Native DDIM on the MI355X against the reference's DDIM (tests/golden/ddim_*.npz, written by tools/make_ddim_golden.py
from the reference's ddim_sample / ddim_reverse_sample / ddim_sample_loop in float64): the three update kernels through
the C ABI, the replayed and the eager chain, the reverse-then-forward round trip, the sampler cache and sample_video."""
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
ATOL = 2e-4     # what tests/test_sampler_gpu.py grants the ancestral update against its float64 fixtures


def make_diffusion(resp):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, rescale_timesteps=True,
                                        rescale_learned_sigmas=True, diffusion_space_kwargs=dict(PIXEL))


@functools.lru_cache(maxsize=None)
def cfgB():
    cfg, sd, inp = load_case("cfgB")
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    return model, d, mk, tuple(inp["x"].shape)


# ------------------------------------------------------------------------------------------------ the update kernels
def _one_hot_head(eps, C=64):
    """Channels-last activation rows and packed filters [Cout][9][C] whose 3x3 convolution IS ``eps`` (centre tap, channel
    co -> output co, everything else 0: the sum adds exact zeros), so the fused kernel's own convolution output is the
    fixture's eps."""
    B, T, Co, H, W = eps.shape
    act = torch.zeros(B * T * H * W, C, device="cuda")
    act[:, :Co] = eps.permute(0, 1, 3, 4, 2).reshape(-1, Co)
    wp = torch.zeros(Co, 9, C, device="cuda")
    for co in range(Co):
        wp[co, 4, co] = 1.0
    return act, wp, torch.zeros(Co, device="cuda")


def _run_kernel(kind, diff, x, eps, z, t, co, clip, seed=None):
    """One DDIM update through the C ABI.  kind: given | rng | fused.  -> sample, pred, noise used (or None), eps_out"""
    from improved_diffusion import _native as nat
    tb = diff.tables(x.device)
    r, rm1 = tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"]
    sample, pred = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    if kind == "given":
        nat.update_x0(x, eps, z, t, r, rm1, co["k1"], co["k2"], co["sigma"], nat.RULE_DDIM, nat.MEAN_EPS, clip, sample, pred)
        return sample, pred, z, None
    if kind == "rng":
        zo = torch.full_like(x, float("nan"))
        nat.update_rng_x0(x, eps, zo, t, r, rm1, co["k1"], co["k2"], co["sigma"], nat.RULE_DDIM, nat.MEAN_EPS, clip, sample, seed,
                          pred)
        return sample, pred, zo, None
    act, wp, bias = _one_hot_head(eps)
    assert nat.lib().lfvdm_conv_out_psample_ok(x.shape[0] * x.shape[1], x.shape[3], x.shape[4], act.shape[1], x.shape[2]) == 0
    eps_out = torch.full_like(x, float("nan"))
    zo = torch.full_like(x, float("nan"))
    nat.conv_out_update_x0(act, wp, bias, eps_out, x, z if seed is None else None, zo if seed is not None else None, t, r, rm1,
                           co["k1"], co["k2"], co["sigma"], nat.RULE_DDIM, nat.MEAN_EPS, clip, sample, seed, pred)
    return sample, pred, (zo if seed is not None else z), eps_out


@pytest.mark.parametrize("tag,resp", [("d1000", ""), ("ddim50", "ddim50")])
def test_update_kernels_match_the_reference(tag, resp):
    """ddim_sample at eta 0 / 0.5 / 1 and ddim_reverse_sample, clamp on and off, t = 0, 1, middle, last: all three kernels
    against the reference's float64 update.  atol 2e-4 on the sample and 2e-4 * sqrt_recip_alphas_cumprod[t] on x0-hat
    (per batch row), the ancestral update's bound.  The kernels that draw their own noise are compared after replacing the
    fixture's z by theirs with the reference's float64 sigma table (sample + sigma (z_kernel - z_fixture))."""
    g = np.load(os.path.join(GOLDEN, "ddim_update.npz"))
    diff = make_diffusion(resp)
    seed = torch.tensor([20240607], dtype=torch.int64, device="cuda")
    worst = {}
    for case in (f"{tag}/t0", f"{tag}/t1"):
        share = float(g[f"{case}/clamp_share"])
        assert 0.1 < share < 0.6, "the clamp bites in a real share of the elements"
        tv = g[f"{case}/t"]
        x, eps, z = (torch.from_numpy(g[f"{case}/{k}"]).cuda() for k in ("x", "eps", "z"))
        t = torch.from_numpy(tv).cuda()
        B = x.shape[0]
        amp = torch.from_numpy(diff.sqrt_recip_alphas_cumprod[tv]).view(B, 1, 1, 1, 1)
        nz = torch.from_numpy((tv != 0).astype(np.float64)).view(B, 1, 1, 1, 1)
        for clip in (0, 1):
            want_pred = torch.from_numpy(g[f"{case}/clip{clip}/pred_xstart"])
            for mode in ETAS + ("reverse",):
                reverse = mode == "reverse"
                eta = 0.0 if reverse else mode
                co = diff.ddim_tables("cuda", eta, reverse)
                assert (co["sigma"] is None) == (eta == 0.0)
                want = torch.from_numpy(g[f"{case}/clip{clip}/{'reverse' if reverse else f'eta{eta}'}/sample"])
                sig = torch.from_numpy(g[f"{tag}/eta{eta}/sigma"][tv]).view(B, 1, 1, 1, 1)
                for kind, sd in (("given", None), ("rng", seed), ("fused", None), ("fused", seed)):
                    if eta == 0.0 and sd is not None and kind == "fused":
                        continue                # deterministic: the seed is not read (checked in the next test)
                    sample, pred, zk, eps_out = _run_kernel(kind, diff, x, eps, z, t, co, clip, sd)
                    torch.cuda.synchronize()
                    exp = want if eta == 0.0 else want + nz * sig * (zk.double().cpu() - z.double().cpu())
                    if eps_out is not None:
                        assert torch.equal(eps_out, eps), "the convolution's own output is the fixture's eps"
                    es = (sample.double().cpu() - exp).abs()
                    ep = (pred.double().cpu() - want_pred).abs()
                    key = (kind, "seed" if sd is not None else "z", mode)
                    w = worst.get(key, (0.0, 0.0))
                    worst[key] = (max(w[0], float(es.max())), max(w[1], float((ep / amp).max())))
                    assert bool((es <= ATOL).all()), (case, clip, mode, kind, float(es.max()))
                    assert bool((ep <= ATOL * amp).all()), (case, clip, mode, kind, float((ep / amp).max()))
    for key, (es, ep) in sorted(worst.items(), key=str):
        print(f"[{tag}] {key}: max|d sample| {es:.2e}  max|d pred_xstart| / amp {ep:.2e}")


def test_eta0_does_no_noise_work():
    """eta = 0 (and the reverse step) run the deterministic instantiation: the result does not depend on the seed or on
    what the noise buffers hold (NaN here), nothing is written to noise_out, and two runs are bitwise equal."""
    g = np.load(os.path.join(GOLDEN, "ddim_update.npz"))
    diff = make_diffusion("ddim50")
    case = "ddim50/t1"
    x, eps = (torch.from_numpy(g[f"{case}/{k}"]).cuda() for k in ("x", "eps"))
    t = torch.from_numpy(g[f"{case}/t"]).cuda()
    nan = torch.full_like(x, float("nan"))
    from improved_diffusion import _native as nat
    tb = diff.tables("cuda")
    r, rm1 = tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"]
    act, wp, bias = _one_hot_head(eps)
    for reverse in (False, True):
        co = diff.ddim_tables("cuda", 0.0, reverse)
        assert co["sigma"] is None
        outs = []
        for seed_value in (1, 987654321):
            seed = torch.tensor([seed_value], dtype=torch.int64, device="cuda")
            for kind in ("given", "rng", "fused"):
                sample, pred = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
                zbuf = nan.clone()
                if kind == "given":
                    nat.update_x0(x, eps, zbuf, t, r, rm1, co["k1"], co["k2"], None, nat.RULE_DDIM, nat.MEAN_EPS, True, sample, pred)
                elif kind == "rng":
                    nat.update_rng_x0(x, eps, zbuf, t, r, rm1, co["k1"], co["k2"], None, nat.RULE_DDIM, nat.MEAN_EPS, True, sample,
                                      seed, pred)
                else:
                    nat.conv_out_update_x0(act, wp, bias, None, x, zbuf, zbuf, t, r, rm1, co["k1"], co["k2"], None,
                                           nat.RULE_DDIM, nat.MEAN_EPS, True, sample, seed, pred)
                torch.cuda.synchronize()
                assert torch.isfinite(sample).all() and torch.isfinite(pred).all(), kind
                assert torch.isnan(zbuf).all(), f"{kind}: the noise buffer is neither read nor written"
                outs.append((sample, pred))
        for s_, p_ in outs[1:]:
            assert torch.equal(s_, outs[0][0]) and torch.equal(p_, outs[0][1]), "all kernels, all seeds: bitwise one result"


def test_eta_positive_draws_the_ancestral_noise_stream():
    """Same (seed, t, element) -> the same z under either rule: what lfvdm_update_rng_x0 and lfvdm_conv_out_update_x0 write
    to noise_out under LFVDM_RULE_DDIM is bitwise what lfvdm_update_rng_x0 writes under LFVDM_RULE_ANCESTRAL."""
    from improved_diffusion import _native as nat
    g = np.load(os.path.join(GOLDEN, "ddim_update.npz"))
    diff = make_diffusion("ddim50")
    case = "ddim50/t0"
    x, eps = (torch.from_numpy(g[f"{case}/{k}"]).cuda() for k in ("x", "eps"))
    t = torch.from_numpy(g[f"{case}/t"]).cuda()
    tb = diff.tables("cuda")
    r, rm1 = tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"]
    co = diff.ddim_tables("cuda", 1.0)
    for seed_value in (5, -77):
        seed = torch.tensor([seed_value], dtype=torch.int64, device="cuda")
        z_anc, z_ddim = torch.zeros_like(x), torch.zeros_like(x)
        nat.update_rng_x0(x, eps, z_anc, t, r, rm1, tb["posterior_mean_coef1"], tb["posterior_mean_coef2"],
                          tb["model_log_variance"], nat.RULE_ANCESTRAL, nat.MEAN_EPS, True, torch.empty_like(x), seed)
        nat.update_rng_x0(x, eps, z_ddim, t, r, rm1, co["k1"], co["k2"], co["sigma"], nat.RULE_DDIM, nat.MEAN_EPS, True,
                          torch.empty_like(x), seed)
        _, _, z_fused, _ = _run_kernel("fused", diff, x, eps, None, t, co, True, seed)
        torch.cuda.synchronize()
        assert float(z_anc.std()) > 0.5
        assert torch.equal(z_anc, z_ddim) and torch.equal(z_anc, z_fused)


def test_spaced_ddim_sample_sends_the_original_timestep():
    """ddim_sample / ddim_reverse_sample on a ddim50 diffusion call the network with the ORIGINAL timestep (index 7 of the
    stride-20 schedule -> 140), as p_sample does (reference respace.py:110-124)."""
    diff = make_diffusion("ddim50")
    assert diff.timestep_map[7] == 140
    seen = []
    x = torch.randn(2, 3, 4, 8, 8, device="cuda")

    class Net:
        def __call__(self, x_, timesteps=None, **kw):
            seen.append(timesteps.clone())
            return 0.1 * x_, None
    t = torch.tensor([7, 0], device="cuda")
    diff.ddim_sample(Net(), x, t, model_kwargs={})
    diff.ddim_reverse_sample(Net(), x, t, model_kwargs={})
    diff.ddim_sample(Net(), x, t, model_kwargs={}, denoised_fn=lambda v: v * 0.5, eta=0.5)
    for ts in seen:
        assert ts.tolist() == [140.0, 0.0], ts
    with pytest.raises(AssertionError):
        diff.ddim_reverse_sample(Net(), x, t, model_kwargs={}, eta=0.5)


# ------------------------------------------------------------------------------------------------ trajectories
def _step_fixture(g, key, j):
    gj = {k: g[f"{key}/{k}"][j] for k in ("sub", "frame_sum", "frame_norm")}
    gj["stride"] = g[f"{key}/stride"]
    return gj


def _bounds(g, diff, j, i):
    """Per-step bounds of a ddim10 chain at cfg B.  On the sample: 2e-4 per step taken, the bound
    test_replayed_cfgB_sampler_plan_follows_the_reference_trajectory uses at this shape.  That bound was set at the top of a
    1000-step chain; where a step of this chain needs more, the yardstick is the reference's OWN float32 run from the same
    inputs (``ref32_dev`` in the fixture: its deviation from the float64 trajectory), times three: two correct fp32
    implementations that round differently can each be off by that much in opposite directions, plus one for the MFMA
    summation order.  x0-hat carries the factor sqrt_recip_alphas_cumprod[t] on top, as in the update test."""
    amp = float(diff.sqrt_recip_alphas_cumprod[i])
    bs = max(ATOL * (j + 1), 3.0 * float(g["ref32_dev/sample"][j]))
    bp = max(ATOL * (j + 1) * amp, 3.0 * float(g["ref32_dev/pred_xstart"][j]))
    return bs, bp


CONFIGS = {   # what the replayed chain is built from; each entry differs from the default in one setting
    "default": {},
    "no_level_chains": {"LFVDM_LEVEL_CHAIN": "0"},
    "no_time_tables": {"LFVDM_TIME_TABLES": "0"},
    "one_step_per_graph": {"LFVDM_STEPS_PER_GRAPH": "1"},
    "two_launch_head": {"LFVDM_FUSED_HEAD": "0"},
}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_replayed_ddim10_chain_follows_the_reference_trajectory(config, monkeypatch):
    """ddim_sample_loop_progressive (captured graph) at cfg B on ddim10, eta = 0, from the fixture's start noise: sample and
    x0-hat of all 10 steps against the reference; ddim_sample_loop (K steps per launch) returns the last of them."""
    for k, v in CONFIGS[config].items():
        monkeypatch.setenv(k, v)
    g = np.load(os.path.join(GOLDEN, "ddim_traj_cfgB_eta0.npz"))
    model, d, mk, shape = cfgB()
    diff = make_diffusion("ddim10")
    assert np.array_equal(np.array(diff.timestep_map), g["timestep_map"])
    outs = []
    for j, out in enumerate(diff.ddim_sample_loop_progressive(model, shape, noise=d["x"].clone(), clip_denoised=True,
                                                              model_kwargs=mk, eta=0.0)):
        assert set(out) == {"sample", "pred_xstart"}
        i = 9 - j
        bs, bp = _bounds(g, diff, j, i)
        es = compare_to_fixture(out["sample"], _step_fixture(g, "sample", j), atol=bs, rtol=0.0)
        ep = compare_to_fixture(out["pred_xstart"], _step_fixture(g, "pred_xstart", j), atol=bp, rtol=0.0)
        print(f"[ddim10 {config}] step {j} (t={i}): sample {es:.2e} (bound {bs:.2e}, fp32 reference {g['ref32_dev/sample'][j]:.2e})"
              f"  pred_xstart {ep:.2e} (bound {bp:.2e}, fp32 reference {g['ref32_dev/pred_xstart'][j]:.2e})")
        outs.append(out["sample"])
    assert len(outs) == 10
    assert torch.equal(outs[-1], out["pred_xstart"]), "t = 0 of the chain: k1 = 1, k2 = 0"
    (key, s), = diff._samplers.items()
    assert key[1] == shape and key[3] == ("ddim", 0.0)
    assert s.plan.head_fused == (config != "two_launch_head")
    assert bool(s.plan.chains) == (config != "no_level_chains")
    assert bool(s.plan.time_steps) == (config != "no_time_tables")
    assert s.K == (1 if config == "one_step_per_graph" else 8)
    s.noise.fill_(float("nan"))              # eta = 0 never looks at the sampler's noise buffer
    final = diff.ddim_sample_loop(model, shape, noise=d["x"].clone(), clip_denoised=True, model_kwargs=mk, eta=0.0,
                                  return_decoded=False)
    assert torch.isnan(s.noise).all()
    assert torch.equal(final, outs[-1]), "run() with K steps per launch == 10 single replays"
    assert len(diff._samplers) == 1


def test_eager_ddim10_chain_follows_the_reference_and_the_replayed_chain():
    """The eager ddim_sample loop (model call + lfvdm_update_x0 per step) against the same fixtures and bounds, and against
    the replayed chain (two fp32 evaluations of one trajectory: twice the per-step bound)."""
    g = np.load(os.path.join(GOLDEN, "ddim_traj_cfgB_eta0.npz"))
    model, d, mk, shape = cfgB()
    diff = make_diffusion("ddim10")
    replayed = [(o["sample"], o["pred_xstart"]) for o in
                diff.ddim_sample_loop_progressive(model, shape, noise=d["x"].clone(), clip_denoised=True, model_kwargs=mk)]
    x = d["x"].clone()
    with torch.no_grad():
        for j, i in enumerate(range(9, -1, -1)):
            t = torch.full((shape[0],), i, device="cuda", dtype=torch.long)
            out = diff.ddim_sample(model, x, t, clip_denoised=True, model_kwargs=mk, eta=0.0)
            x = out["sample"]
            bs, bp = _bounds(g, diff, j, i)
            es = compare_to_fixture(x, _step_fixture(g, "sample", j), atol=bs, rtol=0.0)
            ep = compare_to_fixture(out["pred_xstart"], _step_fixture(g, "pred_xstart", j), atol=bp, rtol=0.0)
            dr = float((x - replayed[j][0]).abs().max())
            print(f"[ddim10 eager] step {j} (t={i}): sample {es:.2e} pred_xstart {ep:.2e}; vs replayed {dr:.2e}")
            assert dr <= 2 * bs, (j, dr)
            assert float((out["pred_xstart"] - replayed[j][1]).abs().max()) <= 2 * bp


@pytest.mark.parametrize("fused", ["1", "0"])
def test_replayed_eta1_chain_with_injected_noise(fused, monkeypatch):
    """eta = 1 with the fixture's per-step noise (GraphSampler inject_noise=True), four steps from the top of ddim10; and the
    eager ddim_sample with the same noise."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    monkeypatch.setenv("LFVDM_FUSED_HEAD", fused)
    g = np.load(os.path.join(GOLDEN, "ddim_traj_cfgB_eta1.npz"))
    model, d, mk, shape = cfgB()
    diff = make_diffusion("ddim10")
    s = GraphSampler(diff, model, shape, True, inject_noise=True, rule=("ddim", 1.0))
    s.begin(d["x"].clone(), mk)
    assert s.plan.head_fused == (fused == "1")
    x = d["x"].clone()
    n = d["x"].numel()
    for j, i in enumerate(range(9, 5, -1)):
        noise = torch.from_numpy(recipe.gaussianish(f"ddimB/eta1/noise{j}", n).reshape(shape).astype(np.float32)).cuda()
        s.noise.copy_(noise)
        out = s.step(i)
        bs, bp = _bounds(g, diff, j, i)
        es = compare_to_fixture(out["sample"], _step_fixture(g, "sample", j), atol=bs, rtol=0.0)
        ep = compare_to_fixture(out["pred_xstart"], _step_fixture(g, "pred_xstart", j), atol=bp, rtol=0.0)
        with torch.no_grad():
            t = torch.full((shape[0],), i, device="cuda", dtype=torch.long)
            x = diff.ddim_sample(model, x, t, clip_denoised=True, model_kwargs=mk, eta=1.0, noise=noise)["sample"]
        ee = compare_to_fixture(x, _step_fixture(g, "sample", j), atol=bs, rtol=0.0)
        print(f"[ddim10 eta=1 fused={fused}] step {j} (t={i}): replayed sample {es:.2e} pred_xstart {ep:.2e}; eager sample {ee:.2e} "
              f"(bound {bs:.2e})")
    # kernel noise: a seeded chain repeats, another seed gives another video
    torch.manual_seed(3)
    a = diff.ddim_sample_loop(model, shape, noise=d["x"].clone(), model_kwargs=mk, eta=1.0, return_decoded=False)
    torch.manual_seed(3)
    b = diff.ddim_sample_loop(model, shape, noise=d["x"].clone(), model_kwargs=mk, eta=1.0, return_decoded=False)
    torch.manual_seed(4)
    c = diff.ddim_sample_loop(model, shape, noise=d["x"].clone(), model_kwargs=mk, eta=1.0, return_decoded=False)
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(a).all()


def test_cfgD_window_on_ddim25():
    """One 14-frame window of the long-video configuration (batch 1) on ddim25, eta = 0: the final sample against the
    reference's.  25 steps taken: 2e-4 * 25, or three times the reference's own float32 deviation if that is larger."""
    g = np.load(os.path.join(GOLDEN, "ddim_window_cfgD.npz"))
    model, _, _, _ = cfgB()
    K = 14
    inp = {k: torch.from_numpy(v) for k, v in recipe.make_inputs(f"cfgD_w{K}", 1, K, 4, 16, 16).items()}
    n_obs = int(g["n_obs"])
    obs = torch.zeros(1, K, 1, 1, 1)
    obs[:, :n_obs] = 1.0
    mk = dict(frame_indices=torch.from_numpy(g["frame_indices"]).cuda(), obs_mask=obs.cuda(), latent_mask=(1 - obs).cuda(),
              x0=inp["x0"].cuda())
    diff = make_diffusion("ddim25")
    out = diff.ddim_sample_loop(model, tuple(inp["x"].shape), noise=inp["x"].cuda(), clip_denoised=True, model_kwargs=mk,
                                return_decoded=False)
    bound = max(ATOL * 25, 3.0 * float(g["ref32_dev"]))
    err = compare_to_fixture(out, {"out": g["out"]}, atol=bound, rtol=0.0)
    print(f"[cfgD window K=14 ddim25] final sample {err:.2e} (bound {bound:.2e}, fp32 reference {float(g['ref32_dev']):.2e})")


def test_reverse_then_forward_round_trip():
    """ddim_reverse_sample for t = 0 .. 9 of ddim10 from the clean cfg-B latent, then ddim_sample_loop from the result: both
    against the REFERENCE's round trip (DDIM inversion at 10 steps is only approximately invertible, so the start latent is
    not the yardstick).  10 and 20 steps taken."""
    g = np.load(os.path.join(GOLDEN, "ddim_roundtrip_cfgB.npz"))
    model, d, mk, shape = cfgB()
    diff = make_diffusion("ddim10")
    x = d["x0"].clone()
    with torch.no_grad():
        for i in range(10):
            t = torch.full((shape[0],), i, device="cuda", dtype=torch.long)
            x = diff.ddim_reverse_sample(model, x, t, clip_denoised=True, model_kwargs=mk)["sample"]
    back = diff.ddim_sample_loop(model, shape, noise=x.clone(), clip_denoised=True, model_kwargs=mk, return_decoded=False)
    for key, got, steps in (("encoded", x, 10), ("decoded", back, 20)):
        gk = {k: g[f"{key}/{k}"] for k in ("sub", "frame_sum", "frame_norm", "stride")}
        bound = max(ATOL * steps, 3.0 * float(g[f"ref32_dev/{key}"]))
        err = compare_to_fixture(got, gk, atol=bound, rtol=0.0)
        print(f"[round trip] {key}: {err:.2e} (bound {bound:.2e}, fp32 reference {float(g[f'ref32_dev/{key}']):.2e})")


# ------------------------------------------------------------------------------------------------ cache and long video
def test_ancestral_chain_is_untouched_by_a_ddim_chain_in_between():
    """The sampler cache is keyed by the rule: an ancestral chain after a DDIM chain on the same model and shape is bitwise
    the ancestral chain before it, and bitwise that of a diffusion object that never ran DDIM."""
    model, d, mk, shape = cfgB()

    def ancestral(diff):
        torch.manual_seed(11)
        return diff.p_sample_loop(model, shape, noise=d["x"].clone(), clip_denoised=True, model_kwargs=mk,
                                  return_decoded=False)[0]
    diff = make_diffusion("ddim10")
    a0 = ancestral(diff)
    for eta in (0.0, 1.0):
        diff.ddim_sample_loop(model, shape, noise=d["x"].clone(), clip_denoised=True, model_kwargs=mk, eta=eta,
                              return_decoded=False)
    a1 = ancestral(diff)
    fresh = ancestral(make_diffusion("ddim10"))
    assert torch.equal(a0, a1) and torch.equal(a0, fresh)
    keys = list(diff._samplers)
    assert sorted(k[3] for k in keys) == [("ancestral",), ("ddim", 0.0), ("ddim", 1.0)]
    assert all(k[1] == shape and k[1][1] == 20 for k in keys), "the shape stays at position 1 of the key"
    assert len({id(s.graph) for s in diff._samplers.values()}) == 3


@pytest.mark.parametrize("scheme", ["autoreg", "hierarchy-2"])
def test_sample_video_selects_the_sampler(scheme):
    """sample_video with use_ddim=True on ddim25 equals the loop of ddim_sample_loop calls written out here with the same
    seeds; with use_ddim=False it is bitwise what an argument namespace without the new attributes gives (today's callers):
    the ancestral chain."""
    from improved_diffusion.video_sampler import default_sampling_args, sample_video, window_inputs
    from improved_diffusion.sampling_schemes import sampling_schemes
    model, _, _, _ = cfgB()
    diff = make_diffusion("ddim25")
    Tv, n_obs = 30, 4
    batch = torch.from_numpy((0.8 * recipe.gaussianish("ddim/video", 2 * Tv * 4 * 16 * 16)).reshape(2, Tv, 4, 16, 16)
                             .astype(np.float32)).cuda()
    kw = dict(sampling_scheme=scheme, n_obs=n_obs, max_frames=10, max_latent_frames=5, device="cuda")
    for eta in ((0.0, 0.5) if scheme == "autoreg" else (0.0,)):
        torch.manual_seed(21)
        got, used = sample_video(default_sampling_args(use_ddim=True, ddim_eta=eta, **kw), model, diff, batch, verbose=False)
        torch.manual_seed(21)
        samples = torch.zeros_like(batch)
        samples[:, :n_obs] = batch[:, :n_obs]
        it = iter(sampling_schemes[scheme](video_length=Tv, num_obs=n_obs, max_frames=10, step_size=5,
                                           optimal_schedule_path=None))
        rows = torch.arange(2, device="cuda")[:, None]
        n_windows = 0
        while True:
            it.set_videos(samples)
            try:
                obs_idx, lat_idx = next(it)
            except StopIteration:
                break
            fi, x0, om, lm = window_inputs(samples, obs_idx, lat_idx, "cuda")
            local = diff.ddim_sample_loop(model, tuple(x0.shape), clip_denoised=True, eta=eta,
                                          model_kwargs=dict(frame_indices=fi, x0=x0, obs_mask=om, latent_mask=lm))
            samples[rows, fi[:, -len(lat_idx[0]):]] = local[:, -len(lat_idx[0]):]
            n_windows += 1
        assert n_windows == len(used) >= 3
        assert torch.equal(got, samples) and torch.isfinite(got).all()
        assert not torch.equal(got[:, n_obs:], batch[:, n_obs:])
    assert all(k[3][0] == "ddim" for k in diff._samplers)
    # the ancestral path: flag off == flag absent (the same seeds)
    from types import SimpleNamespace
    a = default_sampling_args(**kw)
    legacy = SimpleNamespace(**{k: v for k, v in vars(a).items() if k not in ("use_ddim", "ddim_eta")})
    res = []
    for args in (a, legacy):
        torch.manual_seed(22)
        res.append(sample_video(args, model, diff, batch, verbose=False)[0])
    assert torch.equal(res[0], res[1]) and not torch.equal(res[0], got)
    assert any(k[3] == ("ancestral",) for k in diff._samplers)
