"""Diffusion step math + sampling loop on the MI355X vs reference golden vectors (GPU only)."""
import os

import numpy as np
import pytest
import torch

from oracle import recipe
from conftest import GOLDEN
from test_oracle_golden import load_case
from test_forward_gpu import build_native

pytestmark = pytest.mark.gpu

PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}


def make_diffusion(steps, resp):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=steps, timestep_respacing=resp, rescale_timesteps=True,
                                        rescale_learned_sigmas=True, diffusion_space_kwargs=dict(PIXEL))


@pytest.mark.parametrize("tag,steps,resp", [("lin1000", 1000, ""), ("lin1000_r250", 1000, "250")])
def test_diffusion_against_reference_golden(tag, steps, resp):
    g = np.load(os.path.join(GOLDEN, "diffusion.npz"))
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd)
    diff = make_diffusion(steps, resp)
    assert np.array_equal(diff.betas, g[f"{tag}/betas"]) and np.array_equal(np.array(diff.timestep_map), g[f"{tag}/timestep_map"])
    assert np.array_equal(diff.posterior_mean_coef2, g[f"{tag}/posterior_mean_coef2"])
    d = {k: v.cuda() for k, v in inp.items()}
    shape = inp["x"].shape
    noise = [torch.from_numpy(recipe.gaussianish(f"diff/noise{i}", inp["x"].numel()).reshape(shape).astype(np.float32)).cuda()
             for i in range(6)]
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    t = torch.from_numpy(g[f"{tag}/t"]).cuda()
    with torch.no_grad():
        xq = diff.q_sample(d["x0"], t, noise=noise[0])
        np.testing.assert_allclose(xq.cpu().numpy(), g[f"{tag}/q_sample"], atol=1e-6)
        losses = diff.training_losses(model, d["x0"], t, model_kwargs=mk, noise=noise[0],
                                      latent_mask=1 - d["obs_mask"], eval_mask=d["latent_mask"])
        for k in ("mse", "eval-mse", "loss"):
            np.testing.assert_allclose(losses[k].cpu().numpy(), g[f"{tag}/loss/{k}"], rtol=2e-4, atol=1e-6)
        pmv = diff.p_mean_variance(model, d["x"], t, clip_denoised=True, model_kwargs=mk)
        np.testing.assert_allclose(pmv["mean"].cpu().numpy(), g[f"{tag}/pmv/mean"], atol=1e-4)
        amp = 1.0 + float(diff.sqrt_recipm1_alphas_cumprod[g[f"{tag}/t"]].max())
        np.testing.assert_allclose(pmv["pred_xstart"].cpu().numpy(), g[f"{tag}/pmv/pred_xstart"], atol=1e-4 * amp)
        np.testing.assert_allclose(pmv["variance"].cpu().numpy()[:, :1, :1, :1, :1], g[f"{tag}/pmv/variance"], rtol=1e-6)
        np.testing.assert_allclose(pmv["log_variance"].cpu().numpy()[:, :1, :1, :1, :1], g[f"{tag}/pmv/log_variance"], rtol=1e-6)
        # 5-step ancestral trajectory with the recorded noise (reference p_sample, :369-401)
        nt = diff.num_timesteps
        x = d["x"].clone()
        for j, i in enumerate(range(nt - 1, nt - 6, -1)):
            ti = torch.full((shape[0],), i, device="cuda", dtype=torch.long)
            x = diff.p_sample(model, x, ti, clip_denoised=True, model_kwargs=mk, noise=noise[j + 1])["sample"]
            err = float((x.cpu() - torch.from_numpy(g[f"{tag}/traj"][j])).abs().max())
            print(f"[{tag}] step {j}: max|d| vs reference trajectory {err:.2e}")
            assert err < 2e-4 * (j + 1)
        ti = torch.zeros(shape[0], device="cuda", dtype=torch.long)
        xl = diff.p_sample(model, d["x"], ti, clip_denoised=True, model_kwargs=mk, noise=noise[0])["sample"]
        np.testing.assert_allclose(xl.cpu().numpy(), g[f"{tag}/p_sample_t0"], atol=2e-4)


def test_graph_sampler_matches_eager_step():
    """One hipGraph replay == eager p_sample with the same noise; loop API returns finite samples."""
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd)
    diff = make_diffusion(1000, "250")
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    shape = tuple(inp["x"].shape)
    s = diff._graph_sampler(model, shape, True)
    s.begin(d["x"].clone(), mk)
    nt = diff.num_timesteps
    for i in (nt - 1, nt - 2, nt - 3):
        before = s.plan.x_in.clone()
        out = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in s.step(i).items()}
        noise = s.noise.clone()
        ti = torch.full((shape[0],), i, device="cuda", dtype=torch.long)
        with torch.no_grad():
            ref = diff.p_sample(model, before, ti, clip_denoised=True, model_kwargs=mk, noise=noise)
        # (the sampler's private plan is autotuned: other tile shapes => fp32 re-association differences)
        assert torch.allclose(out["sample"], ref["sample"], atol=2e-4), float((out["sample"] - ref["sample"]).abs().max())
        # x0-hat = sqrt(1/acp) x - sqrt(1/acp - 1) eps: the eps difference is amplified by sqrt(1/acp - 1) at this t
        amp = 1.0 + float(diff.sqrt_recipm1_alphas_cumprod[i])
        assert torch.allclose(out["pred_xstart"], ref["pred_xstart"], atol=2e-4 * amp), \
            (float((out["pred_xstart"] - ref["pred_xstart"]).abs().max()), amp)
    # full loop through the public API (250 respaced steps), twice with the same seed -> identical
    torch.manual_seed(0)
    a, attn = diff.p_sample_loop(model, shape, clip_denoised=True, model_kwargs=mk, latent_mask=d["latent_mask"],
                                 return_decoded=False)
    torch.manual_seed(0)
    b, _ = diff.p_sample_loop(model, shape, clip_denoised=True, model_kwargs=mk, latent_mask=d["latent_mask"],
                              return_decoded=False)
    assert attn == {} and a.shape == shape and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)
    assert float(a.abs().max()) < 50
    # progressive generator yields one dict per step and leaves grad mode untouched when abandoned
    gen = diff.p_sample_loop_progressive(model, shape, model_kwargs=mk)
    first = next(gen)
    assert set(first) == {"sample", "pred_xstart", "attn"} and torch.is_grad_enabled()
    gen.close()
    assert torch.is_grad_enabled()


def test_denoised_fn_is_applied_to_x0_hat():
    """denoised_fn (reference gaussian_diffusion.py:305-309): applied to x0-hat before clipping, inside p_mean_variance,
    p_sample and the loop.  Checked against the CPU oracle's step with the same function."""
    from oracle import diffusion_oracle as do, unet_oracle as uo
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd)
    diff = make_diffusion(1000, "")
    tab = do.Tables(do.linear_betas(1000))
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    fn = lambda x: 0.5 * x + 0.1
    t = torch.tensor([700, 0])
    noise = torch.from_numpy(recipe.gaussianish("diff/noise1", inp["x"].numel()).reshape(inp["x"].shape).astype(np.float32))
    with torch.no_grad():
        got = diff.p_sample(model, d["x"], t.cuda(), clip_denoised=True, denoised_fn=fn, model_kwargs=mk, noise=noise.cuda())
        pmv = diff.p_mean_variance(model, d["x"], t.cuda(), clip_denoised=True, denoised_fn=fn, model_kwargs=mk)
        plain = diff.p_sample(model, d["x"], t.cuda(), clip_denoised=True, model_kwargs=mk, noise=noise.cuda())
        eps, _ = uo.unet_forward(sd, cfg, inp["x"], inp["x0"], do.model_timesteps(tab, t), inp["frame_indices"],
                                 inp["obs_mask"], inp["latent_mask"])
    # oracle restatement of the step with the function applied
    bs = lambda a: torch.from_numpy(a[t.numpy()]).float().view(-1, 1, 1, 1, 1)
    pred = fn(bs(tab.sqrt_recip_alphas_cumprod) * inp["x"] - bs(tab.sqrt_recipm1_alphas_cumprod) * eps).clamp(-1, 1)
    mean = bs(tab.posterior_mean_coef1) * pred + bs(tab.posterior_mean_coef2) * inp["x"]
    logvar = np.log(np.append(tab.posterior_variance[1], tab.betas[1:]))
    want = mean + (t != 0).float().view(-1, 1, 1, 1, 1) * torch.exp(0.5 * bs(logvar)) * noise
    amp = 1.0 + float(tab.sqrt_recipm1_alphas_cumprod[700])
    assert torch.allclose(got["pred_xstart"].cpu(), pred, atol=2e-4 * amp)
    assert torch.allclose(pmv["pred_xstart"].cpu(), pred, atol=2e-4 * amp) and torch.allclose(pmv["mean"].cpu(), mean, atol=2e-4 * amp)
    assert torch.allclose(got["sample"].cpu(), want, atol=2e-4 * amp)
    assert not torch.allclose(got["sample"], plain["sample"], atol=1e-3), "the function must change the step"
    # the loop accepts it too (eager path: a Python callback cannot live inside the captured step)
    short = make_diffusion(1000, "4")
    torch.manual_seed(1)
    s, _ = short.p_sample_loop(model, tuple(inp["x"].shape), denoised_fn=fn, model_kwargs=mk, return_decoded=False)
    assert bool(torch.isfinite(s).all()) and float(s.abs().max()) <= 1.0 + 1e-5


def test_latent_space_loop_returns_denormalised_latents():
    """diffusion_space='latent', pre_encoded=True with a stats dict (scripts/video_train.py:87-91): the sampler runs
    on the normalised latents; without a VAE ``return_decoded=True`` is refused BEFORE the chain runs (the reference
    always returns pixels there) and ``decode(..., allow_latents=True)`` hands back z*std+mean."""
    from improved_diffusion import script_util as su
    from oracle import fake_vae
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd)
    st = fake_vae.stats_dict(4)
    diff = su.create_gaussian_diffusion(steps=1000, timestep_respacing="3", rescale_timesteps=True, rescale_learned_sigmas=True,
                                        diffusion_space_kwargs={"diffusion_space": "latent", "pre_encoded": True,
                                                                "pre_encoded_stats_dict": st})
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    torch.manual_seed(2)
    raw, _ = diff.p_sample_loop(model, tuple(inp["x"].shape), model_kwargs=mk, return_decoded=False)
    with pytest.raises(NotImplementedError):
        diff.p_sample_loop(model, tuple(inp["x"].shape), model_kwargs=mk, return_decoded=True)
    want = raw * st["std"].view(1, 1, 4, 1, 1).cuda() + st["mean"].view(1, 1, 4, 1, 1).cuda()
    assert torch.equal(diff.decode(raw, allow_latents=True), want)
    # with the stand-in autoencoder attached the loop decodes
    diff.set_vae(fake_vae.FakeVAE(), fake_vae.FakeImageProcessor(), dtype=torch.float32)
    torch.manual_seed(2)
    dec, _ = diff.p_sample_loop(model, tuple(inp["x"].shape), model_kwargs=mk, return_decoded=True)
    assert dec.shape[:2] == raw.shape[:2] and bool(torch.isfinite(dec).all())


def test_timestep_tables_give_bitwise_the_per_step_result(monkeypatch):
    """The sampler tabulates everything that depends on (t, frame_indices) alone once per chain (FiLM rows, R_q/R_k/R_v)
    and drops the four per-step launches that computed it.  Same kernels on a virtual batch, row-independent arithmetic:
    the samples must be BITWISE those of the per-step plan (LFVDM_TIME_TABLES=0), also for per-sample different t."""
    cfg, sd, inp = load_case("micro")
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    shape = tuple(inp["x"].shape)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("LFVDM_TIME_TABLES", mode)
        monkeypatch.setenv("LFVDM_AUTOTUNE", "0")          # same tile shapes in both runs
        model = build_native(cfg, sd)
        diff = make_diffusion(1000, "25")
        torch.manual_seed(7)
        a, _ = diff.p_sample_loop(model, shape, clip_denoised=True, model_kwargs=mk, return_decoded=False)
        s = diff._graph_sampler(model, shape, True)
        assert bool(s.plan.time_steps) == (mode == "1")
        if mode == "1":
            assert s.table_build_ms > 0 and len(s.plan.steps) < 200
        # arbitrary order / per-sample different t through the step API
        s.begin(d["x"].clone(), mk)
        s.t_buf.copy_(torch.tensor([8, 21], device="cuda"))      # next step: t = (7, 20)
        s.expected_t = 7
        b = s.step(7)["sample"].clone()
        outs[mode] = (a, b, len(s.plan.steps))
    assert torch.equal(outs["1"][0], outs["0"][0]) and torch.equal(outs["1"][1], outs["0"][1])
    assert outs["0"][2] - outs["1"][2] == 4, "three embedding launches and the RPE launch leave the step"


def test_run_is_bitwise_n_single_steps():
    """``GraphSampler.run`` replays K captured steps per graph launch (a launch costs ~18 us of GPU time whatever it
    holds).  The clock is on the device and the noise is keyed by (chain seed, t, element), so the grouping cannot change
    a value: 19 steps through ``run`` (two 8-step launches + three single ones), 19 ``step`` calls and a ``run`` that is
    interrupted by a ``step`` must agree BITWISE, and the chain must end at the same timestep."""
    cfg, sd, inp = load_case("micro")
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    shape = tuple(inp["x"].shape)
    model = build_native(cfg, sd)
    diff = make_diffusion(1000, "")
    s = diff._graph_sampler(model, shape, True)
    assert s.K == 8
    outs = []
    for mode in ("step", "run", "mixed"):
        s.begin(d["x"].clone(), mk)
        s.seed.fill_(12345)                          # the same noise key for the three chains
        if mode == "step":
            for i in range(999, 980, -1):
                out = s.step(i)
        elif mode == "run":
            out = s.run(999, 19)
            assert s.graph_k is not None
        else:
            s.run(999, 9)
            s.step(990)
            out = s.run(989, 9)
        assert s.expected_t == 980 and s.t_buf.tolist() == [981] * shape[0]
        outs.append((out["sample"].clone(), out["pred_xstart"].clone()))
    for a, b in outs[1:]:
        assert torch.equal(outs[0][0], a) and torch.equal(outs[0][1], b)
    # the public loop (25 respaced steps = 3 launches of 8 + 1) equals the progressive generator's last state
    diff25 = make_diffusion(1000, "25")
    torch.manual_seed(3)
    a, _ = diff25.p_sample_loop(model, shape, clip_denoised=True, model_kwargs=mk, return_decoded=False)
    torch.manual_seed(3)
    last = None
    for last in diff25.p_sample_loop_progressive(model, shape, clip_denoised=True, model_kwargs=mk):
        pass
    assert torch.equal(a, last["sample"])


def test_replayed_cfgB_sampler_plan_follows_the_reference_trajectory():
    """The plan the benchmark times - BASELINE.json configs[1] (ch64, batch 2, 20 frames, 4x16x16), autotuned tile
    codes, timestep tables, GroupNorm epilogues, hipGraph replay - against three steps of the REFERENCE's p_sample
    from the top of the 1000-step chain with the recorded noise (tests/golden/sampler_cfgB.npz, generated by
    oracle/make_golden.py::gen_sampler_cfgB from gaussian_diffusion.py:369-401).  Tolerance: 2e-4 per step taken, the
    bound the micro-model trajectories use."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    g = np.load(os.path.join(GOLDEN, "sampler_cfgB.npz"))
    cfg, sd, inp = load_case("cfgB")
    model = build_native(cfg, sd)
    diff = make_diffusion(1000, "")
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    shape = tuple(inp["x"].shape)
    s = GraphSampler(diff, model, shape, True, inject_noise=True)
    s.begin(d["x"].clone(), mk)
    assert s.plan.time_steps == 1000, s.plan.time_table_fallback        # timestep tables on
    assert getattr(s.plan, "tuned", False) and s.graph is not None      # autotuned plan, captured step
    for j, i in enumerate(range(999, 996, -1)):
        noise = torch.from_numpy(recipe.gaussianish(f"samplerB/noise{j}", inp["x"].numel()).reshape(shape).astype(np.float32))
        s.noise.copy_(noise.cuda())
        out = s.step(i)["sample"]
        err = float((out.cpu() - torch.from_numpy(g["traj"][j])).abs().max())
        print(f"[cfgB replay] step {j} (t={i}): max|d| vs reference trajectory {err:.2e}")
        assert err < 2e-4 * (j + 1), (j, err)
    assert s.plan.head_fused, "the benchmarked plan ends in the fused output conv + update"


@pytest.mark.parametrize("name", ["carla32", "cfgB_16x32"])
def test_replayed_sampler_at_32x32_and_nonsquare_latents_follows_the_reference_trajectory(name):
    """The replayed sampler plan (autotuned, level chains, captured step) at the reference's defaults for 4x32x32 latents
    and at the bench model on a 16x32 latent (sample-local chain stages of two samples per tile) against three steps of
    the REFERENCE's p_sample from t = 999 with the recorded noise (oracle/make_golden.py::gen_sampler_nonsquare: a
    subsample plus per-(frame, channel) sums and norms of every step).  Tolerance: 2e-4 per step taken."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    from test_oracle_golden import compare_to_fixture, load_nonsquare
    g = np.load(os.path.join(GOLDEN, f"sampler_{name}.npz"))
    cfg, sd, inp = load_nonsquare(name)
    model = build_native(cfg, sd)
    diff = make_diffusion(1000, "")
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    shape = tuple(inp["x"].shape)
    s = GraphSampler(diff, model, shape, True, inject_noise=True)
    s.begin(d["x"].clone(), mk)
    assert s.plan.time_steps == 1000, s.plan.time_table_fallback
    assert getattr(s.plan, "tuned", False) and s.graph is not None
    assert s.plan.chains, "the low-resolution levels run as persistent chains"
    for j, i in enumerate(range(999, 996, -1)):
        noise = torch.from_numpy(recipe.gaussianish(f"sampler_{name}/noise{j}", inp["x"].numel()).reshape(shape).astype(np.float32))
        s.noise.copy_(noise.cuda())
        out = s.step(i)["sample"]
        torch.cuda.synchronize()
        gj = {k: g[k][j] for k in ("sub", "frame_sum", "frame_norm")}
        gj["stride"] = g["stride"]
        err = compare_to_fixture(out, gj, atol=2e-4 * (j + 1), rtol=0.0)
        print(f"[{name} replay] step {j} (t={i}): max|d| vs reference trajectory {err:.2e}")
    assert not s.plan.chains_aborted()
    if name == "carla32":
        assert s.plan.head_fused, "the plan ends in the fused output conv + update"


def test_fused_head_chain_equals_the_two_launch_chain(monkeypatch):
    """cfg-B sampler with the output conv + update in one launch (lfvdm_conv_out_update_x0, the default) against the same
    chain with the two launches (LFVDM_FUSED_HEAD=0): same noise stream (same chain seed), so the only difference is the
    summation order inside the 64 -> 4 convolution - the samples of 12 steps stay within 2e-5."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    cfg, sd, inp = load_case("cfgB")
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    shape = tuple(inp["x"].shape)
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("LFVDM_FUSED_HEAD", fused)
        s = GraphSampler(make_diffusion(1000, ""), model, shape, True)
        s.begin(d["x"].clone(), mk)
        s.seed.fill_(777)
        assert s.plan.head_fused == (fused == "1")
        out = s.run(999, 12)
        outs.append((out["sample"].clone(), out["pred_xstart"].clone(), s.noise.clone(), len(s.plan.steps) + s.extra_launches))
        del s
    assert torch.equal(outs[0][2], outs[1][2]), "the noise of the last step is the same Philox stream"
    assert float((outs[0][0] - outs[1][0]).abs().max()) < 2e-5
    # (pred_xstart = r * x - rm1 * eps amplifies eps by sqrt(1/abar - 1) ~ 1e3 at the top of the chain before the clip)
    assert float((outs[0][1] - outs[1][1]).abs().max()) < 5e-3
    assert outs[1][3] - outs[0][3] == 1, "one launch less per step"



@pytest.mark.parametrize("K", [20, 14])
def test_replayed_long_video_window_follows_the_reference_trajectory(K):
    """The long-video path of BASELINE.json configs[3] against the REFERENCE: batch 1, 250-step respacing, the frame
    indices of a hierarchy-2 window of the T=1000 schedule (window 2: 20 frames with far-away anchor frames; the
    schedule's only 14-frame window) - the batch-1 tune codes, per-window timestep tables, respaced clock and the
    hipGraph replay, vs ``SpacedDiffusion.p_sample`` (gaussian_diffusion.py:369-401 through respace.py:110-124) with
    recorded noise: three steps from the top of the chain and the last two (t = 0 adds no noise).  Fixture
    tests/golden/sampler_cfgD_window.npz (oracle/make_golden.py::gen_sampler_cfgD_window).  2e-4 per step taken."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    g = np.load(os.path.join(GOLDEN, "sampler_cfgD_window.npz"))
    cfg, sd, _ = load_case("cfgB")
    model = build_native(cfg, sd)
    diff = make_diffusion(1000, "250")
    assert diff.num_timesteps == 250
    tag = f"cfgD_w{K}"
    inp = {k: torch.from_numpy(v) for k, v in recipe.make_inputs(tag, 1, K, cfg["in_channels"], 16, 16).items()}
    fi = torch.from_numpy(g[f"w{K}_frame_indices"])
    n_obs = int(g[f"w{K}_n_obs"])
    obs = torch.zeros(1, K, 1, 1, 1)
    obs[:, :n_obs] = 1.0
    mk = dict(frame_indices=fi.cuda(), obs_mask=obs.cuda(), latent_mask=(1 - obs).cuda(), x0=inp["x0"].cuda())
    shape = tuple(inp["x"].shape)
    s = GraphSampler(diff, model, shape, True, inject_noise=True)
    for leg, steps, x in (("top", (249, 248, 247), inp["x"].clone()), ("bottom", (1, 0), 0.5 * inp["x"] + 0.5 * inp["x0"])):
        s.begin(x.cuda(), mk)
        assert s.plan.time_steps == 250, s.plan.time_table_fallback     # per-window timestep tables on
        assert getattr(s.plan, "tuned", False) and s.graph is not None
        for j, i in enumerate(steps):
            noise = torch.from_numpy(recipe.gaussianish(f"{tag}/{leg}/noise{j}", inp["x"].numel()).reshape(shape).astype(np.float32))
            s.noise.copy_(noise.cuda())
            out = s.step(i)["sample"]
            err = float((out.cpu() - torch.from_numpy(g[f"w{K}_{leg}"][j])).abs().max())
            print(f"[cfgD window K={K}] {leg} step {j} (i={i}): max|d| vs reference trajectory {err:.2e}")
            assert err < 2e-4 * (j + 1), (leg, j, err)


def test_long_video_window_at_the_default_batch_of_8():
    """scripts/video_sample.py:171 defaults to --batch_size=8: eight videos per window (video_sample.py:88-99), each with its
    own frame indices.  The replayed window sampler at B = 8 - its own launch shapes (M = 8 x 20 samples: only the 2x2 level
    still runs as a persistent chain), its own tune codes and timestep tables - must (i) follow the REFERENCE trajectory of
    tests/golden/sampler_cfgD_window.npz on row 0, which carries that fixture's window (2e-4 per step taken), and (ii) give
    on every row what a B = 1 sampler gives for that row alone (rows do not talk to each other: unet.py has no op across
    the batch; forward tolerance 2e-4 + 1e-3 |ref|, the shapes and codes differ).  Three steps from the top of the 250-step
    respaced chain, recorded noise."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    g = np.load(os.path.join(GOLDEN, "sampler_cfgD_window.npz"))
    cfg, sd, _ = load_case("cfgB")
    model = build_native(cfg, sd)
    diff = make_diffusion(1000, "250")
    K, B, C_in = 20, 8, cfg["in_channels"]
    rows = []
    rng = np.random.RandomState(7)
    for r in range(B):
        inp = {k: torch.from_numpy(v) for k, v in recipe.make_inputs("cfgD_w20" if r == 0 else f"cfgD_w20_row{r}", 1, K, C_in, 16, 16).items()}
        if r == 0:
            fi, n_obs = torch.from_numpy(g["w20_frame_indices"]), int(g["w20_n_obs"])
        else:       # another window of the schedule's kind: a few far-away anchors, then consecutive latent frames
            n_obs = int(rng.randint(2, 11))
            start = int(rng.randint(40, 900))
            anchors = np.sort(rng.choice(np.arange(0, start - 1), size=n_obs, replace=False))
            fi = torch.from_numpy(np.concatenate([anchors, start + np.arange(K - n_obs)]).astype(np.int64))[None]
        obs = torch.zeros(1, K, 1, 1, 1)
        obs[:, :n_obs] = 1.0
        noise = [torch.from_numpy(recipe.gaussianish(f"cfgD_w20/top/noise{j}" if r == 0 else f"b8/row{r}/noise{j}",
                                                     inp["x"].numel()).reshape(inp["x"].shape).astype(np.float32)) for j in range(3)]
        rows.append(dict(x=inp["x"], x0=inp["x0"], fi=fi, obs=obs, noise=noise))
    cat = lambda k: torch.cat([r[k] for r in rows], 0)      # noqa: E731

    def run(sel):
        x, x0, fi, obs = (torch.cat([rows[r][k] for r in sel], 0) for k in ("x", "x0", "fi", "obs"))
        mk = dict(frame_indices=fi.cuda(), obs_mask=obs.cuda(), latent_mask=(1 - obs).cuda(), x0=x0.cuda())
        s = GraphSampler(diff, model, tuple(x.shape), True, inject_noise=True)
        s.begin(x.clone().cuda(), mk)
        assert s.plan.time_steps == 250, s.plan.time_table_fallback
        outs = []
        for j, i in enumerate((249, 248, 247)):
            s.noise.copy_(torch.cat([rows[r]["noise"][j] for r in sel], 0).cuda())
            outs.append(s.step(i)["sample"].cpu().clone())
        assert not s.chain_timed_out()
        return outs, s

    full, s8 = run(list(range(B)))
    print("[cfgD B=8] chains:", [(c["n"], c["items"]) for c in s8.plan.chains], "launches per step:", len(s8.plan.steps))
    for j in range(3):
        err = float((full[j][0] - torch.from_numpy(g["w20_top"][j])[0]).abs().max())
        print(f"[cfgD B=8] row 0, step {j}: max|d| vs reference trajectory {err:.2e}")
        assert err < 2e-4 * (j + 1), (j, err)
    worst = 0.0
    for r in range(B):
        single, _ = run([r])
        for j in range(3):
            d = (full[j][r] - single[j][0]).abs()
            tol = 2e-4 + 1e-3 * single[j][0].abs()
            worst = max(worst, float(d.max()))
            assert bool((d <= tol).all()), (r, j, float(d.max()))
    print(f"[cfgD B=8] rows vs eight B=1 runs: worst max|d| {worst:.2e}")


def test_rolling_R_window_is_bitwise_the_whole_chain_tables(monkeypatch):
    """The R tables as a rolling window of `ring` timesteps (LFVDM_TIME_RING; slot t % ring, refilled half a ring at a time
    between graph launches) against whole-chain tables (LFVDM_TIME_RING=0): a 100-step chain through the public loop (8-step
    graph launches that straddle the half-ring boundaries: 100 is not a multiple of 16), single steps in arbitrary order,
    and a window's memory must be the ring's share of the chain's."""
    cfg, sd, inp = load_case("micro")
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    shape = tuple(inp["x"].shape)
    outs = {}
    for ring in ("0", "16", "48"):
        monkeypatch.setenv("LFVDM_TIME_RING", ring)
        monkeypatch.setenv("LFVDM_AUTOTUNE", "0")
        model = build_native(cfg, sd)
        diff = make_diffusion(1000, "100")
        torch.manual_seed(11)
        a, _ = diff.p_sample_loop(model, shape, clip_denoised=True, model_kwargs=mk, return_decoded=False)
        s = diff._graph_sampler(model, shape, True)
        assert s.plan.time_steps == 100 and s.plan.time_ring == int(ring)
        s.begin(d["x"].clone(), mk)
        s.seed.fill_(99)
        singles = []
        for i in (99, 98, 50, 7, 8, 63, 64, 0):          # arbitrary order: every access must find its block resident
            singles.append(s.step(i)["sample"].clone())
        s.begin(d["x"].clone(), mk)
        s.seed.fill_(99)
        r = s.run(99, 37)["sample"].clone()               # 4 launches of 8 + 5 single steps, across block boundaries
        outs[ring] = (a, singles, r, s.plan.time_table_bytes, s.chain_table_ms())
    for ring in ("16", "48"):
        assert torch.equal(outs[ring][0], outs["0"][0]), ring
        assert all(torch.equal(x, y) for x, y in zip(outs[ring][1], outs["0"][1])), ring
        assert torch.equal(outs[ring][2], outs["0"][2]), ring
        assert outs[ring][4] > 0
    assert outs["16"][3] < 0.4 * outs["0"][3], (outs["16"][3], outs["0"][3])


DRIFT_GUARD = 1e-4      # flat regression guard of the full-chain drift test: 25x the worst observed deviation (4.1e-6)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("tag", ["cfgD_window", "cfgB"])
def test_full_chain_drift_vs_oracle(tag):
    """"K-step sampler trajectories ... report the observed curve".  The WHOLE chain of the metric's own
    workloads - cfg B (batch 2, 20 frames, 1000 steps) and a cfg-D window (batch 1, 20 frames with hierarchy-2 anchor
    frames, 250-step respacing) - on the MI355X (``GraphSampler(inject_noise=True)``: the replayed, autotuned plan with its
    persistent level chains) and through the CPU oracle (oracle/unet_oracle.py + diffusion_oracle.py, fp32), both FREE
    RUNNING from the same start with the same recipe noise at every step (reference gaussian_diffusion.py:369-401,509-522,
    respace.py:110-124).  Every step is compared; the curve max|x_hip - x_oracle| is printed every 50 steps (collected into
    profiles/r06_parity_deviations.txt).  Two bounds at every step k (1-based): the DERIVED one, 2e-4 * k - the per-step
    tolerance of the trajectory goldens accumulated linearly, not a number tuned to the observation - and
    a REGRESSION GUARD, a flat 1e-4 on the sample: 25x the worst deviation ever observed over a whole chain (4.1e-6, rounds
    5 and 6), so that an error two orders of magnitude above today's fails long before the derived bound (0.2 at the end of cfg
    B) would notice.  The x0 prediction of the last step is held to the same flat bound."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    from oracle import unet_oracle as uo, diffusion_oracle as do
    try:                                       # the GPU box grants 16 host cores per GPU; a 256-thread OpenMP team on a CPU quota crawls
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    torch.set_num_threads(max(1, min(cores, 16)))
    cfg, sd, inp = load_case("cfgB")
    model = build_native(cfg, sd)
    if tag == "cfgB":
        diff, tab = make_diffusion(1000, ""), do.Tables(do.linear_betas(1000))
        x0, x, fi, obs, lat = inp["x0"], inp["x"].clone(), inp["frame_indices"], inp["obs_mask"], inp["latent_mask"]
    else:
        g = np.load(os.path.join(GOLDEN, "sampler_cfgD_window.npz"))
        diff, tab = make_diffusion(1000, "250"), do.Tables(do.linear_betas(1000), do.space_timesteps(1000, "250"))
        K = 20
        w = {k: torch.from_numpy(v) for k, v in recipe.make_inputs(f"cfgD_w{K}", 1, K, cfg["in_channels"], 16, 16).items()}
        x0, x, fi = w["x0"], w["x"].clone(), torch.from_numpy(g[f"w{K}_frame_indices"])
        obs = torch.zeros(1, K, 1, 1, 1)
        obs[:, :int(g[f"w{K}_n_obs"])] = 1.0
        lat = 1 - obs
    n_t = diff.num_timesteps
    shape = tuple(x.shape)
    mk = dict(frame_indices=fi.cuda(), obs_mask=obs.cuda(), latent_mask=lat.cuda(), x0=x0.cuda())
    s = GraphSampler(diff, model, shape, True, inject_noise=True)
    s.begin(x.cuda(), mk)
    assert getattr(s.plan, "tuned", False) and s.graph is not None
    xo = x.clone()
    worst, curve, pred_o = 0.0, [], None
    with torch.no_grad():
        for k, i in enumerate(range(n_t - 1, -1, -1)):
            noise = torch.from_numpy(recipe.gaussianish(f"drift/{tag}/noise{i}", x.numel()).reshape(shape).astype(np.float32))
            s.noise.copy_(noise.cuda())
            out = s.step(i)
            ti = torch.full((shape[0],), i, dtype=torch.long)
            eps = uo.unet_forward(sd, cfg, xo, x0, do.model_timesteps(tab, ti), fi, obs, lat)[0]
            xo, pred_o = do.p_sample(tab, eps, xo, ti, noise)
            err = float((out["sample"].cpu() - xo).abs().max())
            worst = max(worst, err)
            assert err < 2e-4 * (k + 1), (tag, k, i, err)
            assert err < DRIFT_GUARD, (tag, k, i, err)
            if (k + 1) % 50 == 0 or k == 0 or i == 0:
                curve.append((k + 1, err))
                print(flush=True, end="")
                print(f"[drift {tag}] after {k + 1:4d} steps (t={i:3d}): max|x_hip - x_oracle| = {err:.3e}   (bound {2e-4 * (k + 1):.1e})")
    pred_h = s.pred.cpu()
    perr = float((pred_h - pred_o["pred_xstart"]).abs().max()) if isinstance(pred_o, dict) else float((pred_h - pred_o).abs().max())
    print(f"[drift {tag}] whole chain of {n_t} steps: worst max|d| over all steps {worst:.3e}, final sample {curve[-1][1]:.3e}, "
          f"final x0 prediction {perr:.3e}; no persistent-chain timeout: {not s.chain_timed_out()}")
    assert not s.chain_timed_out()
    assert perr < DRIFT_GUARD and bool(torch.isfinite(out["sample"]).all())
