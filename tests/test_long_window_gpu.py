"""Windows of 33 to 64 frames (``--max_frames`` up to 64) on the MI355X: the temporal attention core's long-window kernels
(attention_temporal_long.hip, the 4-row-tile dR kernel) against the fp64 core, and the network, training step, sampler
and long-video loop at 40 / 64 frames against the oracle.  GPU only."""
import numpy as np
import pytest
import torch

from oracle import recipe, unet_oracle as uo, diffusion_oracle as do
from test_ops_gpu import _temporal_core_f64, rnd, close
from test_forward_gpu import build_native
from test_sampler_gpu import make_diffusion
from test_long_video_cpu import run_scheme

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from improved_diffusion import _native
    _native.lib()
    return _native


def _mask(tag, B, T):
    return (torch.from_numpy(recipe.uniform_pm1(tag, B * T)).view(B, T) > 0).float()


# (B, T, P, C, heads): every T of {33, 40, 48, 57, 64}, P of {1, 4, 16, 64, 256, 37}, head dim F of {8, 16, 32, 64, 96, 128}
# and B of {1, 2, 3} appears at least once
@pytest.mark.parametrize("B,T,P,Cc,heads", [(2, 64, 256, 64, 4), (2, 64, 64, 128, 4), (2, 40, 16, 128, 2), (1, 33, 37, 96, 1),
                                            (3, 48, 4, 128, 1), (2, 57, 1, 32, 4), (1, 64, 16, 256, 2), (2, 40, 256, 128, 4),
                                            (3, 33, 64, 64, 8), (2, 64, 4, 192, 2), (1, 57, 37, 64, 1), (2, 48, 16, 32, 4)])
def test_long_window_forward(nat, B, T, P, Cc, heads):
    """Forward core at 33..64 frames vs fp64: with and without the two-clique mask, attention probabilities (rows sum to
    1), the timestep-table forms (_sel == the plain form on the selected R; _ring bitwise == _sel)."""
    M = B * T * P
    qkv = rnd("tl/qkv", M, 3 * Cc)
    Rs = [0.3 * rnd(f"tl/R{i}", B, T, T, Cc) for i in range(3)]
    mask = _mask("tl/mask", B, T)
    ref = _temporal_core_f64(qkv.double(), Rs[0].double(), Rs[1].double(), Rs[2].double(), mask.double(), B, T, P, Cc, heads).float()
    g = [t.cuda().contiguous() for t in (qkv, *Rs, mask)]
    o = torch.full((M, Cc), float("nan"), device="cuda")
    attn = torch.full((B * P, heads, T, T), float("nan"), device="cuda")
    nat.attn_temporal(g[0], g[1], g[2], g[3], g[4], o, attn, B, T, P, Cc, heads)
    close(o, ref, 5e-5)
    assert bool(torch.isfinite(attn).all()) and float((attn.sum(-1) - 1).abs().max()) < 1e-5
    o2 = torch.full((M, Cc), float("nan"), device="cuda")
    nat.attn_temporal(g[0], g[1], g[2], g[3], None, o2, None, B, T, P, Cc, heads)          # no mask
    ref2 = _temporal_core_f64(qkv.double(), Rs[0].double(), Rs[1].double(), Rs[2].double(), torch.ones(B, T).double(), B, T, P, Cc,
                              heads)
    close(o2, ref2.float(), 5e-5)
    n_t = 3
    tabs = [torch.stack([(0.5 + 0.25 * i) * r for i in range(n_t)]).cuda().contiguous() for r in Rs]
    sel = torch.tensor([(2 * b + 1) % n_t for b in range(B)], dtype=torch.int64, device="cuda")
    o3 = torch.full((M, Cc), float("nan"), device="cuda")
    nat.check(nat.lib().lfvdm_attn_temporal_sel(g[0].data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(),
                                                g[4].data_ptr(), o3.data_ptr(), None, B, T, P, Cc, heads, sel.data_ptr(),
                                                nat.stream()), "lfvdm_attn_temporal_sel")
    picked = [torch.stack([(0.5 + 0.25 * int(sel[b])) * r[b] for b in range(B)]).cuda().contiguous() for r in Rs]
    o3p = torch.full((M, Cc), float("nan"), device="cuda")
    nat.attn_temporal(g[0], picked[0], picked[1], picked[2], g[4], o3p, None, B, T, P, Cc, heads)
    assert torch.equal(o3, o3p), "_sel == the plain form on the selected slices"
    ref3 = _temporal_core_f64(qkv.double(), *[p.cpu().double() for p in picked], mask.double(), B, T, P, Cc, heads)
    close(o3, ref3.float(), 5e-5)
    big = torch.tensor([int(sel[b]) + 3 * (7 + b) for b in range(B)], dtype=torch.int64, device="cuda")
    o4 = torch.full((M, Cc), float("nan"), device="cuda")
    nat.check(nat.lib().lfvdm_attn_temporal_ring(g[0].data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(),
                                                 g[4].data_ptr(), o4.data_ptr(), None, B, T, P, Cc, heads, big.data_ptr(), n_t,
                                                 nat.stream()), "lfvdm_attn_temporal_ring")
    assert torch.equal(o4, o3)


@pytest.mark.parametrize("B,T,P,Cc,heads", [(2, 33, 16, 64, 4), (1, 40, 37, 128, 2), (2, 64, 16, 128, 4), (1, 64, 4, 128, 1),
                                            (2, 40, 5, 32, 4), (1, 33, 9, 96, 1), (2, 64, 64, 64, 4), (1, 64, 3, 192, 2)])
def test_long_window_backward(nat, B, T, P, Cc, heads):
    """dqkv, dR_q, dR_k, dR_v at 33..64 frames vs fp64 autograd of the core; every element written (outputs start as NaN:
    rows 32..63 of the dR tensors come from the third and fourth row tiles); bitwise reproducible."""
    M = B * T * P
    qkv = rnd("tlb/qkv", M, 3 * Cc)
    Rs = [0.3 * rnd(f"tlb/R{i}", B, T, T, Cc) for i in range(3)]
    d_o = rnd("tlb/do", M, Cc)
    mask = _mask("tlb/mask", B, T)
    leaves = [t.double().requires_grad_(True) for t in [qkv] + Rs]
    ref = _temporal_core_f64(leaves[0], leaves[1], leaves[2], leaves[3], mask.double(), B, T, P, Cc, heads)
    (ref * d_o.double()).sum().backward()
    g = [t.cuda().contiguous() for t in (qkv, d_o, *Rs, mask)]
    nanf = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    runs = []
    for _ in range(2):
        dqkv, dRq, dRk, dRv = nanf(M, 3 * Cc), nanf(B, T, T, Cc), nanf(B, T, T, Cc), nanf(B, T, T, Cc)
        ws = torch.full((2, B * P * heads * T * T), float("nan"), device="cuda")
        nat.attn_temporal_bwd(g[0], g[1], g[2], g[3], g[4], g[5], ws[0], ws[1], dqkv, dRq, dRk, dRv, B, T, P, Cc, heads)
        runs.append((dqkv, dRq, dRk, dRv))
    for name, got, want in zip(("dqkv", "dRq", "dRk", "dRv"), runs[0], [l.grad for l in leaves]):
        assert bool(torch.isfinite(got).all()), name
        want = want.float()
        err = float((got.cpu() - want).abs().max())
        assert err <= 3e-5 * (1.0 + float(want.abs().max())) + 3e-5, (name, err, float(want.abs().max()))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "no atomics: bitwise reproducible"


def test_more_than_64_frames_is_refused(nat):
    """T = 65: the C entry points return nonzero, the engine names the limit and the flag."""
    from improved_diffusion import _engine
    B, T, P, Cc, heads = 1, 65, 2, 32, 2
    L = nat.lib()
    qkv = torch.zeros(B * T * P, 3 * Cc, device="cuda")
    R = torch.zeros(B, T, T, Cc, device="cuda")
    o = torch.zeros(B * T * P, Cc, device="cuda")
    ws = torch.zeros(2, B * P * heads * T * T, device="cuda")
    p = lambda t: t.data_ptr()
    assert L.lfvdm_attn_temporal(p(qkv), p(R), p(R), p(R), None, p(o), None, B, T, P, Cc, heads, nat.stream()) != 0
    assert L.lfvdm_attn_temporal_sel(p(qkv), p(R), p(R), p(R), None, p(o), None, B, T, P, Cc, heads, None, nat.stream()) != 0
    assert L.lfvdm_attn_temporal_bwd(p(qkv), p(o), p(R), p(R), p(R), None, p(ws[0]), p(ws[1]), p(qkv), p(R), p(R), p(R), B, T, P, Cc,
                                     heads, nat.stream()) != 0
    torch.cuda.synchronize()
    assert _engine.MAX_FRAMES == 64
    cfg = uo.make_cfg(model_channels=32, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2)
    sd = {k: torch.from_numpy(v) for k, v in recipe.fill_state_dict(uo.param_shapes(cfg)).items()}
    model = build_native(cfg, sd)
    inp = {k: torch.from_numpy(v).cuda() for k, v in recipe.make_inputs("tl/65", 1, 65, 4, 4, 4).items()}
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"at most 64 frames.*--max_frames"):
        model(inp["x"], x0=inp["x0"], timesteps=inp["t"].float(), frame_indices=inp["frame_indices"], obs_mask=inp["obs_mask"],
              latent_mask=inp["latent_mask"])


def _small_model(ch=64, mult=(1, 2), heads=4):
    cfg = uo.make_cfg(model_channels=ch, channel_mult=mult, attention_resolutions=(1, 2), num_heads=heads)
    sd = {k: torch.from_numpy(v) for k, v in recipe.fill_state_dict(uo.param_shapes(cfg)).items()}
    return cfg, sd


@pytest.mark.parametrize("T,B,chain", [(40, 2, "1"), (40, 2, "0"), (64, 2, "1"), (64, 2, "0"), (64, 3, "1")])
def test_long_window_network_forward_vs_fp64(monkeypatch, T, B, chain):
    """``UNetVideoModel.forward`` at 40 and 64 frames (16x16 latents, ch64, 3 padding frames; batch 3 at 64 frames is
    192 frame rows, past the sample-local stages' 128), with the level chains on and off: as close to an fp64
    evaluation as the fp32 CPU oracle is (x3), as test_forward_gpu."""
    monkeypatch.setenv("LFVDM_LEVEL_CHAIN", chain)
    cfg, sd = _small_model()
    inp = {k: torch.from_numpy(v) for k, v in recipe.make_inputs(f"tl/net{T}", B, T, 4, 16, 16, n_pad=3).items()}
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    with torch.no_grad():
        out, _ = model(d["x"], x0=d["x0"], timesteps=d["t"].float(), frame_indices=d["frame_indices"], obs_mask=d["obs_mask"],
                       latent_mask=d["latent_mask"])
        sd64 = {k: v.double() for k, v in sd.items()}
        f64 = lambda t: t.double() if t.is_floating_point() else t
        t64, _ = uo.unet_forward(sd64, cfg, f64(inp["x"]), f64(inp["x0"]), inp["t"].double(), inp["frame_indices"],
                                 f64(inp["obs_mask"]), f64(inp["latent_mask"]))
        o32, _ = uo.unet_forward(sd, cfg, inp["x"], inp["x0"], inp["t"].float(), inp["frame_indices"], inp["obs_mask"],
                                 inp["latent_mask"])
    e_hip = float((out.cpu().double() - t64).abs().max())
    e_cpu = float((o32.double() - t64).abs().max())
    print(f"[T={T} B={B} chain={chain}] error vs fp64: hip {e_hip:.3e}  cpu-oracle-fp32 {e_cpu:.3e}")
    assert e_hip < 3 * e_cpu + 2e-5


@pytest.mark.parametrize("deterministic", ["0", "1"])
def test_long_window_training_step(monkeypatch, deterministic):
    """One ``training_losses`` forward + backward at 40 frames: loss and every parameter gradient vs the oracle's
    autograd; in deterministic mode (with the in-place gradient delivery that TrainLoop uses) two runs give bitwise the
    same gradients."""
    monkeypatch.setenv("LFVDM_DETERMINISTIC", deterministic)
    from improved_diffusion import script_util as su
    cfg, sd = _small_model(ch=32, heads=2)
    B, T, H = 2, 40, 8
    inp = {k: torch.from_numpy(v) for k, v in recipe.make_inputs("tl/train", B, T, 4, H, H, n_pad=3).items()}
    model = build_native(cfg, sd).train()
    model.native_grad_accumulation = deterministic == "1"
    d = {k: v.cuda() for k, v in inp.items()}
    diff = su.create_gaussian_diffusion(steps=1000, rescale_timesteps=True, rescale_learned_sigmas=True)
    tab = do.Tables(do.linear_betas(1000))
    tt = torch.tensor([700, 120])
    noise = torch.from_numpy(recipe.gaussianish("tl/train/noise", inp["x"].numel()).reshape(inp["x"].shape).astype(np.float32))
    lat = 1.0 - inp["obs_mask"]
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    grads, losses = [], []
    for _ in range(2 if deterministic == "1" else 1):
        model.zero_grad(set_to_none=True)
        terms = diff.training_losses(model, d["x0"], tt.cuda(), model_kwargs=mk, noise=noise.cuda(), latent_mask=lat.cuda(),
                                     eval_mask=lat.cuda())
        terms["loss"].mean().backward()
        torch.cuda.synchronize()
        losses.append(terms["loss"].detach().cpu())
        grads.append({k: p.grad.detach().clone() for k, p in model.named_parameters()})
    sdo = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    f64 = lambda t: t.double() if t.is_floating_point() else t

    def oracle_eps(x_t, ts):
        return uo.unet_forward(sdo, cfg, x_t, f64(inp["x0"]), ts.double(), inp["frame_indices"], f64(inp["obs_mask"]),
                               f64(inp["latent_mask"]))[0]
    oterms = do.training_losses(tab, oracle_eps, f64(inp["x0"]), tt, noise.double(), lat.double(), lat.double())
    oterms["loss"].mean().backward()
    lerr = float((losses[0].double() - oterms["loss"].detach()).abs().max())
    assert lerr < 1e-4 * float(oterms["loss"].detach().abs().max()) + 1e-6, lerr
    gmax = max(float(v.grad.abs().max()) for v in sdo.values() if v.grad is not None)
    worst, worst_key = 0.0, None
    for k, g in grads[0].items():
        ref = sdo[k].grad
        assert ref is not None, k
        err = float((g.cpu().double() - ref).abs().max())
        if err > worst:
            worst, worst_key = err, k
    print(f"[T=40 training, deterministic={deterministic}] loss max|d| {lerr:.2e}, grad max|d| {worst:.2e} (max|g| {gmax:.2e})")
    assert worst < 2e-4 * gmax, (worst, worst_key, gmax)
    if deterministic == "1":
        assert torch.equal(losses[0], losses[1])
        for k in grads[0]:
            assert torch.equal(grads[0][k], grads[1][k]), k


@pytest.mark.parametrize("tables", ["1", "0", "budget"])
def test_long_window_sampler_follows_the_oracle(monkeypatch, tables):
    """``GraphSampler(inject_noise=True)`` at 40 frames over respaced steps (10-step respacing: the top three and the last
    two) follows the oracle's ``p_sample`` trajectory, with the timestep tables on, forced off, and refused by a pool
    too small for them (the _TableBudget fallback to per-step R networks)."""
    if tables == "budget":
        monkeypatch.setenv("LFVDM_TIME_TABLE_GB", "0.01")
    else:
        monkeypatch.setenv("LFVDM_TIME_TABLES", tables)
    from improved_diffusion.gaussian_diffusion import GraphSampler
    cfg, sd = _small_model(ch=32, heads=2)
    B, T, H = 2, 40, 8
    model = build_native(cfg, sd)
    diff = make_diffusion(1000, "10")
    tab = do.Tables(do.linear_betas(1000), do.space_timesteps(1000, "10"))
    inp = {k: torch.from_numpy(v) for k, v in recipe.make_inputs("tl/samp", B, T, 4, H, H, n_pad=3).items()}
    mk = dict(frame_indices=inp["frame_indices"].cuda(), obs_mask=inp["obs_mask"].cuda(), latent_mask=inp["latent_mask"].cuda(),
              x0=inp["x0"].cuda())
    shape = tuple(inp["x"].shape)
    s = GraphSampler(diff, model, shape, True, inject_noise=True)
    for leg, steps, x in (("top", (9, 8, 7), inp["x"].clone()), ("bottom", (1, 0), 0.5 * inp["x"] + 0.5 * inp["x0"])):
        s.begin(x.cuda(), mk)
        if tables == "1":
            assert s.plan.time_steps == 10, s.plan.time_table_fallback
        else:
            assert not s.plan.time_steps and s.plan.time_table_fallback
        cur = x.clone()
        for j, i in enumerate(steps):
            noise = torch.from_numpy(recipe.gaussianish(f"tl/samp/{leg}/noise{j}", inp["x"].numel()).reshape(shape).astype(np.float32))
            s.noise.copy_(noise.cuda())
            out = s.step(i)["sample"].cpu()
            t = torch.full((B,), i, dtype=torch.int64)
            eps, _ = uo.unet_forward(sd, cfg, cur, inp["x0"], do.model_timesteps(tab, t), inp["frame_indices"], inp["obs_mask"],
                                     inp["latent_mask"])
            want, _ = do.p_sample(tab, eps, cur, t, noise)
            err = float((out - want).abs().max())
            print(f"[T=40 sampler tables={tables}] {leg} step {j} (i={i}): max|d| {err:.2e}")
            assert err < 2e-4 * (j + 1), (leg, j, err)          # the per-step allowance of test_sampler_gpu's trajectories
            cur = out.clone()


def test_long_video_with_40_frame_windows():
    """``sample_video`` with max_frames = 40 and 4 respaced steps per window: finishes, visits exactly the windows of the
    sampling scheme, leaves the observed frames alone, finite output."""
    from improved_diffusion.video_sampler import sample_video, default_sampling_args
    cfg, sd = _small_model(ch=32, heads=2)
    model = build_native(cfg, sd).eval()
    diff = make_diffusion(1000, "4")
    scheme, T, n_obs, K, step = "autoreg", 90, 10, 40, 20
    g = torch.Generator().manual_seed(3)
    batch = torch.randn(1, T, 4, 8, 8, generator=g)
    args = default_sampling_args(sampling_scheme=scheme, n_obs=n_obs, max_frames=K, max_latent_frames=step, device="cuda")
    torch.manual_seed(7)
    samples, used = sample_video(args, model, diff, batch, verbose=False)
    want = run_scheme(scheme, T, n_obs, K, step)
    assert [[list(map(int, o[0])), list(map(int, l[0]))] for o, l in used] == want
    assert max(len(o) + len(l) for o, l in want) == K
    assert samples.shape == batch.shape and bool(torch.isfinite(samples).all())
    assert torch.equal(samples[:, :n_obs], batch[:, :n_obs])
    assert float(samples[:, n_obs:].std()) > 1e-3
