"""Known-region sampling on the MI355X: the blend and re-noise launches against their formulas in float64, the three noise
streams, the replayed step that ends with the blend, the chain's invariants, resampling and the long-video plumbing."""
import numpy as np
import pytest
import torch

from test_oracle_golden import load_case
from test_forward_gpu import build_native
from test_sampler_gpu import make_diffusion

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
# the issue's two shapes, one whose H*W is no multiple of 4 (the scalar mask path) and one of more than 1024 * 256 quads
# per row (the grid-stride walk)
OP_SHAPES = [(2, 3, 4, 4, 4), (1, 2, 4, 8, 4), (2, 2, 4, 3, 3), (1, 5, 4, 256, 256)]
SAMPLERS = [("ancestral", ("ancestral",)), ("ddim", ("ddim", 0.0)), ("dpm_solver", ("dpmpp2m",))]


def t_cases(B, n):
    """j = 0, a middle j and j = n - 1, per-sample different where there is more than one sample."""
    mid = n // 2
    return [[0, mid], [mid, n - 1], [n - 1, 0]] if B == 2 else [[0], [mid], [n - 1]]


def op_inputs(shape, seed):
    B, T, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x, known, eps = (torch.randn(shape, generator=g) for _ in range(3))
    mask = torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, (B, T, H, W), generator=g)]
    return x, known, eps, mask


def blend_check(diff, got, x, known, eps, mask, t):
    """Every element within 4 * 2^-23 * (|a known| + |s eps| + |x|) of the float64 formula; at j = 0 bitwise."""
    co = diff.known_region_coefficients()
    a = torch.from_numpy(co["a"][t]).view(-1, 1, 1, 1, 1)
    s = torch.from_numpy(co["s"][t]).view(-1, 1, 1, 1, 1)
    m = mask.double().unsqueeze(2)
    ak, se = a * known.double(), s * eps.double()
    want = m * (ak + se) + (1 - m) * x.double()
    bound = 4 * U * (ak.abs() + se.abs() + x.double().abs())
    err = (got.double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"shape {tuple(x.shape)} t {list(t)}: max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), worst
    m5 = mask.unsqueeze(2).expand_as(x)
    for b, j in enumerate(t):
        if j == 0:
            assert torch.equal(got[b][m5[b] == 1], known[b][m5[b] == 1]), "m = 1 at j = 0: the known video, bitwise"
        assert torch.equal(got[b][m5[b] == 0], x[b][m5[b] == 0]), "m = 0: untouched, bitwise"


@pytest.mark.parametrize("shape", OP_SHAPES)
@pytest.mark.parametrize("fixed", [False, True], ids=["fresh", "fixed"])
def test_blend_op(shape, fixed):
    from improved_diffusion import _native as nat
    diff = make_diffusion(1000, "")
    tb = diff.known_region_tables("cuda")
    x, known, eps, mask = op_inputs(shape, 7)
    seed = torch.tensor([20221201], dtype=torch.int64, device="cuda")
    for t in t_cases(shape[0], diff.num_timesteps):
        tt = torch.tensor(t, device="cuda")
        xs = x.cuda()
        noise_out = torch.full(shape, 123.0, device="cuda")
        if fixed:
            nat.known_blend(xs, known.cuda(), mask.cuda(), tt, tb["a"], tb["s"], eps=eps.cuda(), seed=seed, noise_out=noise_out)
            assert bool((noise_out == 123.0).all()), "fixed noise: noise_out is not written"
            used = eps
        else:
            nat.known_blend(xs, known.cuda(), mask.cuda(), tt, tb["a"], tb["s"], seed=seed, noise_out=noise_out)
            used = noise_out.cpu()
            assert bool(torch.isfinite(used).all()) and not bool((used == 123.0).any())
            # without noise_out: the same result
            xs2 = x.cuda()
            nat.known_blend(xs2, known.cuda(), mask.cuda(), tt, tb["a"], tb["s"], seed=seed)
            assert torch.equal(xs, xs2)
        blend_check(diff, xs.cpu(), x, known, used, mask, t)


@pytest.mark.parametrize("shape", OP_SHAPES)
def test_renoise_op(shape):
    """x = sqrt(1 - beta) x + sqrt(beta) eps: two products and a sum, within 4 * 2^-23 * (|c x| + |d eps|)."""
    from improved_diffusion import _native as nat
    diff = make_diffusion(1000, "")
    tb, co = diff.known_region_tables("cuda"), diff.known_region_coefficients()
    x = op_inputs(shape, 9)[0]
    seed = torch.tensor([5], dtype=torch.int64, device="cuda")
    for t in t_cases(shape[0], diff.num_timesteps):
        xs, noise_out = x.cuda(), torch.empty(shape, device="cuda")
        nat.renoise(xs, torch.tensor(t, device="cuda"), tb["sqrt_1mbeta"], tb["sqrt_beta"], seed, noise_out=noise_out)
        xs2 = x.cuda()
        nat.renoise(xs2, torch.tensor(t, device="cuda"), tb["sqrt_1mbeta"], tb["sqrt_beta"], seed)
        assert torch.equal(xs, xs2)
        cx = torch.from_numpy(co["sqrt_1mbeta"][t]).view(-1, 1, 1, 1, 1) * x.double()
        de = torch.from_numpy(co["sqrt_beta"][t]).view(-1, 1, 1, 1, 1) * noise_out.cpu().double()
        err, bound = (xs.cpu().double() - (cx + de)).abs(), 4 * U * (cx.abs() + de.abs())
        print(f"shape {shape} t {t}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all())


def test_noise_streams_are_disjoint():
    from improved_diffusion import _native as nat
    diff = make_diffusion(1000, "")
    shape = (1, 8, 4, 32, 32)
    n = int(np.prod(shape))
    assert n >= 32768
    tb = diff.known_region_tables("cuda")
    recip, recipm1, c1, c2, sg, R, M = diff._update_args(torch.device("cuda"))
    z = lambda: torch.zeros(shape, device="cuda")
    ones = torch.ones(shape[0], shape[1], shape[3], shape[4], device="cuda")

    def draws(seed, j):
        sd, t = torch.tensor([seed], dtype=torch.int64, device="cuda"), torch.tensor([j], device="cuda")
        up, bl, rn = z(), z(), z()
        nat.update_rng_x0(z(), z(), up, t, recip, recipm1, c1, c2, sg, R, M, True, z(), sd)
        nat.known_blend(z(), z(), ones, t, tb["a"], tb["s"], seed=sd, noise_out=bl)
        nat.renoise(z(), t, tb["sqrt_1mbeta"], tb["sqrt_beta"], sd, noise_out=rn)
        return [v.flatten().double().cpu() for v in (up, bl, rn)]
    up, bl, rn = draws(1234567, 500)
    bl2 = draws(1234567, 499)[1]
    for name, v in (("update", up), ("blend", bl), ("renoise", rn), ("blend, t - 1", bl2)):
        mean, var = float(v.mean()), float(v.var())
        print(f"{name}: mean {mean:+.4f} var {var:.4f}")
        assert abs(mean) < 5 / np.sqrt(n) and abs(var - 1) < 5 * np.sqrt(2 / n), name
    corr = lambda p, q: float(((p - p.mean()) * (q - q.mean())).mean() / (p.std() * q.std()))
    for name, p, q in (("update/blend", up, bl), ("update/renoise", up, rn), ("blend/renoise", bl, rn), ("blend t/t-1", bl, bl2)):
        c = corr(p, q)
        print(f"corr {name}: {c:+.4f}")
        assert abs(c) < 5 / np.sqrt(n), name
    again = draws(1234567, 500)
    assert all(torch.equal(p, q) for p, q in zip((up, bl, rn), again)), "the same (seed, t) reproduces bitwise"
    other = draws(1234568, 500)
    assert all(abs(corr(p, q)) < 5 / np.sqrt(n) for p, q in zip((up, bl, rn), other)), "another seed: another stream"


@pytest.fixture(scope="module")
def micro():
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd).eval()
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    shape = tuple(inp["x"].shape)
    B, T, _, H, W = shape
    g = torch.Generator().manual_seed(17)
    known = torch.randn(shape, generator=g).cuda()
    mask = torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, (B, T, H, W), generator=g)].cuda()
    return model, d, mk, shape, known, mask


@pytest.mark.parametrize("name,rule", SAMPLERS)
def test_replayed_step_ends_with_the_blend(micro, name, rule):
    """step(i) of the known-region sampler == the eager update fed the sampler's recorded update noise, then the float64
    blend with the recorded blend noise: within the replayed step's 2e-4 (tests/test_sampler_gpu.py) plus the op's bound."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    model, d, mk, shape, known, mask = micro
    diff = make_diffusion(1000, "10")
    fixed = name != "ancestral"
    plain = GraphSampler(diff, model, shape, True, rule=rule)
    s = GraphSampler(diff, model, shape, True, rule=rule)
    s.enable_known_region(fixed, record_noise=True)
    eps = torch.randn(shape, generator=torch.Generator().manual_seed(3)).cuda() if fixed else None
    s.begin(d["x"].clone(), mk, known=known, known_mask=mask, known_eps=eps)
    plain.begin(d["x"].clone(), mk)
    assert len(s.plan.steps) == len(plain.plan.steps) and s.extra_launches == plain.extra_launches + 1
    co = diff.known_region_coefficients()
    nt = diff.num_timesteps
    prev = None
    for i in (nt - 1, nt - 2):
        before = s.plan.x_in.clone()
        out = s.step(i)["sample"].clone()
        ti = torch.full((shape[0],), i, device="cuda", dtype=torch.long)
        with torch.no_grad():
            if name == "ancestral":
                ref = diff.p_sample(model, before, ti, clip_denoised=True, model_kwargs=mk, noise=s.noise.clone())
            elif name == "ddim":
                ref = diff.ddim_sample(model, before, ti, clip_denoised=True, model_kwargs=mk, eta=0.0)
            else:
                ref = diff.dpm_solver_sample(model, before, ti, clip_denoised=True, model_kwargs=mk, prev_pred_xstart=prev)
        prev = s.pred.clone()
        z = (eps if fixed else s.known_noise).double()
        m = mask.double().unsqueeze(2)
        ak, se, x = co["a"][i] * known.double(), co["s"][i] * z, ref["sample"].double()
        want = m * (ak + se) + (1 - m) * x
        tol = 2e-4 + 4 * U * (ak.abs() + se.abs() + x.abs())
        err = (out.double() - want).abs()
        print(f"{name} t={i}: max|d| {float(err.max()):.2e}")
        assert bool((err <= tol).all()), float((err - tol).max())
        assert not torch.allclose(out, ref["sample"], atol=1e-2), "the blend changed the state"


def plain_loop(diff, name, model, shape, mk):
    if name == "ancestral":
        return diff.p_sample_loop(model, shape, clip_denoised=True, model_kwargs=mk, return_decoded=False)[0]
    if name == "ddim":
        return diff.ddim_sample_loop(model, shape, clip_denoised=True, model_kwargs=mk, eta=0.0, return_decoded=False)
    return diff.dpm_solver_sample_loop(model, shape, clip_denoised=True, model_kwargs=mk, return_decoded=False)


@pytest.mark.parametrize("name,rule", SAMPLERS)
def test_chain_invariants(micro, monkeypatch, name, rule):
    model, d, mk, shape, known, mask = micro
    B, T, _, H, W = shape
    lat = d["latent_mask"]
    on = (lat > 0).expand(shape)
    assert bool(on.any()) and not bool(on.all())
    kr = lambda diff, kn, m: diff.known_region_sample_loop(model, shape, kn, m, sampler=name, clip_denoised=True, model_kwargs=mk,
                                                            latent_mask=lat, return_decoded=False)
    diff = make_diffusion(1000, "10")
    # an empty mask: bitwise the plain loop of the same seed (the seed is drawn once, the blend is a no-op at m = 0)
    torch.manual_seed(4)
    want = plain_loop(diff, name, model, shape, mk)
    torch.manual_seed(4)
    got = kr(diff, known, torch.zeros(B, T, H, W, device="cuda"))
    assert torch.equal(got, want)
    assert len(diff._samplers) == 1 and len(diff._known_samplers) == 1
    (ps,), (ks,) = diff._samplers.values(), diff._known_samplers.values()
    assert len(ks.plan.steps) + ks.extra_launches == len(ps.plan.steps) + ps.extra_launches + 1, "the blend is counted"
    # a full mask: known on the latent frames, bitwise; a second chain with other data on the SAME sampler and graphs
    graphs = (id(ks.graph), id(ks.graph_k))
    torch.manual_seed(5)
    full = kr(diff, known, torch.ones(1, 1, 1, 1, device="cuda"))
    assert torch.equal(full[on], known[on])
    torch.manual_seed(6)
    soft = kr(diff, -known, mask)
    assert list(diff._known_samplers.values()) == [ks] and (id(ks.graph), id(ks.graph_k)) == graphs
    one = (mask.unsqueeze(2) * lat).expand(shape) == 1
    assert torch.equal(soft[one], (-known)[one]) and bool(torch.isfinite(soft).all())
    fresh = make_diffusion(1000, "10")
    torch.manual_seed(6)
    assert torch.equal(kr(fresh, -known, mask), soft), "a cached sampler's second chain == a fresh sampler's first"
    # one step per graph launch == eight
    monkeypatch.setenv("LFVDM_STEPS_PER_GRAPH", "1")
    single = make_diffusion(1000, "10")
    torch.manual_seed(6)
    assert torch.equal(kr(single, -known, mask), soft)
    (s1,) = single._known_samplers.values()
    assert s1.K == 1 and ks.K > 1


@pytest.mark.parametrize("r", [2, 12])
def test_resampling(micro, monkeypatch, r):
    """r = 2 and an r above 9, where the repeat key's offset k * stride no longer fits 64 bits unreduced (RePaint's own r is
    10).  U-Net forwards are counted as replays of the sampler's captured graphs times the steps each holds: a replay of
    the single-step graph issues the plan's launches once, one of the K-step graph K times."""
    model, d, mk, shape, known, mask = micro
    lat = d["latent_mask"]
    on = (lat > 0).expand(shape)
    diff = make_diffusion(1000, "10")
    n = diff.num_timesteps
    replayed = []
    replay = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replayed.append(self), replay(self))[1])

    def forwards(s):
        """-> U-Net forwards since the last call, from the replays of s's graphs."""
        assert all(g is s.graph or g is s.graph_k for g in replayed)
        count = sum(1 if g is s.graph else s.K for g in replayed)
        replayed.clear()
        return count
    torch.manual_seed(8)
    out = diff.known_region_sample_loop(model, shape, known, torch.ones(1, 1, 1, 1, device="cuda"), resample_steps=r,
                                        model_kwargs=mk, latent_mask=lat, return_decoded=False)
    (s,) = diff._known_samplers.values()
    assert torch.equal(out[on], known[on]) and bool(torch.isfinite(out).all())
    assert s.graph_k is None, "resampling is driven over the single-step graph"
    got = forwards(s)
    print(f"r = {r}: {got} forwards, {got * len(s.plan.steps)} plan launches")
    assert got == r * (n - 1) + 1
    torch.manual_seed(8)
    soft = diff.known_region_sample_loop(model, shape, known, mask, resample_steps=r, model_kwargs=mk, latent_mask=lat,
                                         return_decoded=False)
    assert forwards(s) == r * (n - 1) + 1
    torch.manual_seed(8)
    again = diff.known_region_sample_loop(model, shape, known, mask, resample_steps=r, model_kwargs=mk, latent_mask=lat,
                                          return_decoded=False)
    replayed.clear()
    torch.manual_seed(8)
    once = diff.known_region_sample_loop(model, shape, known, mask, model_kwargs=mk, latent_mask=lat, return_decoded=False)
    assert forwards(s) == n, "without resampling: one forward per timestep"
    assert bool(torch.isfinite(soft).all()) and torch.equal(soft, again) and not torch.equal(soft, once)
    # the slow path counts the same forwards, through the module itself
    calls = []
    h = model.register_forward_hook(lambda *a: calls.append(1))
    try:
        slow = diff.known_region_sample_loop(model, shape, known, torch.ones(1, 1, 1, 1, device="cuda"), resample_steps=r,
                                             denoised_fn=lambda x: x, model_kwargs=mk, latent_mask=lat, return_decoded=False)
    finally:
        h.remove()
    assert len(calls) == r * (n - 1) + 1 and torch.equal(slow[on], known[on])


def test_sample_video_with_a_known_half(micro):
    from improved_diffusion.video_sampler import sample_video, default_sampling_args, window_inputs
    model = micro[0]
    diff = make_diffusion(1000, "ddim10")
    B, T, n_obs = 2, 10, 2
    g = torch.Generator().manual_seed(12)
    batch = torch.randn(B, T, 4, 16, 16, generator=g)
    known_video = torch.randn(B, T, 4, 16, 16, generator=g)
    known_mask = torch.zeros(B, T, 16, 16)
    known_mask[..., :8] = 1.0
    args = default_sampling_args(sampling_scheme="autoreg", n_obs=n_obs, max_frames=6, max_latent_frames=4, use_ddim=True,
                                 device="cuda")
    torch.manual_seed(31)
    out, used = sample_video(args, model, diff, batch, verbose=False, known_video=known_video, known_mask=known_mask)
    assert len(used) == 2
    assert torch.equal(out[:, :n_obs], batch[:, :n_obs]), "observed frames are unchanged"
    assert torch.equal(out[:, n_obs:, :, :, :8], known_video[:, n_obs:, :, :, :8]), "the known half, bitwise"
    assert bool(torch.isfinite(out).all()) and not torch.equal(out[:, n_obs:, :, :, 8:], known_video[:, n_obs:, :, :, 8:])
    # both arguments None: what sample_video did before they existed - each window one ddim_sample_loop, restated here
    torch.manual_seed(31)
    off, used_off = sample_video(args, model, diff, batch, verbose=False)
    torch.manual_seed(31)
    samples = torch.zeros_like(batch, device="cuda")
    samples[:, :n_obs] = batch[:, :n_obs].cuda()
    rows = torch.arange(B, device="cuda")[:, None]
    for obs_idx, lat_idx in used_off:
        fi, x0, om, lm = window_inputs(samples, obs_idx, lat_idx, torch.device("cuda"))
        local = diff.ddim_sample_loop(model, tuple(x0.shape), clip_denoised=True,
                                      model_kwargs=dict(frame_indices=fi, x0=x0, obs_mask=om, latent_mask=lm), eta=0.0,
                                      latent_mask=lm, return_decoded=False)
        nl = len(lat_idx[0])
        samples[rows, fi[:, -nl:]] = local[:, -nl:]
    assert used_off == used and torch.equal(off, samples.cpu())
    assert not torch.equal(off, out)
