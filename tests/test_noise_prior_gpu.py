"""Temporally correlated noise prior on the MI355X: lfvdm_noise_prior_factor against the float64 reference, both modes of
lfvdm_noise_prior_fill (mix mode against float64 ``L_ref @ xi``, draw mode against the counter-exact Philox reference on
stream 4), the refusals, the replayed sampler step under a prior, and training.  GPU only.

Bounds.  Factor: |L - L_ref| <= 2^-23 (entries are at most 1 in magnitude, the arithmetic is fp64, only the store rounds).
Mix: per element T * 2^-23 * sum_j |L_ij| |xi_j| (the rounding of L to fp32 and of at most T fmaf, each half an ulp of a
partial sum that never exceeds that sum of magnitudes).  Draw: the per-xi tolerance of tests/test_noise_exact_gpu.py
(TOL_UNITS units of 2^-23 max(1, m)) propagated through |L|, plus the mix bound."""
import functools

import numpy as np
import pytest
import torch

from oracle import philox_ref as pr
from improved_diffusion import noise_prior as npr
from test_oracle_golden import load_case
from test_forward_gpu import build_native
from test_noise_exact_gpu import UNIT, TOL_UNITS, S, SEEDS, check, seed_tensor

pytestmark = pytest.mark.gpu

PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
U = 2.0 ** -23
STREAM_PRIOR = 4


@pytest.fixture(scope="module")
def nat():
    from improved_diffusion import _native
    _native.lib()
    return _native


def make_diffusion(resp="4", **kw):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, rescale_timesteps=True, rescale_learned_sigmas=True,
                                        diffusion_space_kwargs=dict(PIXEL), **kw)


def shuffled(B, T, seed, scale=1, span=3):
    """(B, T) distinct frame indices per row out of span * T, in random order, times ``scale``"""
    rs = np.random.RandomState(seed)
    return np.stack([rs.permutation(span * T)[:T] for _ in range(B)]).astype(np.int64) * scale


def with_repeats(B, T, seed):
    f = shuffled(B, T, seed)
    f[:, 1] = f[:, 0]
    f[:, T // 2:] = f[:, :T - T // 2]      # the second half repeats the first
    return f


# ------------------------------------------------------------------------------------------------ the factor
FACTOR_CASES = {
    "T1-mixed": (np.array([[5], [0]]), "mixed:1"),
    "T2-progressive": (np.array([[3, 1], [1, 3]]), "progressive:2"),
    "T20-cov": (shuffled(2, 20, 1), "cov:0.2:0.5:0.9"),
    "T33-progressive": (shuffled(3, 33, 2), "progressive:2"),
    "T64-rho0.99": (shuffled(2, 64, 3), "cov:0.1:0.8:0.99"),
    "T64-mixed": (shuffled(1, 64, 4), "mixed:2"),
    "T20-repeats-singular": (with_repeats(2, 20, 5), "cov:0.25:0.75:0.5"),
    "T20-repeats-progressive": (with_repeats(2, 20, 6), "progressive:2"),
    "T20-repeats-independent-part": (with_repeats(2, 20, 7), "cov:0.2:0.5:0.9"),
    "T20-gaps-1e6": (shuffled(2, 20, 8, scale=10 ** 6), "progressive:2"),
    "T33-gaps-1e6-rho0.99": (shuffled(2, 33, 9, scale=10 ** 6), "cov:0.3:0.6:0.99"),
    "T20-sorted-consecutive": (np.arange(20)[None], "progressive:2"),
}


@pytest.mark.parametrize("case", list(FACTOR_CASES))
def test_factor_against_float64(nat, case):
    f, spec = FACTOR_CASES[case]
    prior = npr.parse_noise_prior(spec)
    B, T = f.shape
    L = torch.full((B, T, T), float("nan"), device="cuda")
    nat.noise_prior_factor(torch.from_numpy(f).cuda(), *prior, out=L)
    torch.cuda.synchronize()
    got = L.cpu().numpy()
    ref = npr.noise_prior_factor_ref(f, *prior)
    assert np.all(np.isfinite(got))
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"[noise prior factor] {case}: max |L - L_ref| = {err:.3e} (bound {U:.3e})")
    assert err <= U
    upper = np.triu(np.ones((T, T), dtype=bool), 1)
    assert np.array_equal(got[:, upper].view(np.uint32), np.zeros_like(got[:, upper], dtype=np.uint32)), "upper triangle: +0 bitwise"
    if "repeats" in case and "independent" not in case:
        half = T - T // 2
        # a repeated frame has its twin's row - up to the fp64 residue (1e-16) that the frames between the two leave in the
        # twin's later columns - and a column that is exactly zero (the pivot rule)
        assert np.abs(got[:, T // 2:].astype(np.float64) - got[:, :half]).max() <= 1e-12
        assert not np.any(got[:, :, T // 2:]), "a twin's column is zero"


# ------------------------------------------------------------------------------------------------ fill, mix mode
TILE, GRID_CAP = 32, 1024      # csrc/noise_prior.hip: elements per workgroup tile, workgroups per sample
MIX_SHAPES = [(2, 20, 4, 8, 8), (1, 64, 4, 2, 2), (3, 33, 3, 4, 4), (2, 1, 4, 4, 4),
              (1, 3, 1, 1, TILE * GRID_CAP + 40),      # 1026 tiles: a second pass of two workgroups, the last tile 8 wide
              (2, 5, 3, 5, 5)]                         # E = 75: no multiple of 4 - the scalar instance, a ragged tile


@functools.lru_cache(maxsize=None)
def mix_case(shape):
    """-> (f, prior, L on the device, L_ref float64, xi on the device, the float64 product and its bound), once per shape"""
    from improved_diffusion import _native as nat
    B, T = shape[:2]
    prior = npr.parse_noise_prior("cov:0.2:0.6:0.9")
    f = shuffled(B, T, sum(shape))
    L = nat.noise_prior_factor(torch.from_numpy(f).cuda(), *prior)
    ref = npr.noise_prior_factor_ref(f, *prior)
    xi = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)))
    x64 = xi.reshape(B, T, -1).double().numpy()
    want = np.einsum("bij,bje->bie", ref, x64)
    bound = T * U * np.einsum("bij,bje->bie", np.abs(ref), np.abs(x64))
    return f, prior, L, ref, xi.cuda(), want, bound


@pytest.mark.parametrize("shape", MIX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mix_against_float64(nat, shape):
    _, _, L, _, xi, want, bound = mix_case(shape)
    B, T = shape[:2]
    out = torch.full(shape, float("nan"), device="cuda")
    nat.noise_prior_fill(L, out, xi=xi)
    again = torch.full(shape, float("nan"), device="cuda")
    nat.noise_prior_fill(L, again, xi=xi)
    inplace = xi.clone()
    nat.noise_prior_fill(L, inplace, xi=inplace)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(B, T, -1).astype(np.float64)
    assert np.all(np.isfinite(got))
    ratio = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    print(f"[noise prior mix] {shape}: largest error / bound = {ratio:.3f}")
    assert np.all(np.abs(got - want) <= bound)
    assert torch.equal(again, out), "two launches agree bitwise"
    assert torch.equal(inplace, out), "in place equals out of place bitwise"
    eye = torch.eye(T, device="cuda").repeat(B, 1, 1)
    ident = torch.full(shape, float("nan"), device="cuda")
    nat.noise_prior_fill(eye, ident, xi=xi)
    assert torch.equal(ident, xi), "L = I returns xi bitwise"
    # the sum of an element does not depend on where its tile lies in the launch: the first 64 elements of every frame as a
    # launch of their own
    E = int(np.prod(shape[2:]))
    if E > 64:
        part = xi.reshape(B, T, E)[:, :, :64].contiguous()
        small = torch.empty_like(part)
        nat.noise_prior_fill(L, small, xi=part)
        assert torch.equal(small, out.reshape(B, T, E)[:, :, :64])


def test_apply_noise_prior_takes_the_native_launches(nat):
    shape = MIX_SHAPES[0]
    f, prior, L, _, xi, want, bound = mix_case(shape)
    got = npr.apply_noise_prior(xi, torch.from_numpy(f).cuda(), prior)
    ref = torch.empty_like(xi)
    nat.noise_prior_fill(L, ref, xi=xi)
    assert got.data_ptr() != xi.data_ptr() and torch.equal(got, ref)
    cpu = npr.apply_noise_prior(xi.cpu(), torch.from_numpy(f), prior)      # the float64 torch path, rounded to fp32
    assert np.all(np.abs(cpu.double().numpy().reshape(want.shape) - want) <= bound)
    assert np.all(np.abs(got.cpu().double().numpy().reshape(want.shape) - want) <= bound)
    # float indices and an (B, T, 1, 1, 1) layout are taken as they come in model_kwargs
    assert torch.equal(npr.apply_noise_prior(xi, torch.from_numpy(f).cuda().float().view(shape[0], shape[1], 1, 1, 1), prior), ref)


# ------------------------------------------------------------------------------------------------ fill, draw mode
DRAW_T = [500, 3, 999]      # t != row index
DRAW_SHAPES = [(3, 5, 100), (1, 3, TILE * GRID_CAP + 40)]


def draw(nat, L, seed, t, shape):
    out = torch.full(shape, float("nan"), device="cuda")
    nat.noise_prior_fill(L, out, seed=seed_tensor(seed), t=torch.tensor(t, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("seed", [S, SEEDS[1], SEEDS[-1]])
@pytest.mark.parametrize("shape", DRAW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_draw_with_identity_is_the_stream_4_row_noise(nat, shape, seed):
    B, T, E = shape
    t = DRAW_T[:B]
    eye = torch.eye(T, device="cuda").repeat(B, 1, 1)
    got = draw(nat, eye, seed, t, shape)
    z, m = pr.row_stream_noise(seed, STREAM_PRIOR, t, T * E)
    check(f"noise_prior_fill draw {shape} seed {seed:#x}", got.view(B, T * E), (z, m))


def test_draw_stream_and_key(nat):
    shape = DRAW_SHAPES[0]
    B, T, E = shape
    eye = torch.eye(T, device="cuda").repeat(B, 1, 1)
    got = draw(nat, eye, S, DRAW_T, shape).view(B, T * E).cpu().numpy().astype(np.float64)
    for stream in (0, 1, 2):
        z, _ = pr.row_stream_noise(S, stream, DRAW_T, T * E)
        assert np.mean(np.abs(got - z) < 1e-3) < 0.01, f"stream 4 differs from stream {stream} at the same key"
    for other in (S + 2 ** 32, ((S & 0xFFFFFFFF) << 32) | (S >> 32)):      # both key words count
        assert np.mean(draw(nat, eye, other, DRAW_T, shape).view(B, T * E).cpu().numpy() == got) < 1e-3
    rows = draw(nat, eye, S, [DRAW_T[1], DRAW_T[0], DRAW_T[2]], shape).view(B, T * E).cpu().numpy()
    assert np.mean(rows[0] == got[1]) < 1e-3, "the batch row is a counter word of its own"


@pytest.mark.parametrize("shape", DRAW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_draw_with_a_factor(nat, shape):
    B, T, E = shape
    t = DRAW_T[:B]
    prior = npr.parse_noise_prior("cov:0.2:0.6:0.9")
    f = shuffled(B, T, 31)
    L = nat.noise_prior_factor(torch.from_numpy(f).cuda(), *prior)
    ref = npr.noise_prior_factor_ref(f, *prior)
    got = draw(nat, L, S, t, shape)
    z, m = pr.row_stream_noise(S, STREAM_PRIOR, t, T * E)
    z, m = z.reshape(B, T, E), m.reshape(B, T, E)
    want = np.einsum("bij,bje->bie", ref, z)
    absL = np.abs(ref)
    bound = (np.einsum("bij,bje->bie", absL, TOL_UNITS * UNIT * np.maximum(1.0, m))
             + T * U * np.einsum("bij,bje->bie", absL, np.abs(z)))
    g = got.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(g))
    print(f"[noise prior draw] {shape}: largest error / bound = {float((np.abs(g - want) / bound).max()):.3f}")
    assert np.all(np.abs(g - want) <= bound)
    # the draw is the mix of its own xi: the same bytes as mix mode over the L = I draw
    xi = draw(nat, torch.eye(T, device="cuda").repeat(B, 1, 1), S, t, shape)
    mixed = torch.empty_like(xi)
    nat.noise_prior_fill(L, mixed, xi=xi)
    assert torch.equal(mixed, got)
    assert torch.equal(draw(nat, L, S, t, shape), got), "two launches agree bitwise"


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_out_unwritten(nat):
    lib = nat.lib()
    st = nat.stream()
    seed, t = seed_tensor(S), torch.zeros(2, dtype=torch.int64, device="cuda")
    L = torch.eye(65, device="cuda").repeat(2, 1, 1)
    out = torch.full((2, 65, 16), float("nan"), device="cuda")
    xi = torch.ones(2, 65, 16, device="cuda")
    fi = torch.zeros(2, 65, dtype=torch.int64, device="cuda")
    p = lambda v: v.data_ptr()      # noqa: E731
    assert lib.lfvdm_noise_prior_fill(p(L), p(xi), None, None, p(out), 2, 65, 16, st) == 1, "T = 65, mix mode"
    assert lib.lfvdm_noise_prior_fill(p(L), None, p(seed), p(t), p(out), 2, 65, 16, st) == 1, "T = 65, draw mode"
    assert lib.lfvdm_noise_prior_fill(p(L), None, p(seed), p(t), p(out), 2, 4, 6, st) == 1, "E % 4 != 0, draw mode"
    assert lib.lfvdm_noise_prior_fill(p(L), None, None, p(t), p(out), 2, 4, 8, st) == 1, "draw mode without a seed"
    assert lib.lfvdm_noise_prior_fill(p(L), p(xi), None, None, p(out), 2, 0, 8, st) == 1
    Lout = torch.full((2, 65, 65), float("nan"), device="cuda")
    assert lib.lfvdm_noise_prior_factor(p(fi), 0.0, 1.0, 0.5, p(Lout), 2, 65, st) == 1
    assert lib.lfvdm_noise_prior_factor(p(fi), 0.5, 0.6, 0.5, p(Lout), 2, 4, st) == 1
    assert lib.lfvdm_noise_prior_factor(p(fi), 0.0, 1.0, 1.0, p(Lout), 2, 4, st) == 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(Lout).all())
    with pytest.raises(RuntimeError, match="invalid shape"):
        nat.noise_prior_fill(L, out, xi=xi)
    # the same buffers, accepted: T = 4, E = 8
    assert lib.lfvdm_noise_prior_fill(p(L), None, p(seed), p(t), p(out), 2, 4, 8, st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.view(-1)[:64]).all()) and bool(torch.isnan(out.view(-1)[64:]).all())


# ------------------------------------------------------------------------------------------------ the sampler
@functools.lru_cache(maxsize=None)
def micro():
    """The micro model of tests/golden/forward_micro.npz with shuffled, widely spaced frame indices."""
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd).eval()
    d = {k: v.cuda() for k, v in inp.items()}
    B, T = inp["x"].shape[:2]
    fi = torch.from_numpy(shuffled(B, T, 41, span=9)).to(device="cuda", dtype=d["frame_indices"].dtype)
    mk = dict(frame_indices=fi.view(d["frame_indices"].shape), obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    return model, d, mk, tuple(inp["x"].shape)


def test_ancestral_chain_is_the_manual_chain_bitwise(nat, monkeypatch):
    """Four replayed ancestral steps under progressive:2.  After each: the sampler's noise is lfvdm_noise_prior_fill's draw
    under the chain's seed at the step's timestep, within the draw bound of L_ref xi_ref; sample and pred_xstart are
    lfvdm_update_x0 of the state the step started from, the network output it saw and that noise - bit for bit.

    Launches: the step is today's un-fused step (LFVDM_FUSED_HEAD=0: clock + forward with a head conv of its own + update)
    plus the fill - the count of the un-fused branch that draws with ``normal_()`` and then updates."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    model, d, mk, shape = micro()
    B, T = shape[:2]
    inner = int(np.prod(shape[1:]))
    diff = make_diffusion()
    diff.set_noise_prior("progressive:2")
    prior = diff.noise_prior
    fi = mk["frame_indices"].reshape(B, T).to(torch.int64)
    L = nat.noise_prior_factor(fi, *prior)
    ref = npr.noise_prior_factor_ref(fi.cpu().numpy(), *prior)
    absL = np.abs(ref)
    torch.manual_seed(21)
    s = GraphSampler(diff, model, shape, True)
    s.begin(d["x"].clone(), mk)
    assert s.prior == prior and torch.equal(s.prior_L, L) and not s.plan.head_fused
    recip, recipm1, c1, c2, sg, R, M = diff._update_args(torch.device("cuda"))
    for i in range(diff.num_timesteps - 1, -1, -1):
        before = s.plan.x_in.clone()
        out = s.step(i)
        torch.cuda.synchronize()
        t = torch.full((B,), i, dtype=torch.int64, device="cuda")
        noise = torch.empty(shape, device="cuda")
        nat.noise_prior_fill(L, noise, seed=s.seed, t=t)
        assert torch.equal(s.noise, noise), i
        sample, pred = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
        nat.update_x0(before, s.plan.out, noise, t, recip, recipm1, c1, c2, sg, R, M, True, sample, pred)
        assert torch.equal(out["sample"], sample) and torch.equal(out["pred_xstart"], pred), i
        z, m = pr.row_stream_noise(int(s.seed), STREAM_PRIOR, [i] * B, inner)
        z, m = z.reshape(B, T, -1), m.reshape(B, T, -1)
        want = np.einsum("bij,bje->bie", ref, z)
        bound = (np.einsum("bij,bje->bie", absL, TOL_UNITS * UNIT * np.maximum(1.0, m))
                 + T * U * np.einsum("bij,bje->bie", absL, np.abs(z)))
        assert np.all(np.abs(s.noise.cpu().numpy().reshape(want.shape).astype(np.float64) - want) <= bound), i
    assert int(s.seed) >> 32, "the chain's key comes from random_(): 63 bits"
    launches = len(s.plan.steps) + s.extra_launches
    monkeypatch.setenv("LFVDM_FUSED_HEAD", "0")
    plain = GraphSampler(make_diffusion(), model, shape, True)
    plain.begin(d["x"].clone(), mk)
    assert not plain.plan.head_fused and plain.prior is None
    assert len(s.plan.steps) == len(plain.plan.steps) and launches == len(plain.plan.steps) + plain.extra_launches + 1


def test_chain_with_dynamic_thresholding_and_with_torch_noise(monkeypatch):
    model, d, mk, shape = micro()
    diff = make_diffusion()
    diff.set_noise_prior("progressive:2")
    diff.set_dynamic_threshold(0.995)
    torch.manual_seed(3)
    outs = [o["sample"] for o in diff.p_sample_loop_progressive(model, shape, clip_denoised=True, model_kwargs=mk)]
    assert len(outs) == 4 and all(bool(torch.isfinite(o).all()) for o in outs)
    (s,) = diff._samplers.values()
    assert s.prior == diff.noise_prior and s.threshold == (0.995, None)
    # LFVDM_SAMPLER_NOISE=torch: torch's draw, mixed in place (read when the step is captured: a fresh diffusion object)
    monkeypatch.setenv("LFVDM_SAMPLER_NOISE", "torch")
    other = make_diffusion()
    other.set_noise_prior("progressive:2")
    torch.manual_seed(3)
    outs = [o["sample"] for o in other.p_sample_loop_progressive(model, shape, clip_denoised=True, model_kwargs=mk)]
    assert len(outs) == 4 and all(bool(torch.isfinite(o).all()) for o in outs)
    (st,) = other._samplers.values()
    assert st.extra_launches == s.extra_launches - 4 + 1, "the torch draw is one more launch, the threshold four fewer"


def test_deterministic_ddim_carries_the_prior_in_x_T_alone():
    model, d, mk, shape = micro()
    plain, prior = make_diffusion(), make_diffusion()
    prior.set_noise_prior("progressive:2")
    run = lambda df, noise: df.ddim_sample_loop(model, shape, noise=noise, clip_denoised=True, model_kwargs=mk, eta=0.0,      # noqa: E731
                                                return_decoded=False)
    x_T = d["x"].clone()
    assert torch.equal(run(plain, x_T.clone()), run(prior, x_T.clone())), "the same explicit noise: bitwise the same chain"
    (sp,), (sq,) = plain._samplers.values(), prior._samplers.values()
    assert sq.prior is not None and sp.prior is None
    assert len(sp.plan.steps) + sp.extra_launches == len(sq.plan.steps) + sq.extra_launches, "nothing extra per step"
    torch.manual_seed(8)
    drawn = run(prior, None)
    torch.manual_seed(8)
    start = npr.apply_noise_prior(torch.randn(*shape, device="cuda"), mk["frame_indices"], "progressive:2")
    assert torch.equal(drawn, run(plain, start)), "noise=None: x_T is L randn under torch's generator"
    torch.manual_seed(8)
    assert not torch.equal(drawn, run(plain, None))


def test_prior_unset_is_the_chain_of_a_diffusion_that_never_had_one():
    model, d, mk, shape = micro()
    never, unset = make_diffusion(), make_diffusion()
    unset.set_noise_prior("mixed:1")
    unset.set_noise_prior(None)
    chains = []
    for df in (never, unset):
        torch.manual_seed(13)
        chains.append([o["sample"].clone() for o in df.p_sample_loop_progressive(model, shape, clip_denoised=True, model_kwargs=mk)])
    assert all(torch.equal(a, b) for a, b in zip(*chains))
    (sa,), (sb,) = never._samplers.values(), unset._samplers.values()
    assert list(never._samplers) == list(unset._samplers) and sb.prior is None and sb.prior_L is None
    assert (sa.plan.head_fused, sa.extra_launches, len(sa.plan.steps)) == (sb.plan.head_fused, sb.extra_launches, len(sb.plan.steps))


def test_known_region_and_bpd_refuse_on_the_device():
    model, d, mk, shape = micro()
    diff = make_diffusion()
    diff.set_noise_prior("mixed:1")
    with pytest.raises(NotImplementedError, match="noise prior"):
        diff.known_region_sample_loop(model, shape, d["x"], torch.ones(1, 1, 1, 1, device="cuda"), model_kwargs=mk,
                                      return_decoded=False)
    with pytest.raises(NotImplementedError, match="noise prior"):
        diff.calc_bpd_loop(model, d["x"], model_kwargs=mk)
    assert not diff._known_samplers and not diff._bpd_evals


# ------------------------------------------------------------------------------------------------ training
def test_training_losses_draw_under_the_prior(monkeypatch):
    monkeypatch.setenv("LFVDM_DETERMINISTIC", "1")
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd).train()
    _, d, mk, shape = micro()
    diff = make_diffusion(resp="")
    diff.set_noise_prior("mixed:1")
    t = torch.tensor([700, 120], device="cuda")[:shape[0]]
    lat = 1.0 - d["obs_mask"]
    torch.manual_seed(5)
    drawn = diff.training_losses(model, d["x0"], t, model_kwargs=mk, latent_mask=lat, eval_mask=lat)
    torch.manual_seed(5)
    noise = npr.apply_noise_prior(torch.randn_like(d["x0"]), mk["frame_indices"], "mixed:1")
    given = diff.training_losses(model, d["x0"], t, model_kwargs=mk, noise=noise, latent_mask=lat, eval_mask=lat)
    off = make_diffusion(resp="")
    torch.manual_seed(5)
    plain = off.training_losses(model, d["x0"], t, model_kwargs=mk, latent_mask=lat, eval_mask=lat)
    for k in ("mse", "eval-mse", "loss"):
        assert bool(torch.isfinite(drawn[k]).all()) and torch.equal(drawn[k], given[k]), k
    assert not torch.equal(drawn["loss"], plain["loss"])


def test_train_loop_step_under_a_prior_runs_in_the_captured_graph(monkeypatch):
    from test_loss_weighting_gpu import _device_loop
    monkeypatch.delenv("LFVDM_LOSS_WEIGHTING", raising=False)
    monkeypatch.delenv("LFVDM_NOISE_PRIOR", raising=False)
    monkeypatch.setenv("LFVDM_TRAIN_GRAPH", "1")
    cfg, sd, _ = load_case("micro")
    loop = _device_loop(cfg, sd, noise_prior="mixed:1")
    assert loop.noise_prior == "cov:0.5:0.0:0.0" and loop.diffusion.noise_prior == (0.5, 0.0, 0.0)
    assert loop._checkpoint_config()["noise_prior"] == "cov:0.5:0.0:0.0"
    seen = []
    inner = loop._graphed_micro_step

    def recording(*a, **k):
        weighted, raw = inner(*a, **k)
        torch.cuda.synchronize()
        seen.append((raw.clone(), loop._graph_state.get("graph") is not None))
        return weighted, raw
    monkeypatch.setattr(loop, "_graphed_micro_step", recording)
    torch.manual_seed(1); np.random.seed(1)
    for _ in range(4):
        loop.forward_backward()
        loop.optimize_normal()
        loop.step += 1
    loop._flush_loss_log()
    torch.cuda.synchronize()
    assert [r for _, r in seen] == [False, False, True, True]
    assert all(bool(torch.isfinite(raw).all()) and float(raw.min()) > 0 for raw, _ in seen)
    assert not torch.equal(seen[2][0], seen[3][0]), "a replay draws fresh noise"
    assert bool(torch.isfinite(loop.arena.p).all())
