"""Search for optimised conditioning frames on the MI355X: the three launches of csrc/schedule_search.hip against numpy /
fp64 restatements, and the native backend of ``find_optimal_schedule`` against the eager composition of the public API
(micro model of the forward tests, V = 2 videos of 10 frames, windows of K = 6, 3 timesteps).  GPU only.

Measured on the MI355X (the scores of all 77 candidates of the walk below, native against eager, same seed): largest
relative deviation 4.83e-7 with 1 candidate per pass and 3.88e-7 with 4.  The assertion stands at ten times the larger
value, 4.83e-6 (the ceiling is 1e-4)."""
import numpy as np
import pytest
import torch

from oracle import recipe, unet_oracle as uo
from improved_diffusion import _native as nat, optimal_schedule as osch, script_util as su
from improved_diffusion.sampling_schemes import sampling_schemes
from improved_diffusion.video_sampler import default_sampling_args, sample_video

pytestmark = pytest.mark.gpu

V, T_VIDEO, N_OBS, K, STEP, N_T, SEED = 2, 10, 3, 6, 2, 3, 11
SCORE_RTOL = 4.83e-6       # ten times the measured deviation (module docstring); never looser than 1e-4
assert SCORE_RTOL <= 1e-4


def make_scheme(path=None):
    return sampling_schemes["autoreg"](video_length=T_VIDEO, num_obs=N_OBS, max_frames=K, step_size=STEP,
                                       optimal_schedule_path=path)


@pytest.fixture(scope="module")
def setup():
    from test_forward_gpu import build_native
    cfg = uo.make_cfg(model_channels=32, channel_mult=(1, 2), attention_resolutions=(1, 2))
    sd = {k: torch.from_numpy(v) for k, v in recipe.fill_state_dict(uo.param_shapes(cfg)).items()}
    model = build_native(cfg, sd)
    diffusion = su.create_gaussian_diffusion(steps=1000, rescale_timesteps=True)
    g = torch.Generator().manual_seed(3)
    base = torch.randn(V, 1, 4, 16, 16, generator=g)
    videos = ((base + 0.15 * torch.randn(V, T_VIDEO, 4, 16, 16, generator=g).cumsum(1)) * 0.5).cuda()
    return model, diffusion, videos


def run(setup, backend, group=None, seed=SEED):
    model, diffusion, videos = setup
    scheme = make_scheme()
    scorer = osch.make_scorer(model, diffusion, videos, scheme, n_timesteps=N_T, seed=seed, group=group, backend=backend)
    return osch.greedy_schedule(scheme, scorer), scorer


@pytest.fixture(scope="module")
def eager(setup):
    """The eager composition, once: {(s, chosen-so-far as candidates list) -> scores} through its rounds."""
    return run(setup, "eager")


def tables(diffusion):
    tb = diffusion.tables(torch.device("cuda"))
    return tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"]


# ------------------------------------------------------------------------------------------------ window assembly
@pytest.mark.parametrize("chw", [(4, 8, 8), (3, 6, 6)])
@pytest.mark.parametrize("vg", [(1, 1), (2, 4)])
def test_assemble_against_numpy_gather(chw, vg):
    Vn, G = vg
    W, Tv = Vn * G, 10
    rng = np.random.RandomState(7)
    pool = rng.standard_normal((Vn, Tv) + chw).astype(np.float32)
    table = np.full((W, K), -1, dtype=np.int32)
    role = np.zeros((W, K), dtype=np.int32)
    for g in range(G):
        # candidate g: frames 0, 1 observed in every window (the same video frame in several batch elements), one more
        # observed frame per candidate, two latents, the rest padding; candidate 0 keeps two padding slots
        frames, roles = osch.window_slots([7, 8], [0, 1] + ([2 + g] if g else []), K)
        table[g * Vn:(g + 1) * Vn], role[g * Vn:(g + 1) * Vn] = frames, roles
    assert (table[0] < 0).sum() == 2
    d = lambda a: torch.from_numpy(a).cuda()
    x0, xs = torch.full((W, K) + chw, 9.0).cuda(), torch.full((W, K) + chw, 9.0).cuda()
    obs, lat, mask = (torch.full((W * K,), 9.0).cuda() for _ in range(3))
    fi = torch.full((W, K), 9, dtype=torch.int64).cuda()
    nat.search_assemble(d(pool), d(table), d(role), x0, xs, obs, lat, mask, fi)
    torch.cuda.synchronize()
    ref = np.zeros((W, K) + chw, dtype=np.float32)
    for w in range(W):
        for k in range(K):
            if table[w, k] >= 0:
                ref[w, k] = pool[w % Vn, table[w, k]]
    assert np.array_equal(x0.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(xs.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(obs.cpu().numpy().reshape(W, K), (role == nat.SLOT_OBS).astype(np.float32))
    assert np.array_equal(lat.cpu().numpy().reshape(W, K), (role == nat.SLOT_LATENT).astype(np.float32))
    assert np.array_equal(mask.cpu().numpy().reshape(W, K), (role != nat.SLOT_PAD).astype(np.float32))
    assert np.array_equal(fi.cpu().numpy(), np.maximum(table, 0).astype(np.int64))


# ------------------------------------------------------------------------------------------------ noise and q_sample
def launch_head(diffusion, x_start, table, t_list, j, seed, step, Vn):
    sa, sb = tables(diffusion)
    W = table.shape[0]
    noise, x_t = torch.full_like(x_start, 7.0), torch.full_like(x_start, 7.0)
    t_buf = torch.full((W,), -5, dtype=torch.int64, device="cuda")
    ctl = torch.tensor([j, 0, len(t_list), 0], dtype=torch.int32, device="cuda")
    key = torch.tensor([seed, step], dtype=torch.int64, device="cuda")
    tl = torch.tensor(t_list, dtype=torch.int64, device="cuda")
    nat.search_noise_qsample(x_start, table, tl, ctl, key, sa, sb, noise, x_t, t_buf, Vn)
    torch.cuda.synchronize()
    return noise, x_t, t_buf, ctl


def test_noise_and_q_sample(setup):
    _, diffusion, _ = setup
    sa, sb = tables(diffusion)
    Vn, G, chw = 2, 2, (4, 8, 8)
    W = Vn * G
    # video 0 shows frame 5 in slot 0 of window 0 and in slot 2 of window 2; video 1 likewise in windows 1 and 3
    table_np = np.array([[5, 1, 2, 7, 8, -1]] * Vn + [[0, 1, 5, 7, 8, -1]] * Vn, dtype=np.int32)
    table = torch.from_numpy(table_np).cuda()
    x_start = torch.randn((W, K) + chw, generator=torch.Generator().manual_seed(1)).cuda()
    x_start[:, 5] = 0
    t_list = [999, 400, 0]
    outs = [launch_head(diffusion, x_start, table, t_list, j, SEED, 2, Vn) for j in range(3)]
    for j, (noise, x_t, t_buf, ctl) in enumerate(outs):
        t = t_list[j]
        assert t_buf.tolist() == [t + 1] * W, "the plan's clock pre-decrements: it is handed t + 1"
        assert ctl.tolist() == [j + 1, 0, 3, 0], "the position advances once per launch, the ticket is back at zero"
        a, b = float(sa[t]), float(sb[t])
        xs64, z64, xt64 = x_start.cpu().double(), noise.cpu().double(), x_t.cpu().double()
        err = (xt64 - (a * xs64 + b * z64)).abs()
        bound = 2.0 * 2.0 ** -23 * ((a * xs64).abs() + (b * z64).abs())
        assert bool((err <= bound).all()), float((err - bound).max())
        assert bool((noise[:, 5] == 0).all()) and bool((x_t[:, 5] == 0).all()), "padding slots are zero"
        # one (video, frame, j): the same bits in another slot and another batch element
        for v in range(Vn):
            assert torch.equal(noise[v, 0], noise[Vn + v, 2]), "frame 5"
            for k in (1, 3, 4):
                assert torch.equal(noise[v, k], noise[Vn + v, k])
        assert not torch.equal(noise[0, 0], noise[1, 0]), "another video"
        assert not torch.equal(noise[0, 0], noise[0, 1]), "another frame"
        # the eager backend's fill is the same stream
        fill = torch.empty_like(noise)
        nat.search_noise_fill(table, SEED, 2, j, fill, Vn)
        assert torch.equal(fill, noise)
    assert not torch.equal(outs[0][0], outs[1][0]), "another timestep position"
    other_step = launch_head(diffusion, x_start, table, t_list, 0, SEED, 3, Vn)[0]
    other_seed = launch_head(diffusion, x_start, table, t_list, 0, SEED + 1, 2, Vn)[0]
    assert not torch.equal(outs[0][0][:, :5], other_step[:, :5]) and not torch.equal(outs[0][0][:, :5], other_seed[:, :5])
    for other in (outs[1][0], other_step, other_seed):      # not merely different somewhere: unrelated draws
        c = np.corrcoef(outs[0][0][:, :5].flatten().cpu().numpy(), other[:, :5].flatten().cpu().numpy())[0, 1]
        assert abs(c) < 4 / np.sqrt(outs[0][0][:, :5].numel())


def test_noise_moments():
    Vn, Kn, chw = 8, 10, (4, 16, 16)
    table = torch.arange(Kn, dtype=torch.int32).repeat(Vn, 1).cuda()         # 80 distinct (video, frame) pairs
    noise = torch.empty((Vn, Kn) + chw, device="cuda")
    nat.search_noise_fill(table, 12345, 1, 0, noise, Vn)
    z = noise.flatten().cpu().double().numpy()
    n = z.size
    assert n >= 2 ** 16
    assert abs(z.mean()) <= 4 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1) <= 4 * np.sqrt(2 / n), z.var()


# ------------------------------------------------------------------------------------------------ score reduction
def test_score_reduction_against_fp64():
    G, n = 4, 1000
    rng = np.random.RandomState(5)
    terms = (rng.standard_normal((G * V, n)) ** 2).astype(np.float32)
    t_list = [999, 500, 0]
    scores = torch.empty(G, device="cuda")
    nat.search_scores(torch.from_numpy(terms).cuda(), torch.tensor(t_list, device="cuda"), scores, G, V, col_base=n - 1)
    got = scores.cpu().numpy()
    cols = [n - 1 - t for t in t_list]
    for g in range(G):
        ref = terms[g * V:(g + 1) * V][:, cols].astype(np.float64).mean()
        assert abs(float(got[g]) - ref) <= N_T * V * float(np.spacing(np.float32(ref))), (g, got[g], ref)


# ------------------------------------------------------------------------------------------------ the search
@pytest.mark.parametrize("group", [1, 4])
def test_scores_against_eager_backend(setup, eager, group):
    """Same seed, same U-Net kernels: the scores agree at rounding level, and in every round the frame the native backend
    picks is, by the eager scores, within that tolerance of the best."""
    e_sched, e_scorer = eager
    n_sched, n_scorer = run(setup, "native", group=group)
    assert n_scorer.G == group and n_scorer.ev.G == group
    if group == 4:
        assert any(len(c) % 4 for _, c, _ in n_scorer.rounds), "a partly filled last pass is part of the case"
    e_by_key = {}
    for s, cands, scores in e_scorer.rounds:
        e_by_key.setdefault((s, tuple(cands)), scores)
    worst = 0.0
    assert len(n_scorer.rounds) == len(e_scorer.rounds)
    for s, cands, scores in n_scorer.rounds:
        ref = e_by_key.get((s, tuple(cands)))
        assert ref is not None, f"step {s}: the backends diverged before the candidates {cands}"
        rel = np.abs(scores.astype(np.float64) - ref) / np.abs(ref)
        worst = max(worst, float(rel.max()))
        pick = int(np.argmin(scores))
        assert ref[pick] <= ref.min() + SCORE_RTOL * abs(ref.min()), (s, cands, scores, ref)
    print(f"[group {group}] largest relative deviation native vs eager over {sum(len(c) for _, c, _ in n_scorer.rounds)} "
          f"scores: {worst:.3e}")
    assert worst <= SCORE_RTOL, worst
    assert n_sched == e_sched


def test_replay_sees_the_listed_timesteps(setup):
    _, scorer = run(setup, "native", group=4)
    ev = scorer.ev
    t_list = [977, 312, 45, 0]
    ev.set_step(SEED, 1, t_list)
    ev.assemble(torch.from_numpy(scorer.round_slots([5, 6], [], [0, 1, 2, 3])[0]).cuda())
    for j, t in enumerate(t_list):
        ev.replay()
        torch.cuda.synchronize()
        assert ev.t_buf.tolist() == [t] * ev.plan.B and int(ev.ctl[0]) == j + 1
        assert float(ev.plan.tin[0]) == float(ev.ts_table[t])
    assert not ev.chain_timed_out()


def test_deterministic_one_capture_one_readback_per_round(setup):
    a_sched, a = run(setup, "native", group=4)
    b_sched, b = run(setup, "native", group=4)
    assert a_sched == b_sched
    assert len(a.rounds) == len(b.rounds)
    for (s0, c0, x0), (s1, c1, x1) in zip(a.rounds, b.rounds):
        assert s0 == s1 and c0 == c1 and np.array_equal(x0.view(np.uint32), x1.view(np.uint32))
    assert a.ev is b.ev and a.ev.captures == 1, "one shape, one capture - across rounds, window steps and calls"
    n_rounds = sum(min(K - len(lat), len(done)) for _, lat, done in osch.walk_scheme(make_scheme()))
    assert n_rounds == 16
    assert a.readbacks == n_rounds == len(a.rounds) and b.readbacks == n_rounds
    other_sched, other = run(setup, "native", group=4, seed=SEED + 1)
    assert other.ev.captures == 1
    assert any(not np.array_equal(x, y) for (_, _, x), (_, _, y) in zip(a.rounds, other.rounds)), "another seed, other noise"


def test_end_to_end_schedule_drives_sampling(setup, tmp_path):
    model, diffusion, videos = setup
    schedule = osch.find_optimal_schedule(model, diffusion, videos, make_scheme(), n_timesteps=N_T, seed=SEED)
    osch.save_optimal_schedule(schedule, tmp_path)
    args = default_sampling_args(sampling_scheme="autoreg", n_obs=N_OBS, max_frames=K, max_latent_frames=STEP,
                                 optimality="linspace-t", eval_dir=tmp_path, device="cuda")
    _, used = sample_video(args, model, diffusion, videos, just_get_indices=True, verbose=False)
    assert len(used) == len(schedule) == 4
    for s, (obs, lat) in enumerate(used):
        assert all(o == schedule[s] for o in obs), (s, obs, schedule[s])
        assert len(schedule[s]) == min(K - len(lat[0]), N_OBS + s * STEP)
