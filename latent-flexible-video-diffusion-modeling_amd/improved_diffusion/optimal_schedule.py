"""Optimised sampling schemes: search for the conditioning frames of every window step of a sampling scheme, and write
the ``optimal_schedule.pt`` that ``SamplingSchemeBase(optimal_schedule_path=...)`` and ``sample_video(..., optimality=...,
eval_dir=...)`` consume - a dict {window step -> observed frame indices}.  Not in the reference (its ``--optimality`` help
points at a script it does not ship); the algorithm is defined here.

    python -m improved_diffusion.optimal_schedule CHECKPOINT --sampling_scheme autoreg --optimality linspace-t
           --n_timesteps 10 --n_videos 2 --eval_dir DIR [--T --n_obs --max_frames --max_latent_frames --seed]

The search.  The scheme is walked with its own ``next_indices()`` (its own latent frames are committed), which gives for
window step s the latent frames L_s and the frames D_s done before it.  The conditioning frames are then chosen greedily
forward: ``max_frames - len(L_s)`` times (at most ``len(D_s)``), every frame c of D_s not yet chosen is scored and the one
with the lowest score joins ``chosen`` (ties: the lowest frame index).  score(c) is the mean, over the V videos and the
sub-sampled timesteps, of the variational-bound term in bits per dimension (``GaussianDiffusion._vb_terms_bpd``) restricted
to the latent frames, in a window of ``max_frames`` slots with ``chosen + [c]`` observed, L_s latent and the rest padding.
``sorted(chosen)`` is stored under s; an unconditional first window gets no entry.

Common random numbers.  Within a window step every candidate of every round is scored at the SAME timesteps and under the
SAME noise: the noise of a frame is a function of (seed, s, timestep position j, video, video frame index, element) alone
- not of the slot the frame sits in, nor of the batch element that holds it.  The score of a candidate is a Monte-Carlo
estimate over a handful of timesteps and videos; with fresh noise per candidate the difference between two candidates would
carry two independent estimation errors, each larger than the effect of swapping one conditioning frame, and the argmin
would mostly pick the luckiest draw.  Under shared noise the errors are common to all candidates and cancel in the
comparison, which is all the greedy step needs.

Backends.  ``native`` (a ``UNetVideoModel`` on the GPU): one pass scores ``group`` candidates on the V videos as a batch of
``group * V`` windows through one captured hipGraph (``SearchEvaluator``, csrc/schedule_search.hip): the conditioning sets
reach the device as an int32 slot table, the scores come back once per greedy round.  ``eager``: the same search composed
from the public API per candidate (hand-built ``model_kwargs``, ``q_sample(noise=...)``, ``_vb_terms(..., noise=...)``), for
any callable model on any device - the yardstick of the native backend.  On the GPU its noise is the native stream
(lfvdm_search_noise_fill); on the CPU it is ``cpu_noise``: numpy's ``default_rng([seed, s, j, video, frame])`` - another
generator, the same keying rule - and the term is evaluated by ``losses.py`` in torch.

The effect of optimised schedules on the sample quality of a trained model has not been measured here.
"""
import copy
import math
import os

import numpy as np
import torch as th

from . import _native as nat
from ._replay import ReplayedStep
from .sampling_schemes import AdaptiveSamplingSchemeBase, sampling_schemes

SCHEDULE_FILE = "optimal_schedule.pt"
OPTIMALITIES = ("linspace-t", "random-t")
_SEED_MASK = (1 << 63) - 1        # the seed travels as a non-negative int64


# ---------------------------------------------------------------------------------------------- host-side pieces
def timestep_list(num_timesteps, optimality, n_timesteps, seed=0, step=0):
    """The sub-sampled timesteps of window step ``step``, descending.  ``linspace-t``: evenly spread over the chain, both
    ends included; ``random-t``: distinct draws of ``np.random.RandomState(seed + step)``."""
    n = int(n_timesteps)
    if optimality not in OPTIMALITIES:
        raise ValueError(f"optimality is one of {OPTIMALITIES}, got {optimality!r}")
    if not 1 <= n <= num_timesteps:
        raise ValueError(f"n_timesteps must lie in [1, {num_timesteps}], got {n}")
    if optimality == "linspace-t":
        ts = np.unique(np.linspace(0, num_timesteps - 1, n).round().astype(np.int64))
    else:
        ts = np.random.RandomState((int(seed) + int(step)) % (1 << 32)).choice(num_timesteps, size=n, replace=False)
    return sorted((int(t) for t in ts), reverse=True)


def walk_scheme(scheme):
    """[(s, L_s, D_s)] of the conditional window steps of ``scheme`` (a copy is walked; the scheme's own conditioning
    frames are ignored, its latent frames committed)."""
    sc = copy.deepcopy(scheme)
    sc.optimal_schedule = None
    steps = []
    while not sc.is_done():
        s = sc._current_step
        unconditional = sc._num_obs == 0 and s == 0
        done = sorted(int(i) for i in sc._done_frames)
        obs, lat = ([], sc.get_unconditional_indices()) if unconditional else sc.next_indices()
        sc._check_and_commit(obs, lat)
        if unconditional:
            sc._obs_frames = lat
        else:
            steps.append((s, [int(i) for i in lat], done))
    return steps


def greedy_schedule(scheme, score_fn):
    """The greedy forward selection over ``walk_scheme(scheme)``.  ``score_fn(s, latent, chosen, candidates)`` returns one
    finite score per candidate (candidates ascending); -> {s: sorted(chosen)}."""
    K = scheme._max_frames
    schedule = {}
    for s, lat, done in walk_scheme(scheme):
        budget = min(K - len(lat), len(done))
        chosen = []
        for _ in range(budget):
            cands = [c for c in done if c not in chosen]
            scores = np.asarray(score_fn(s, list(lat), list(chosen), list(cands)), dtype=np.float64)
            if scores.shape != (len(cands),) or not np.isfinite(scores).all():
                raise RuntimeError(f"window step {s}: the scorer returned {scores!r} for the candidates {cands}")
            chosen.append(cands[int(np.argmin(scores))])       # first minimum = lowest frame index
        schedule[s] = sorted(chosen)
    return schedule


def window_slots(lat, obs, K):
    """(frames, roles) of one window of K slots: observed frames (ascending) first, then the latents - the order
    ``video_sampler.window_inputs`` lays out - then padding (-1)."""
    obs = sorted(obs)
    if len(obs) + len(lat) > K:
        raise ValueError(f"{len(obs)} observed + {len(lat)} latent frames do not fit a window of {K}")
    n_pad = K - len(obs) - len(lat)
    return (list(obs) + list(lat) + [-1] * n_pad,
            [nat.SLOT_OBS] * len(obs) + [nat.SLOT_LATENT] * len(lat) + [nat.SLOT_PAD] * n_pad)


def cpu_noise(seed, step, j, video, frame, shape):
    """The CPU backend's noise of one frame: numpy's ``default_rng([seed, step, j, video, frame])`` (PCG64 behind a
    SeedSequence of the five integers), ``standard_normal`` in fp32.  Keyed as the native stream is, not equal to it."""
    rng = np.random.default_rng([int(seed) & _SEED_MASK, int(step), int(j), int(video), int(frame)])
    return rng.standard_normal(int(np.prod(shape)), dtype=np.float32).reshape(shape)


def _unwrap(model):
    inner = getattr(model, "model", model)       # _WrappedModel -> module
    return getattr(inner, "module", inner)       # DDP -> module


def _refuse(scheme, diffusion):
    from .gaussian_diffusion import ModelVarType
    if isinstance(scheme, AdaptiveSamplingSchemeBase):
        raise ValueError(f"the adaptive scheme {scheme.typename!r} chooses its conditioning frames per video while it samples: "
                         "there is no fixed schedule to optimise")
    if diffusion.model_var_type not in (ModelVarType.FIXED_LARGE, ModelVarType.FIXED_SMALL):
        raise NotImplementedError("the search scores with the fixed-sigma variational-bound terms: learned sigma "
                                  "(learn_sigma=True) is not supported")
    # the scores are variational-bound terms under independent noise keyed by video frame (set_noise_prior's docstring)
    diffusion._refuse_noise_prior("the schedule search (find_optimal_schedule)")


# ---------------------------------------------------------------------------------------------- native backend
class SearchEvaluator(ReplayedStep):
    """One evaluation step of the search (lfvdm_search_noise_qsample: position -> t, noise, x_t; the plan's clock; U-Net
    forward; lfvdm_vb_terms into the column of t) captured ONCE as a hipGraph over a private plan of W = G * V windows.  The
    plan carries no timestep tables: the frame indices change with every pass, and the R tables are keyed by them.  A pass
    is ``run_pass``: slot table -> lfvdm_search_assemble, the graph n_t times, lfvdm_search_scores."""

    def __init__(self, diffusion, unet, shape, clip_denoised, V):
        super().__init__(diffusion, unet, shape, clip_denoised, False, time_tables=False)
        W, K = self.plan.B, self.plan.T
        if W % V:
            raise ValueError(f"{W} windows are no whole number of candidates on {V} videos")
        dev, n = self.plan.dev, diffusion.num_timesteps
        self.V, self.G = int(V), W // int(V)
        self.x_start = th.zeros(self.shape, device=dev)
        self.noise = th.zeros(self.shape, device=dev)
        self.mask = th.zeros(W, K, device=dev)                      # the latent frames: what the term is restricted to
        self.slots = th.full((2, W, K), -1, dtype=th.int32, device=dev)   # [0] video frame per slot, [1] role per slot
        self.slots[1].zero_()
        self.t_list = th.zeros(n, dtype=th.int64, device=dev)
        self.n_t = 1
        self.ctl = th.tensor([0, 0, 1, 0], dtype=th.int32, device=dev)    # position, ticket, n_t, unused
        self.key = th.zeros(2, dtype=th.int64, device=dev)               # seed, window step
        self.terms = th.zeros(W, n, device=dev)
        self.pool = None
        self.captures = 0
        self.passes = 0

    @property
    def launches_per_step(self):
        """Launches of one replayed step: the noise / q_sample head, the clock, the plan's own, the term."""
        return len(self.plan.steps) + 3

    def _step_body(self):
        pl, tb, d = self.plan, self.tb, self.diffusion
        nat.search_noise_qsample(self.x_start, self.slots[0], self.t_list, self.ctl, self.key, tb["sqrt_alphas_cumprod"],
                                 tb["sqrt_one_minus_alphas_cumprod"], self.noise, pl.x_in, self.t_buf, self.V)
        pl.tick(self.t_buf, self.ts_table)          # t_buf holds t + 1: t, the model timestep (and FiLM rows) of t
        pl.launch()
        recip, recipm1, c1, c2, post_lv, model_lv = d._vb_tables(pl.dev)
        nat.vb_terms(self.x_start, pl.x_in, pl.out, None, self.t_buf, recip, recipm1, c1, c2, post_lv, model_lv, self.mask,
                     nat.MEAN_X0 if self.x0_mode else nat.MEAN_EPS, self.clip, self.terms, None, None, None,
                     col_base=d.num_timesteps - 1)

    def _capture_step(self):
        super()._capture_step()
        self.captures += 1

    def set_pool(self, videos):
        """The resident video pool (V, T_video, C, H, W)."""
        if videos.shape[0] != self.V or tuple(videos.shape[2:]) != self.shape[2:]:
            raise ValueError(f"videos {tuple(videos.shape)} do not fit an evaluator of {self.V} videos, frames {self.shape[2:]}")
        self.pool = videos.to(self.plan.dev, th.float32).contiguous()

    def set_step(self, seed, step, t_list):
        """The window step's noise key and timesteps (descending) -> the device words the captured step reads."""
        n = self.diffusion.num_timesteps
        ts = [int(t) for t in t_list]
        if not ts or len(ts) > min(n, 65535) or any(not 0 <= t < n for t in ts):
            raise ValueError(f"at most 65535 timesteps, each in [0, {n}): got {ts}")
        if not 0 <= int(step) < (1 << 24):
            raise ValueError(f"window step {step} does not fit the noise counter")
        self.n_t = len(ts)
        self.t_list[:self.n_t].copy_(th.tensor(ts, dtype=th.int64))
        self.ctl.copy_(th.tensor([0, 0, self.n_t, 0], dtype=th.int32))
        self.key.copy_(th.tensor([int(seed) & _SEED_MASK, int(step)], dtype=th.int64))

    def assemble(self, slots):
        """``slots`` (2, W, K) int32 (device) -> the plan's and the evaluator's window buffers; the position back to 0."""
        pl = self.plan
        self.slots.copy_(slots)
        nat.search_assemble(self.pool, self.slots[0], self.slots[1], pl.x0_in, self.x_start, pl.obs, self.mask, pl.mask, pl.fi)
        self.ctl[:2].zero_()

    def replay(self):
        """One replay of the captured step: the next timestep position."""
        self.graph.replay()
        self._abort_unchecked = True

    def run_pass(self, slots, scores):
        """One pass: ``scores`` (G,) <- the candidates of ``slots``.  No host synchronisation."""
        pl = self.plan
        with th.no_grad():
            if pl._sig != pl.weight_signature():
                pl.refresh_weights()            # parameters changed since the last pass
            self.assemble(slots)
            if self.graph is None:
                self._capture_step()
                self.ctl[:2].zero_()            # the warm-up step advanced the position
            for _ in range(self.n_t):
                self.replay()
            nat.search_scores(self.terms, self.t_list[:self.n_t], scores, self.G, self.V,
                              col_base=self.diffusion.num_timesteps - 1)
        self.passes += 1


def _search_evaluator(diffusion, unet, shape, clip_denoised, V):
    cache = diffusion.__dict__.setdefault("_search_evals", {})
    key = (id(unet), tuple(shape), bool(clip_denoised), int(V))
    ev = cache.get(key)
    if ev is None or ev.unet is not unet or ev.engine is not unet.native_engine():
        cache.clear()       # graphs pin device memory: one search shape at a time
        ev = cache[key] = SearchEvaluator(diffusion, unet, shape, clip_denoised, V)
    return ev


class NativeScorer:
    """score_fn of ``greedy_schedule`` on the native backend.  ``rounds`` keeps (s, candidates, scores) of every greedy
    round; ``readbacks`` counts the score read-backs: one per round (a round rerun after a level-chain timeout reads again)."""

    def __init__(self, model, diffusion, videos, K, *, optimality, n_timesteps, seed, clip_denoised, group):
        unet = _unwrap(model)
        V = videos.shape[0]
        self.G = max(1, 8 // V) if group is None else int(group)
        if self.G < 1:
            raise ValueError(f"group must be at least 1, got {group}")
        self.V, self.K, self.seed, self.optimality, self.n_timesteps = V, int(K), int(seed), optimality, int(n_timesteps)
        self.diffusion = diffusion
        self.ev = _search_evaluator(diffusion, unet, (self.G * V, self.K) + tuple(videos.shape[2:]), clip_denoised, V)
        self.ev.set_pool(videos)
        self.step = None
        self.readbacks = 0
        self.rounds = []

    def round_slots(self, lat, chosen, cands):
        """(P, 2, W, K) int32: the slot and role tables of the passes of one round.  The last pass is filled up with repeats
        of its first candidate; their scores are dropped."""
        G, V, K = self.G, self.V, self.K
        P = (len(cands) + G - 1) // G
        tabs = np.empty((P, 2, G * V, K), dtype=np.int32)
        for p in range(P):
            for g in range(G):
                i = p * G + g
                c = cands[i] if i < len(cands) else cands[p * G]
                frames, roles = window_slots(lat, chosen + [c], K)
                tabs[p, 0, g * V:(g + 1) * V] = frames
                tabs[p, 1, g * V:(g + 1) * V] = roles
        return tabs

    def __call__(self, s, lat, chosen, cands):
        ev, G = self.ev, self.G
        if s != self.step:
            ev.set_step(self.seed, s, timestep_list(self.diffusion.num_timesteps, self.optimality, self.n_timesteps, self.seed, s))
            self.step = s
        tabs = th.from_numpy(self.round_slots(lat, chosen, cands)).to(ev.plan.dev)
        for attempt in range(2):
            scores = th.empty(tabs.shape[0] * G, device=ev.plan.dev)
            for p in range(tabs.shape[0]):
                ev.run_pass(tabs[p], scores[p * G:(p + 1) * G])
            host = scores.cpu().numpy()[:len(cands)]           # the round's one host synchronisation
            self.readbacks += 1
            # the samplers' protocol: a persistent level chain that gave up a wait leaves garbage behind - say so, run one
            # launch per stage from now on (the graph is captured again) and score the round again
            if attempt == 0 and ev.chain_timed_out():
                ev.fall_back()
                continue
            break
        self.rounds.append((s, list(cands), host.copy()))
        return host


# ---------------------------------------------------------------------------------------------- eager backend
def _vb_term_torch(diffusion, x_start, x_t, out, t, clip_denoised, latent_mask):
    """The term of ``lfvdm_vb_terms`` in plain torch (losses.py), for tensors that are not on the GPU -> (B,)."""
    from .losses import discretized_gaussian_log_likelihood, normal_kl
    tb = diffusion.tables(x_t.device)

    def at(name):
        return tb[name][t].reshape(-1, 1, 1, 1, 1)
    pred = out if diffusion.predicts_xstart else at("sqrt_recip_alphas_cumprod") * x_t - at("sqrt_recipm1_alphas_cumprod") * out
    if clip_denoised:
        pred = pred.clamp(-1, 1)
    c1, c2 = at("posterior_mean_coef1"), at("posterior_mean_coef2")
    mean_model, mean_true = c1 * pred + c2 * x_t, c1 * x_start + c2 * x_t
    model_lv = at("model_log_variance").expand(x_t.shape)
    kl = normal_kl(mean_true, at("posterior_log_variance_clipped"), mean_model, model_lv)
    nll = -discretized_gaussian_log_likelihood(x_start, means=mean_model, log_scales=0.5 * model_lv)
    term = th.where((t == 0).reshape(-1, 1, 1, 1, 1), nll, kl) * latent_mask.reshape(x_t.shape[0], x_t.shape[1], 1, 1, 1)
    return term.flatten(1).mean(dim=1) / math.log(2.0)


class EagerScorer:
    """score_fn of ``greedy_schedule`` composed from the public API, one candidate at a time: windows of K slots (padding:
    zero frames, frame index 0, neither observed nor latent), ``q_sample(noise=...)``, ``_vb_terms(..., noise=...)``."""

    def __init__(self, model, diffusion, videos, K, *, optimality, n_timesteps, seed, clip_denoised):
        self.model, self.diffusion, self.videos = model, diffusion, videos.float()
        self.K, self.seed, self.optimality, self.n_timesteps = int(K), int(seed), optimality, int(n_timesteps)
        self.clip = bool(clip_denoised)
        self.rounds = []

    def _noise(self, table, s, j):
        V, K = table.shape
        shape = (V, K) + tuple(self.videos.shape[2:])
        if self.videos.is_cuda:
            noise = th.empty(shape, device=self.videos.device)
            nat.search_noise_fill(table, self.seed & _SEED_MASK, s, j, noise, V)
            return noise
        noise = np.zeros(shape, dtype=np.float32)
        for v in range(V):
            for k in range(K):
                f = int(table[v, k])
                if f >= 0:
                    noise[v, k] = cpu_noise(self.seed, s, j, v, f, shape[2:])
        return th.from_numpy(noise).to(self.videos.device)

    def score(self, s, lat, obs):
        """The score of the conditioning set ``obs`` at window step ``s`` (python float, accumulated in float64)."""
        d, dev = self.diffusion, self.videos.device
        V = self.videos.shape[0]
        frames, roles = window_slots(lat, obs, self.K)
        table = th.tensor([frames] * V, dtype=th.int32, device=dev)
        role = th.tensor([roles] * V, device=dev)
        fi = table.long().clamp(min=0)
        pad = (table < 0).reshape(V, self.K, 1, 1, 1)
        x_start = self.videos[th.arange(V, device=dev)[:, None], fi].masked_fill(pad, 0.0).contiguous()
        obs_mask = (role == nat.SLOT_OBS).float().reshape(V, self.K, 1, 1, 1)
        latent_mask = (role == nat.SLOT_LATENT).float().reshape(V, self.K, 1, 1, 1)
        model_kwargs = dict(frame_indices=fi, x0=x_start, obs_mask=obs_mask, latent_mask=latent_mask)
        terms = []
        for j, t_j in enumerate(timestep_list(d.num_timesteps, self.optimality, self.n_timesteps, self.seed, s)):
            t = th.full((V,), t_j, dtype=th.long, device=dev)
            noise = self._noise(table, s, j)
            with th.no_grad():
                if x_start.is_cuda:
                    x_t = d.q_sample(x_start, t, noise=noise)
                    vb = d._vb_terms(self.model, x_start, x_t, t, self.clip, model_kwargs, latent_mask, noise=noise)["output"]
                else:
                    tb = d.tables(dev)
                    x_t = (tb["sqrt_alphas_cumprod"][t].reshape(-1, 1, 1, 1, 1) * x_start
                           + tb["sqrt_one_minus_alphas_cumprod"][t].reshape(-1, 1, 1, 1, 1) * noise)
                    out, _ = d._wrap_model(self.model)(x_t, timesteps=d._scale_timesteps(t), **model_kwargs)
                    vb = _vb_term_torch(d, x_start, x_t, out, t, self.clip, latent_mask)
            terms.append(vb)
        return float(th.stack(terms, dim=1).double().mean())

    def __call__(self, s, lat, chosen, cands):
        scores = np.array([self.score(s, lat, chosen + [c]) for c in cands])
        self.rounds.append((s, list(cands), scores.copy()))
        return scores


# ---------------------------------------------------------------------------------------------- public interface
def pick_backend(model, videos, backend="auto"):
    """``auto``: native for a ``UNetVideoModel`` on the GPU, the eager composition for everything else."""
    from .unet import UNetVideoModel
    if backend not in ("auto", "native", "eager"):
        raise ValueError(f"backend is 'auto', 'native' or 'eager', got {backend!r}")
    native_ok = isinstance(_unwrap(model), UNetVideoModel) and videos.is_cuda
    if backend == "native" and not native_ok:
        raise ValueError("backend='native' needs a UNetVideoModel and videos on the GPU")
    return "native" if backend == "native" or (backend == "auto" and native_ok) else "eager"


def make_scorer(model, diffusion, videos, scheme, *, optimality="linspace-t", n_timesteps=10, seed=0, clip_denoised=True,
                group=None, backend="auto"):
    """The score_fn ``find_optimal_schedule`` hands to ``greedy_schedule`` (it keeps the per-round scores and counters)."""
    _refuse(scheme, diffusion)
    if videos.dim() != 5:
        raise ValueError(f"videos are (V, T_video, C, H, W), got {tuple(videos.shape)}")
    if videos.shape[1] < scheme._video_length:
        raise ValueError(f"the scheme walks {scheme._video_length} frames, the videos have {videos.shape[1]}")
    timestep_list(diffusion.num_timesteps, optimality, n_timesteps, seed, 0)       # refuse bad settings before anything runs
    kw = dict(optimality=optimality, n_timesteps=n_timesteps, seed=seed, clip_denoised=clip_denoised)
    if pick_backend(model, videos, backend) == "native":
        return NativeScorer(model, diffusion, videos, scheme._max_frames, group=group, **kw)
    return EagerScorer(model, diffusion, videos, scheme._max_frames, **kw)


def find_optimal_schedule(model, diffusion, videos, scheme, *, optimality="linspace-t", n_timesteps=10, seed=0,
                          clip_denoised=True, group=None, backend="auto"):
    """{window step -> observed frame indices} for ``scheme`` (an instance of a non-adaptive scheme of
    ``sampling_schemes``; it is not advanced), chosen on ``videos`` (V, T_video, C, H, W) in diffusion space.  See the
    module docstring for the algorithm; ``group``: candidates per pass (default: the largest with group * V <= 8)."""
    scorer = make_scorer(model, diffusion, videos, scheme, optimality=optimality, n_timesteps=n_timesteps, seed=seed,
                         clip_denoised=clip_denoised, group=group, backend=backend)
    return greedy_schedule(scheme, scorer)


def save_optimal_schedule(schedule, eval_dir):
    """``eval_dir/optimal_schedule.pt``: where ``sample_video(..., optimality=..., eval_dir=...)`` looks for it."""
    os.makedirs(eval_dir, exist_ok=True)
    path = os.path.join(str(eval_dir), SCHEDULE_FILE)
    th.save({int(s): [int(i) for i in obs] for s, obs in schedule.items()}, path)
    return path


def main(argv=None):
    import argparse
    from pathlib import Path
    from . import script_util as su
    from .video_datasets import default_T_dict, get_train_dataset
    ap = argparse.ArgumentParser(description="Search the optimal conditioning frames of a sampling scheme")
    ap.add_argument("checkpoint_path")
    ap.add_argument("--sampling_scheme", required=True, choices=sorted(sampling_schemes))
    ap.add_argument("--optimality", default="linspace-t", choices=OPTIMALITIES)
    ap.add_argument("--n_timesteps", type=int, default=10)
    ap.add_argument("--n_videos", type=int, default=2)
    ap.add_argument("--eval_dir", required=True)
    ap.add_argument("--T", type=int, default=None)
    ap.add_argument("--n_obs", type=int, default=36)
    ap.add_argument("--max_frames", type=int, default=20)
    ap.add_argument("--max_latent_frames", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda" if th.cuda.is_available() else "cpu")
    args = ap.parse_args(argv)
    # model, diffusion and dataset come from the checkpoint, as for sampling
    data = th.load(args.checkpoint_path, map_location="cpu")
    cfg = dict(data["config"])
    defaults = su.model_and_diffusion_defaults()
    model, diffusion = su.create_model_and_diffusion(**{k: cfg.get(k, v) for k, v in defaults.items()})
    model.load_state_dict(data["state_dict"])
    model = model.to(args.device).eval()
    T = args.T if args.T is not None else cfg.get("T") or default_T_dict[cfg["dataset"]]
    step = args.max_latent_frames if args.max_latent_frames is not None else args.max_frames // 2
    scheme = sampling_schemes[args.sampling_scheme](video_length=T, num_obs=args.n_obs, max_frames=args.max_frames,
                                                    step_size=step)
    np.random.seed(args.seed)       # the training set cuts its windows with numpy's global generator
    dataset = get_train_dataset(cfg["dataset"], T=T)
    videos = th.stack([dataset[i][0] for i in range(args.n_videos)]).to(args.device)
    if getattr(diffusion, "diffusion_space", None) == "latent" and not getattr(diffusion, "pre_encoded", False):
        videos = diffusion.encode(videos)
    schedule = find_optimal_schedule(model, diffusion, videos, scheme, optimality=args.optimality,
                                     n_timesteps=args.n_timesteps, seed=args.seed)
    path = save_optimal_schedule(schedule, Path(args.eval_dir))
    for s in sorted(schedule):
        print(f"step {s}: condition on {schedule[s]}")
    print(f"wrote {path}")
    return schedule


if __name__ == "__main__":
    main()
