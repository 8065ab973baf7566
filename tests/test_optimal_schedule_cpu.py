"""Search for optimised conditioning frames (improved_diffusion/optimal_schedule.py), host side: the greedy driver against
a scripted scorer, the eager backend on a toy analytic model with a planted answer, the timestep lists, the refusals and
the C ABI of the new entries.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from improved_diffusion import _native, optimal_schedule as osch, script_util as su
from improved_diffusion.sampling_schemes import sampling_schemes

NEW_EXPORTS = ("lfvdm_search_assemble", "lfvdm_search_noise_qsample", "lfvdm_search_noise_fill", "lfvdm_search_scores")
T_VIDEO, N_OBS, K, STEP = 12, 3, 6, 2
SCHEMES = ("autoreg", "long-range", "hierarchy-2")


def make_scheme(name, path=None):
    return sampling_schemes[name](video_length=T_VIDEO, num_obs=N_OBS, max_frames=K, step_size=STEP, optimal_schedule_path=path)


def scripted_score(s, c):
    """Deterministic, with ties: candidates c and c + 1 (c even) share a score."""
    return float(((c // 2) * 7 + 3 * s) % 5)


@pytest.mark.parametrize("name", SCHEMES)
def test_greedy_driver_against_scripted_scorer(name, tmp_path):
    steps = osch.walk_scheme(make_scheme(name))
    by_step = {s: (lat, done) for s, lat, done in steps}
    calls = []

    def score_fn(s, lat, chosen, cands):
        calls.append((s, list(lat), list(chosen), list(cands)))
        return [scripted_score(s, c) for c in cands]

    scheme = make_scheme(name)
    schedule = osch.greedy_schedule(scheme, score_fn)
    assert scheme._current_step == 0 and scheme._done_frames == set(range(N_OBS)), "the caller's scheme is not advanced"

    # keys: exactly the conditional steps of the scheme as it iterates on its own
    own = list(iter(make_scheme(name)))
    assert sorted(schedule) == list(range(len(own))) == sorted(by_step)
    for s, (obs, lat) in enumerate(own):
        assert by_step[s][0] == [int(i) for i in lat], "the walk commits the scheme's own latent frames"

    # replay the rounds: candidates are D_s minus what is chosen, the pick is the first minimum, the budget is filled
    expect = {}
    for s, lat, chosen, cands in calls:
        L, D = by_step[s]
        assert lat == L and set(cands) <= set(D) and not set(cands) & set(chosen) and not set(cands) & set(L)
        assert cands == sorted(set(D) - set(chosen)), "every frame done before the step is a candidate, and no other"
        assert chosen == expect.get(s, [])
        sc = [scripted_score(s, c) for c in cands]
        pick = min(c for c, v in zip(cands, sc) if v == min(sc))          # ties -> lowest frame index
        expect.setdefault(s, []).append(pick)
    for s, (L, D) in by_step.items():
        assert len(schedule[s]) == min(K - len(L), len(D)), "budget filled, or capped by the frames done"
        assert schedule[s] == sorted(expect[s]) and len(set(schedule[s])) == len(schedule[s])

    # the saved file drives a fresh scheme to completion with those observed frames
    path = osch.save_optimal_schedule(schedule, tmp_path)
    assert os.path.basename(path) == "optimal_schedule.pt"
    loaded = torch.load(path)
    assert loaded == schedule and all(isinstance(k, int) for k in loaded)
    fresh = make_scheme(name, path)
    seen = list(iter(fresh))
    assert fresh.is_done() and len(seen) == len(own)
    for s, (obs, lat) in enumerate(seen):
        assert obs == schedule[s] and [int(i) for i in lat] == by_step[s][0]


def test_budget_capped_by_frames_done():
    scheme = sampling_schemes["autoreg"](video_length=8, num_obs=2, max_frames=6, step_size=2)
    schedule = osch.greedy_schedule(scheme, lambda s, lat, chosen, cands: [float(c) for c in cands])
    assert schedule[0] == [0, 1], "two frames done: the budget of four is capped"
    assert schedule[1] == [0, 1, 2, 3]


def test_unconditional_first_window_gets_no_entry():
    scheme = sampling_schemes["autoreg"](video_length=10, num_obs=0, max_frames=6, step_size=2)
    schedule = osch.greedy_schedule(scheme, lambda s, lat, chosen, cands: [float(-c) for c in cands])
    assert 0 not in schedule and min(schedule) == 1
    assert schedule[1] == [2, 3, 4, 5], "the lowest score is the highest frame here"


class NearestObservedModel:
    """Toy analytic x0-predictor: a latent frame's estimate is the content of the nearest observed frame (by frame index;
    ties: the earlier slot).  Counts its calls."""

    def __init__(self):
        self.calls = 0

    def __call__(self, x_t, timesteps, frame_indices, obs_mask, latent_mask, x0):
        self.calls += 1
        out = torch.zeros_like(x_t)
        obs = obs_mask.reshape(obs_mask.shape[0], -1) > 0
        for b in range(x_t.shape[0]):
            slots = torch.nonzero(obs[b]).flatten()
            for k in range(x_t.shape[1]):
                dist = (frame_indices[b, slots] - frame_indices[b, k]).abs()
                out[b, k] = x0[b, slots[int(dist.argmin())]]
        return out, None


@pytest.mark.parametrize("name", SCHEMES)
def test_eager_backend_finds_planted_answer(name):
    """Videos are a linear ramp in time: the closer the observed frame, the smaller the term.  Round 1 of every step must pick
    a frame adjacent to the latents whenever one is done."""
    diffusion = su.create_gaussian_diffusion(steps=50, predict_xstart=True)
    ramp = torch.linspace(-0.9, 0.9, T_VIDEO).reshape(1, T_VIDEO, 1, 1, 1)
    videos = (ramp * torch.tensor([1.0, -0.8]).reshape(2, 1, 1, 1, 1)).expand(2, T_VIDEO, 2, 4, 4).contiguous()
    scheme = make_scheme(name)
    model = NearestObservedModel()
    scorer = osch.make_scorer(model, diffusion, videos, scheme, n_timesteps=3, seed=5, backend="auto")
    assert isinstance(scorer, osch.EagerScorer), "a plain callable on the CPU goes to the eager composition"
    schedule = osch.greedy_schedule(scheme, scorer)
    assert model.calls > 0
    first_round = {}
    for s, cands, scores in scorer.rounds:
        first_round.setdefault(s, cands[int(np.argmin(scores))])
    checked = 0
    for s, lat, done in osch.walk_scheme(make_scheme(name)):
        adjacent = [d for d in done if any(abs(d - l) == 1 for l in lat)]
        if adjacent:
            assert first_round[s] in adjacent, (s, lat, done, first_round[s])
            checked += 1
        assert first_round[s] in schedule[s]
    assert checked > 0
    # the same seed gives the same schedule, through the public entry
    again = osch.find_optimal_schedule(NearestObservedModel(), diffusion, videos, make_scheme(name), n_timesteps=3, seed=5)
    assert again == schedule


def test_cpu_noise_is_keyed_by_frame_not_by_slot():
    a = osch.cpu_noise(3, 1, 2, 0, 7, (2, 4, 4))
    assert a.dtype == np.float32 and np.array_equal(a, osch.cpu_noise(3, 1, 2, 0, 7, (2, 4, 4)))
    for other in ((4, 1, 2, 0, 7), (3, 2, 2, 0, 7), (3, 1, 0, 0, 7), (3, 1, 2, 1, 7), (3, 1, 2, 0, 6)):
        assert not np.array_equal(a, osch.cpu_noise(*other, (2, 4, 4)))


def test_timestep_lists():
    ts = osch.timestep_list(1000, "linspace-t", 10)
    assert ts == [int(v) for v in np.linspace(0, 999, 10).round()][::-1]
    assert ts[0] == 999 and ts[-1] == 0 and all(a > b for a, b in zip(ts, ts[1:]))
    assert osch.timestep_list(50, "linspace-t", 3) == [49, 24, 0] or osch.timestep_list(50, "linspace-t", 3) == [49, 25, 0]
    r1 = osch.timestep_list(1000, "random-t", 10, seed=3, step=2)
    assert r1 == osch.timestep_list(1000, "random-t", 10, seed=3, step=2), "reproducible by seed"
    assert r1 == osch.timestep_list(1000, "random-t", 10, seed=4, step=1), "keyed by seed + step"
    assert r1 != osch.timestep_list(1000, "random-t", 10, seed=3, step=3)
    assert len(set(r1)) == 10 and all(a > b for a, b in zip(r1, r1[1:])) and all(0 <= t < 1000 for t in r1)
    assert r1 == sorted(np.random.RandomState(5).choice(1000, size=10, replace=False).tolist(), reverse=True)
    with pytest.raises(ValueError):
        osch.timestep_list(1000, "best-t", 10)
    with pytest.raises(ValueError):
        osch.timestep_list(10, "random-t", 11)


def test_refusals():
    videos = torch.zeros(1, T_VIDEO, 2, 4, 4)
    model = NearestObservedModel()
    adaptive = sampling_schemes["adaptive-autoreg"](video_length=T_VIDEO, num_obs=N_OBS, max_frames=K, step_size=STEP)
    fixed = su.create_gaussian_diffusion(steps=50)
    with pytest.raises(ValueError, match="adaptive"):
        osch.find_optimal_schedule(model, fixed, videos, adaptive)
    learned = su.create_gaussian_diffusion(steps=50, learn_sigma=True)
    with pytest.raises(NotImplementedError, match="learn_sigma"):
        osch.find_optimal_schedule(model, learned, videos, make_scheme("autoreg"))
    with pytest.raises(ValueError, match="backend"):
        osch.find_optimal_schedule(model, fixed, videos, make_scheme("autoreg"), backend="native")
    assert model.calls == 0, "refused before anything runs"


def test_window_slots_order():
    frames, roles = osch.window_slots([7, 8], [5, 1], 6)
    assert frames == [1, 5, 7, 8, -1, -1]
    assert roles == [_native.SLOT_OBS] * 2 + [_native.SLOT_LATENT] * 2 + [_native.SLOT_PAD] * 2
    with pytest.raises(ValueError):
        osch.window_slots([7, 8], [1, 2, 3, 4, 5], 6)


def test_search_entries_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "lfvdm_hip.h")).read()
    declared = set(re.findall(r"\b(lfvdm_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW_EXPORTS:
        assert name in declared, f"{name} is not declared in include/lfvdm_hip.h"
        assert name in _native.EXPORTS and name in _native._SIGS, name
        assert hasattr(lib, name), name
    assert len(_native._SIGS["lfvdm_search_assemble"][0]) == 15
    assert len(_native._SIGS["lfvdm_search_noise_qsample"][0]) == 15
    src = open(os.path.join(ROOT, "latent-flexible-video-diffusion-modeling_amd", "csrc", "philox_normal.h")).read()
    ids = dict(re.findall(r"(NOISE_STREAM_[A-Z]+) = (\d+)", src))
    assert len(set(ids.values())) == len(ids) == 4 and ids["NOISE_STREAM_SEARCH"] == "3", "every stream has an id of its own"
