"""Frame distances and farthest-point selection without a GPU (improved_diffusion/frame_select.py, csrc/frame_select.hip):
the float64 definition against pooling composed by hand, the spec parser and every refusal, the CPU selection against the
scheme's existing host loop with an identity embed_fn, the adaptive schemes under ``set_frame_metric``, the distance cache,
``sample_video`` with ``adaptive_metric`` and the two C-ABI additions (declared, bound, exported, refusing before a launch).

Bound of a float32 distance against the float64 reference (``rel_bound``): all terms are non-negative, so any summation
order has relative error at most (n + 2) 2^-24 with n the longest addition chain; n = D (the element count) bounds every
order, plus (2^L)^2 for the pooling sums.  At D <= 1025 a dropped or doubled element is a relative error of about 1 / D, far
above the bound.

Picks are compared between float32 and float64 routes only on inputs with a MARGIN (``select_with_margin``): at every free
pick the float64 reference's best and second-best min_d differ by more than 4 x that bound, relative.  A pick whose best
min_d is exactly 0 is exempt: then every candidate has been picked (distinct frames have positive distances), every route
holds exact zeros (x - x = 0) and argmax returns position 0 in all of them.  Random-walk videos (cumulative sum of N(0, 1)
frames times 0.3) give margins of 1e-4 and more; the assertion is on the reference itself, no case is skipped."""
import contextlib
import ctypes
import functools
import io
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "latent-flexible-video-diffusion-modeling_amd")
NEW_EXPORTS = ("lfvdm_frame_dist_rows", "lfvdm_fps_select")
E_SHAPE, E_UNSUPPORTED = 1, 3
ADAPTIVE = ("adaptive-autoreg", "adaptive-hierarchy-2", "adaptive-hierarchy-3")


def rel_bound(D, L):
    return (D + 2 + (2 ** L) ** 2) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def walk(B, T, C, H, W, seed):
    """Random-walk videos (B, T, C, H, W) float32: neighbouring frames are close, distant ones far.  Shared, never modified."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, C, H, W, generator=g, dtype=torch.float64).cumsum(dim=1) * 0.3).float()


@functools.lru_cache(maxsize=None)
def full_reference(B, T, C, H, W, seed, L):
    """(B, T, T) float64: every pair of frames of ``walk`` by the reference."""
    from improved_diffusion.frame_select import frame_distance_reference
    v = walk(B, T, C, H, W, seed)
    return frame_distance_reference(v[:, :, None], v[:, None, :], L)


def select_with_margin(d64, cand, n, forced, bound):
    """The host loop on the float64 matrix ``d64`` (T, T) of one video -> (frames picked, worst relative margin over the free
    picks); asserts the margin (module docstring)."""
    sub = d64[np.ix_(cand, cand)]
    min_d = np.full(len(cand), np.inf)
    picks, worst = [forced[0]], np.inf
    for i in range(1, n):
        min_d = np.minimum(min_d, sub[picks[-1]])
        if i < len(forced):
            picks.append(forced[i])
            continue
        order = np.sort(min_d)[::-1]
        best, second = order[0], order[1] if len(order) > 1 else -np.inf
        if best > 0:
            margin = (best - second) / best
            worst = min(worst, margin)
            assert margin > 4 * bound, f"pick {i}: margin {margin:.2e} is not above 4 x the bound {bound:.2e}: choose another seed"
        picks.append(int(np.argmax(min_d)))
    return [cand[p] for p in picks], worst


def identity_embed(vids, idx):
    return torch.stack([vids[:, i].flatten(1) for i in idx], dim=1)


def make_scheme(name, T, n_obs, K, step):
    from improved_diffusion.sampling_schemes import sampling_schemes
    with contextlib.redirect_stdout(io.StringIO()):
        return iter(sampling_schemes[name](video_length=T, num_obs=n_obs, max_frames=K, step_size=step))


def run_adaptive(scheme, videos, before_select=None):
    """Drive an adaptive scheme over fixed ``videos`` -> [(obs per video, lat)] as ints.  ``before_select(cand, n, forced)`` is
    called ahead of every selection."""
    if before_select is not None:
        inner = scheme.select_obs_indices

        def checked(possible_next_indices, n, always_selected=(0,)):
            before_select(list(possible_next_indices), n, list(always_selected))
            return inner(possible_next_indices, n, always_selected)
        scheme.select_obs_indices = checked
    out = []
    with contextlib.redirect_stdout(io.StringIO()):
        while True:
            scheme.set_videos(videos)
            try:
                obs, lat = next(scheme)
            except StopIteration:
                break
            out.append(([[int(i) for i in o] for o in obs], [int(i) for i in lat[0]]))
    return out


def margin_checker(ref64, bound, log=None):
    """-> a ``before_select`` that asserts the margin of this selection on every video of the float64 matrix ``ref64``."""
    def check(cand, n, forced):
        for b in range(ref64.shape[0]):
            _, worst = select_with_margin(ref64[b].numpy(), cand, n, forced, bound)
            if log is not None:
                log.append(worst)
    return check


# ------------------------------------------------------------------------------------------------ C ABI
def test_new_exports_are_declared_bound_and_exported():
    from improved_diffusion import _native
    hdr = open(os.path.join(ROOT, "include", "lfvdm_hip.h")).read()
    declared = set(re.findall(r"\b(lfvdm_[a-z0-9_]+)\s*\(", hdr))
    lib = _native.lib()
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _native.EXPORTS and name in _native._SIGS, name
        assert hasattr(lib, name), name
    assert len(_native._SIGS["lfvdm_frame_dist_rows"][0]) == 13 and len(_native._SIGS["lfvdm_fps_select"][0]) == 10
    assert callable(_native.frame_dist_rows) and callable(_native.fps_select)
    src = open(os.path.join(PKG, "csrc", "frame_select.hip")).read()
    assert "atomicAdd" not in src and "atomic_" not in src, "no float atomics: the summation order is fixed"


def test_entries_refuse_bad_arguments_before_any_launch():
    """No device here: a launch would fail with LFVDM_E_LAUNCH (2), so 1 / 3 show that the refusal came first."""
    from improved_diffusion import _native
    lib = _native.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)      # a non-null pointer; nothing is ever read through it

    def rows(x=p, B=2, T=8, C=3, H=8, W=8, L=3, new=p, n_new=2, cand=p, n_cand=3, dist=p):
        return lib.lfvdm_frame_dist_rows(x, B, T, C, H, W, L, new, n_new, cand, n_cand, dist, None)
    for kw in (dict(L=0), dict(L=4), dict(H=6), dict(W=10), dict(H=7, L=2), dict(B=0), dict(T=0), dict(C=0), dict(n_new=0),
               dict(n_cand=-1), dict(x=None), dict(dist=None), dict(new=None), dict(cand=None), dict(B=65536), dict(T=65536),
               dict(C=1 << 20, H=1 << 6, W=1 << 6, L=1), dict(x=p + 2)):
        assert rows(**kw) == E_SHAPE, kw

    def fps(dist=p, B=2, T=8, cand=p, n_cand=5, forced=p, n_forced=1, n=3, picks=p):
        return lib.lfvdm_fps_select(dist, B, T, cand, n_cand, forced, n_forced, n, picks, None)
    for kw in (dict(B=0), dict(T=0), dict(n_cand=0), dict(n_forced=0), dict(n=0), dict(dist=None), dict(cand=None),
               dict(forced=None), dict(picks=None), dict(T=65536)):
        assert fps(**kw) == E_SHAPE, kw
    assert fps(n_cand=4097, T=5000) == E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ metric
def test_parse_frame_metric():
    from improved_diffusion.frame_select import parse_frame_metric
    assert [parse_frame_metric(f"msl2:{k}") for k in (1, 2, 3)] == [1, 2, 3]
    assert parse_frame_metric(" msl2:2 ") == 2
    for bad in ("msl2", "msl2:", "msl2:0", "msl2:4", "msl2:1.0", "l2:1", "lpips", "", "msl2:1:2", None, 2, "MSL2:1"):
        with pytest.raises(ValueError, match="msl2"):
            parse_frame_metric(bad)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_reference_equals_pooling_composed_by_hand(L):
    from improved_diffusion.frame_select import frame_distance_reference
    torch.manual_seed(L)
    a, b = torch.randn(2, 5, 3, 12, 20), torch.randn(2, 5, 3, 12, 20)
    got = frame_distance_reference(a, b, L)
    assert got.dtype == torch.float64 and got.shape == (2, 5)
    d = (a.double() - b.double()).reshape(10, 3, 12, 20)
    want = (d ** 2).mean(dim=(1, 2, 3))
    if L >= 2:
        want = want + (F.avg_pool2d(d, 2) ** 2).mean(dim=(1, 2, 3))
    if L >= 3:
        want = want + (F.avg_pool2d(F.avg_pool2d(d, 2), 2) ** 2).mean(dim=(1, 2, 3))
    torch.testing.assert_close(got.reshape(10), want / L, rtol=1e-13, atol=0)
    # and with the pooling written as a block mean, no library pooling at all
    k = 1 << (L - 1)
    blk = d.reshape(10, 3, 12 // k, k, 20 // k, k).mean(dim=(3, 5))
    top = (blk ** 2).mean(dim=(1, 2, 3))
    lv = frame_distance_reference(a, b, L) * L - (frame_distance_reference(a, b, L - 1) * (L - 1) if L > 1 else 0)
    torch.testing.assert_close(lv.reshape(10), top, rtol=1e-12, atol=0)
    # msl2:1 is the plain mean squared difference; broadcasting a frame against many; zero for equal frames
    torch.testing.assert_close(frame_distance_reference(a, b, 1), ((a.double() - b.double()) ** 2).mean(dim=(2, 3, 4)), rtol=1e-14, atol=0)
    assert frame_distance_reference(a[:, :1], a, L).shape == (2, 5) and float(frame_distance_reference(a, a, L).abs().max()) == 0.0


def test_indivisible_frames_are_refused_naming_the_largest_usable_level():
    from improved_diffusion.frame_select import FrameDistanceCache, frame_distance_reference, frame_distances
    a = torch.zeros(1, 2, 3, 6, 8)
    with pytest.raises(ValueError, match=r"largest usable L is 2"):
        frame_distance_reference(a, a, 3)
    with pytest.raises(ValueError, match=r"largest usable L is 1"):
        frame_distances(torch.zeros(1, 2, 3, 7, 8), [0], [1], 2)
    with pytest.raises(ValueError, match=r"largest usable L is 1"):
        frame_distances(torch.zeros(1, 2, 3, 8, 5), [0], [1], 3)
    assert frame_distances(a, [0], [1], 2).shape == (1, 2, 2)
    for bad in (0, 4, 1.0, True, "2"):
        with pytest.raises(ValueError):
            frame_distance_reference(a, a, bad)
        with pytest.raises(ValueError):
            FrameDistanceCache(bad)
    with pytest.raises(ValueError, match="outside"):
        frame_distances(a, [2], [0], 1)
    with pytest.raises(ValueError, match="outside"):
        frame_distances(a, [0], [-1], 1)
    with pytest.raises(ValueError):
        frame_distances(torch.zeros(2, 3, 4, 4), [0], [1], 1)
    with pytest.raises(ValueError, match="out must be"):
        frame_distances(a, [0], [1], 1, out=torch.zeros(1, 2, 2))          # the CPU matrix is float64


def test_cpu_frame_distances_footprint_symmetry_and_vectors():
    from improved_diffusion.frame_select import frame_distance_reference, frame_distances
    v = walk(2, 12, 4, 8, 8, 0)
    new, cand = [7, 2, 9], [0, 9, 4, 4]                                     # unsorted, overlapping, repeated
    dist = frame_distances(v, new, cand, 3)
    assert dist.dtype == torch.float64 and dist.shape == (2, 12, 12)
    want = torch.full((2, 12, 12), float("nan"), dtype=torch.float64)
    for i in new:
        for j in new + cand:
            want[:, i, j] = want[:, j, i] = frame_distance_reference(v[:, i], v[:, j], 3)
    torch.testing.assert_close(dist, want, rtol=1e-13, atol=0, equal_nan=True)
    assert torch.equal(torch.isnan(dist), torch.isnan(want))
    assert all(float(dist[:, i, i].abs().max()) == 0.0 for i in new)
    assert torch.equal(dist.nan_to_num(-1.0), dist.transpose(1, 2).nan_to_num(-1.0))
    # generic vectors: (B, T, D) is C = D, H = W = 1
    vec = v.flatten(2)
    torch.testing.assert_close(frame_distances(vec, new, cand, 1), frame_distances(v, new, cand, 1), rtol=1e-13, atol=0, equal_nan=True)
    with pytest.raises(ValueError, match="largest usable L is 1"):
        frame_distances(vec, new, cand, 2)


# ------------------------------------------------------------------------------------------------ selection
SELECT_CASES = [  # (name, cand builder, n, forced positions)
    ("reversed", lambda T: list(range(T - 1, -1, -1)), 10, [0]),
    ("forced-3", lambda T: list(range(T)), 10, [5, 0, 17]),
    ("forced-all", lambda T: list(range(0, T, 2)), 4, [3, 1, 2, 0]),
    ("more-picks-than-candidates", lambda T: [9, 3, 30, 12], 7, [1]),
    ("one-candidate", lambda T: [11], 3, [0]),
    ("forced-longer-than-n", lambda T: list(range(T)), 2, [4, 6, 8]),
]


@pytest.mark.parametrize("shape,L,seed", [((3, 4, 4), 1, 0), ((4, 16, 16), 3, 1)], ids=["3x4x4-L1", "4x16x16-L3"])
@pytest.mark.parametrize("case", SELECT_CASES, ids=lambda c: c[0])
def test_cpu_selection_equals_the_schemes_host_loop(case, shape, L, seed):
    """farthest_point_select on the CPU matrix against AdaptiveSamplingSchemeBase.select_obs_indices as it stands, fed an
    embedding whose squared distances are D x the metric: the identity for L = 1; for L levels the concatenation of the
    pooled frames scaled by 2^l (sum over D / 4^l pooled elements of (2^l p)^2 = D x that level's mean)."""
    from improved_diffusion.frame_select import frame_distances, farthest_point_select
    _, build, n, forced = case
    B, T = 2, 40
    v = walk(B, T, *shape, seed)
    cand = build(T)
    D = int(np.prod(shape))
    ref = full_reference(B, T, *shape, seed, L)
    want = [select_with_margin(ref[b].numpy(), cand, n, forced, rel_bound(D, L))[0] for b in range(B)]
    dist = frame_distances(v, cand, [], L)
    got = farthest_point_select(dist, cand, n, forced)
    assert got == want

    def embed(vids, idx):
        fr = [vids[:, i] for i in idx]
        return torch.stack([torch.cat([(F.avg_pool2d(f, 1 << lv) if lv else f).flatten(1) * 2.0 ** lv for lv in range(L)], dim=1)
                            for f in fr], dim=1)
    sch = make_scheme("adaptive-autoreg", T, 4, 10, 5)
    sch.set_embed_fn(embed)
    sch.set_videos(v)
    assert sch.select_obs_indices(cand, n, always_selected=forced) == got
    if L == 1:
        sch2 = make_scheme("adaptive-autoreg", T, 4, 10, 5)
        sch2.set_embed_fn(identity_embed)
        sch2.set_videos(v)
        assert sch2.select_obs_indices(cand, n, always_selected=forced) == got


def test_selection_refusals_and_ties():
    from improved_diffusion.frame_select import farthest_point_select
    d = torch.zeros(1, 6, 6, dtype=torch.float64)
    for kw in (dict(cand=[]), dict(forced=[]), dict(n=0), dict(forced=[6]), dict(forced=[-1]), dict(cand=[0, 6])):
        a = dict(dict(cand=[0, 1, 2, 3, 4, 5], n=3, forced=[0]), **kw)
        with pytest.raises(ValueError):
            farthest_point_select(d, a["cand"], a["n"], a["forced"])
    with pytest.raises(ValueError):
        farthest_point_select(torch.zeros(6, 6), [0], 1)
    # constructed ties: frames 2 and 4 are equally far from frame 0, the lowest POSITION wins
    d[0, 0, 2] = d[0, 2, 0] = d[0, 0, 4] = d[0, 4, 0] = 5.0
    d[0, 2, 4] = d[0, 4, 2] = 1.0
    assert farthest_point_select(d, [0, 1, 2, 3, 4, 5], 2) == [[0, 2]]
    assert farthest_point_select(d, [0, 5, 4, 3, 2, 1], 2) == [[0, 4]]
    assert farthest_point_select(d, [0, 1, 2], 5) == [[0, 2, 0, 0, 0]]     # all picked: argmax of zeros is position 0


# ------------------------------------------------------------------------------------------------ schemes
SCHEME_CASES = [("adaptive-autoreg", 40, 4, 10, 5, 0), ("adaptive-hierarchy-2", 48, 4, 10, 5, 1)]


@pytest.mark.parametrize("name,T,n_obs,K,step,seed", SCHEME_CASES, ids=[c[0] for c in SCHEME_CASES])
def test_schemes_with_the_metric_equal_the_identity_embedding(name, T, n_obs, K, step, seed):
    shape, B = (3, 4, 4), 2
    v = walk(B, T, *shape, seed)
    ref = full_reference(B, T, *shape, seed, 1)
    old = make_scheme(name, T, n_obs, K, step)
    old.set_embed_fn(identity_embed)
    want = run_adaptive(old, v)
    new = make_scheme(name, T, n_obs, K, step)
    new.set_frame_metric("msl2:1")
    margins = []
    got = run_adaptive(new, v, margin_checker(ref, rel_bound(int(np.prod(shape)), 1), margins))
    print(f"[frame select {name}] {len(got)} windows, {len(margins)} margin checks, worst margin {min(margins):.2e}")
    assert got == want and len(got) > 4 and margins
    assert any(o[0] != o[1] for o, _ in got), "the videos differ, so should some of their conditioning frames"


def test_metric_and_embed_fn_exclude_each_other():
    s = make_scheme("adaptive-autoreg", 20, 2, 6, 2)
    s.set_frame_metric("msl2:2")
    with pytest.raises(ValueError, match="not both"):
        s.set_embed_fn(identity_embed)
    s = make_scheme("adaptive-hierarchy-2", 20, 2, 6, 2)
    s.set_embed_fn(identity_embed)
    with pytest.raises(ValueError, match="not both"):
        s.set_frame_metric("msl2:1")
    with pytest.raises(ValueError, match="msl2"):
        make_scheme("adaptive-autoreg", 20, 2, 6, 2).set_frame_metric("lpips")
    from improved_diffusion.sampling_schemes import sampling_schemes
    assert not hasattr(sampling_schemes["autoreg"], "set_frame_metric")


def test_cache_filled_window_by_window_equals_one_filled_at_once():
    from improved_diffusion.frame_select import FrameDistanceCache, frame_distance_reference
    v = walk(2, 20, 4, 8, 8, 2)
    inc, once = FrameDistanceCache(2), FrameDistanceCache(2)
    done = set()
    for grow in ([3, 0, 1], [10, 11], [], [19, 5, 6, 7], [2]):
        done |= set(grow)
        d = inc.update(v, done)
        assert sorted(inc.cached) == sorted(done)
    full = once.update(v, sorted(done, reverse=True))
    torch.testing.assert_close(d, full, rtol=1e-13, atol=0, equal_nan=True)
    idx = sorted(done)
    want = frame_distance_reference(v[:, idx][:, :, None], v[:, idx][:, None, :], 2)
    torch.testing.assert_close(d[:, idx][:, :, idx], want, rtol=1e-13, atol=0)
    rest = [i for i in range(20) if i not in done]
    assert bool(torch.isnan(d[:, rest]).all()) and bool(torch.isnan(d[:, :, rest]).all())
    # another tensor (data_ptr), another shape: it starts over
    assert inc.update(v.clone(), [0, 1]) is not d and inc.cached == [0, 1]
    assert inc.update(v[:, :10].contiguous(), [4]).shape == (2, 10, 10) and inc.cached == [4]
    with pytest.raises(ValueError, match="4096"):
        FrameDistanceCache(1).update(torch.zeros(1, 4097, 1), [0])


# ------------------------------------------------------------------------------------------------ sample_video
def _check_windows(used, B, T, n_obs, K):
    done = set(range(n_obs))
    for obs, lat in used:
        assert len(obs) == B and len(lat) == B and all(list(l) == list(lat[0]) for l in lat)
        assert not (set(lat[0]) & done), "every frame is generated exactly once"
        for b in range(B):
            assert len(obs[b]) + len(lat[b]) <= K and set(int(i) for i in obs[b]) <= done, "conditions only on finished frames"
        done |= set(int(i) for i in lat[0])
    assert done == set(range(T))


@pytest.mark.parametrize("scheme", ADAPTIVE)
def test_sample_video_runs_the_adaptive_schemes_with_a_metric_and_no_lpips(scheme, monkeypatch):
    """Fails on the parent commit with ImportError('adaptive sampling schemes need the `lpips` package ...')."""
    from improved_diffusion.video_sampler import default_sampling_args, sample_video
    monkeypatch.setitem(sys.modules, "lpips", None)                    # importing it raises ImportError, installed or not
    B, T, n_obs, K, step = 2, 40, 6, 10, 5                              # 6 observed frames: the first window has 5 to choose
    truth = walk(B, T, 4, 8, 8, 3)
    args = default_sampling_args(sampling_scheme=scheme, n_obs=n_obs, max_frames=K, max_latent_frames=step, device="cpu",
                                 adaptive_metric="msl2:3")
    with contextlib.redirect_stdout(io.StringIO()):
        samples, used = sample_video(args, None, None, truth, just_get_indices=True, verbose=False)
    assert torch.equal(samples, truth)
    _check_windows(used, B, T, n_obs, K)
    if scheme == "adaptive-autoreg":
        done = set(range(n_obs))
        for obs, lat in used:
            assert all(int(o[0]) == max(done) for o in obs), "each video's first conditioning frame is the most recent one"
            assert all(len(set(o)) == K - step for o in obs)
            done |= set(lat[0])
    assert any(list(o[0]) != list(o[1]) for o, _ in used)


def test_without_a_metric_the_lpips_fallback_stays_and_points_to_the_option(monkeypatch):
    from improved_diffusion.video_sampler import default_sampling_args, sample_video
    monkeypatch.setitem(sys.modules, "lpips", None)
    monkeypatch.delenv("LFVDM_ADAPTIVE_METRIC", raising=False)
    truth = walk(2, 40, 4, 8, 8, 3)
    args = default_sampling_args(sampling_scheme="adaptive-autoreg", n_obs=4, max_frames=10, max_latent_frames=5, device="cpu")
    assert args.adaptive_metric is None
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(ImportError, match="adaptive_metric"):
        sample_video(args, None, None, truth, just_get_indices=True, verbose=False)


def test_sample_video_metric_option_environment_and_refusals(monkeypatch):
    from types import SimpleNamespace
    from improved_diffusion.video_sampler import default_sampling_args, resolve_adaptive_metric, sample_video
    monkeypatch.setitem(sys.modules, "lpips", None)
    monkeypatch.delenv("LFVDM_ADAPTIVE_METRIC", raising=False)
    assert resolve_adaptive_metric(SimpleNamespace()) is None
    truth = walk(2, 40, 4, 8, 8, 3)
    kw = dict(n_obs=4, max_frames=10, max_latent_frames=5, device="cpu")
    with contextlib.redirect_stdout(io.StringIO()):
        _, by_arg = sample_video(default_sampling_args(sampling_scheme="adaptive-hierarchy-2", adaptive_metric="msl2:2", **kw),
                                 None, None, truth, just_get_indices=True, verbose=False)
        monkeypatch.setenv("LFVDM_ADAPTIVE_METRIC", "msl2:2")
        assert resolve_adaptive_metric(SimpleNamespace()) == "msl2:2"
        assert resolve_adaptive_metric(SimpleNamespace(adaptive_metric="msl2:1")) == "msl2:1"      # the argument wins
        _, by_env = sample_video(default_sampling_args(sampling_scheme="adaptive-hierarchy-2", **kw), None, None, truth,
                                 just_get_indices=True, verbose=False)
    assert by_env == by_arg
    # a metric with a non-adaptive scheme, from either source
    for a in (default_sampling_args(sampling_scheme="autoreg", **kw),
              default_sampling_args(sampling_scheme="hierarchy-2", adaptive_metric="msl2:1", **kw)):
        with pytest.raises(ValueError, match="adaptive"):
            sample_video(a, None, None, truth, just_get_indices=True, verbose=False)
    monkeypatch.setenv("LFVDM_ADAPTIVE_METRIC", "lpips")
    with pytest.raises(ValueError, match="msl2"):
        sample_video(default_sampling_args(sampling_scheme="adaptive-autoreg", **kw), None, None, truth, just_get_indices=True,
                     verbose=False)
    monkeypatch.delenv("LFVDM_ADAPTIVE_METRIC")
    # frames that do not fit the levels
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(ValueError, match="largest usable L is 2"):
        sample_video(default_sampling_args(sampling_scheme="adaptive-autoreg", adaptive_metric="msl2:3", **kw), None, None,
                     walk(1, 40, 3, 6, 6, 0), just_get_indices=True, verbose=False)
