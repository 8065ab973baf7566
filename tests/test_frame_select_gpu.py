"""Frame distances and farthest-point selection on the MI355X (csrc/frame_select.hip through the binding and through
improved_diffusion/frame_select.py): distance rows against the float64 reference within the bound of
test_frame_select_cpu.py ((D + 2 + (2^L)^2) 2^-24 relative, D <= 1025 so that a dropped or doubled element is far above it);
the footprint inside a NaN-filled matrix with guard bands; bitwise symmetry, reproducibility, independence of launch, tile
and list position, scalar against vector loads; the selection launch against the host loop on the SAME matrix (exact, ties
and NaN included); the schemes on the device against the CPU on margin-checked videos; sample_video on the device."""
import contextlib
import io

import numpy as np
import pytest
import torch

from test_frame_select_cpu import (SCHEME_CASES, _check_windows, full_reference, make_scheme, margin_checker, rel_bound,
                                   run_adaptive, walk)

pytestmark = pytest.mark.gpu

NAN = float("nan")
T_ROWS = 150
GUARD = 4096


def bits(t):
    return t.contiguous().view(torch.int32)


def rows_reference(v, new, tgt, L):
    """(B, n_new, n_tgt) float64 on the CPU."""
    from improved_diffusion.frame_select import frame_distance_reference
    v5 = v if v.dim() == 5 else v[..., None, None]
    return torch.stack([frame_distance_reference(v5[:, tgt], v5[:, i:i + 1], L) for i in new], dim=1)


def lists(T, n_new, n_cand, order, seed):
    """Disjoint new / cand lists of distinct frames; order: sorted, reversed, shuffled, or overlapping (cand also holds
    half of new and repeats an entry)."""
    rng = np.random.RandomState(seed)
    perm = rng.permutation(T)[:n_new + n_cand].tolist()
    new, cand = sorted(perm[:n_new]), sorted(perm[n_new:])
    if order == "reversed":
        new, cand = new[::-1], cand[::-1]
    elif order == "shuffled":
        new, cand = perm[:n_new], perm[n_new:]
    elif order == "overlapping":
        cand = (perm[n_new:n_new + n_cand - n_new // 2 - 1] + new[:n_new // 2] + perm[n_new:n_new + 1])[:n_cand]
        rng.shuffle(cand)
        assert len(cand) == n_cand
    return new, cand


def launch_rows(v, new, cand, L):
    """lfvdm_frame_dist_rows through the binding into a NaN matrix between NaN guard bands -> dist (B, T, T), the bands."""
    from improved_diffusion import _native as nat
    v5 = v if v.dim() == 5 else v[..., None, None]
    B, T, C, H, W = v5.shape
    buf = torch.full((B * T * T + 2 * GUARD,), NAN, device="cuda")
    dist = buf[GUARD:GUARD + B * T * T].view(B, T, T)
    idx = torch.tensor(new + cand, dtype=torch.int32, device="cuda")
    nat.frame_dist_rows(v5, B, T, C, H, W, L, idx[:len(new)], idx[len(new):] if cand else None, dist)
    torch.cuda.synchronize()
    return dist, (buf[:GUARD], buf[GUARD + B * T * T:])


def check_rows(tag, v, new, cand, L):
    dist, guards = launch_rows(v.cuda(), new, cand, L)
    B, T = v.shape[:2]
    D = v[0, 0].numel()
    tgt = new + cand
    ref = rows_reference(v, new, tgt, L)
    got = dist.cpu()
    written = torch.zeros(T, T, dtype=torch.bool)
    worst = 0.0
    for a, i in enumerate(new):
        for c, j in enumerate(tgt):
            written[i, j] = written[j, i] = True
            g = got[:, i, j].double()
            if i == j:
                assert bool((g == 0).all()) and bool((got[:, j, i] == 0).all()), (tag, i)
                continue
            assert bool((ref[:, a, c] > 0).all())
            worst = max(worst, float(((g - ref[:, a, c]).abs() / ref[:, a, c]).max()))
    bound = rel_bound(D, L)
    print(f"[frame dist {tag}] B={B} D={D} L={L} n_new={len(new)} n_cand={len(cand)}: worst rel err {worst:.2e} "
          f"({worst / bound:.3f} of the bound {bound:.2e})")
    assert worst <= bound
    assert torch.equal(~torch.isnan(got), written.expand(B, T, T)), "exactly the specified entries are written"
    assert all(bool(torch.isnan(g).all()) for g in guards), "nothing outside the matrix is written"
    assert torch.equal(bits(dist), bits(dist.transpose(1, 2))), "d(i, j) and d(j, i) are the same bits"
    return dist


# (C, H, W, L) of the issue and the two generic-vector sizes, each with its own batch size, list sizes and list order;
# between them they cover B in 1..3, n_new in {1, 3, 17}, n_cand in {1, 33, 130} and every order
ROW_CASES = [
    ((3, 4, 4), 1, 1, 1, 130, "reversed"),
    ((4, 16, 16), 3, 3, 17, 33, "shuffled"),
    ((3, 12, 20), 3, 2, 3, 130, "overlapping"),
    ((5, 7, 9), 1, 3, 17, 1, "sorted"),
    ((1, 2, 2), 2, 2, 3, 33, "shuffled"),
    ((1,), 1, 3, 17, 130, "overlapping"),
    ((1025,), 1, 2, 1, 1, "reversed"),
]


def case_videos(shape, B, seed=0):
    dims = shape if len(shape) == 3 else (shape[0], 1, 1)
    v = walk(B, T_ROWS, *dims, seed)
    return v if len(shape) == 3 else v.flatten(2)


@pytest.mark.parametrize("shape,L,B,n_new,n_cand,order", ROW_CASES, ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c))
def test_distance_rows_match_the_float64_reference(shape, L, B, n_new, n_cand, order):
    v = case_videos(shape, B)
    new, cand = lists(T_ROWS, n_new, n_cand, order, seed=n_new + n_cand)
    check_rows(f"{shape} {order}", v, new, cand, L)


def test_distance_rows_every_list_size_and_no_candidates():
    v = case_videos((4, 8, 8), 2)
    for n_new in (1, 3, 17):
        for n_cand in (1, 33, 130):
            new, cand = lists(T_ROWS, n_new, n_cand, "shuffled", seed=n_new * n_cand)
            check_rows("4x8x8 sizes", v, new, cand, 2)
    check_rows("4x8x8 no candidates", v, [5, 140, 7, 5], [], 3)


def test_distance_rows_through_the_module_equal_the_binding():
    from improved_diffusion.frame_select import frame_distances
    for shape, L in (((4, 16, 16), 3), ((1025,), 1)):
        v = case_videos(shape, 2)
        new, cand = lists(T_ROWS, 17, 33, "overlapping", seed=3)
        want, _ = launch_rows(v.cuda(), new, cand, L)
        got = frame_distances(v.cuda(), new, cand, L)
        assert got.is_cuda and got.dtype == torch.float32 and torch.equal(bits(got), bits(want))
        # the CPU path: the same footprint, the same values within the bound
        cpu = frame_distances(v, new, cand, L)
        assert torch.equal(torch.isnan(cpu), torch.isnan(got.cpu()))
        err = ((got.cpu().double() - cpu).abs() / cpu.clamp_min(1e-300)).nan_to_num(0.0)
        assert float(err.max()) <= rel_bound(v[0, 0].numel(), L)


def test_bitwise_reproducible_and_independent_of_launch_tile_and_position():
    """The same pair computed by another launch, in another tile, at another list position, as (i, j) or as (j, i), with
    vector or with scalar loads: the same bits.  An incremental fill equals a one-shot fill."""
    from improved_diffusion.frame_select import FrameDistanceCache, frame_distances
    for shape, L in (((4, 16, 16), 3), ((3, 12, 20), 2), ((5, 7, 9), 1)):
        v = case_videos(shape, 2).cuda()
        frames = lists(T_ROWS, 40, 0, "shuffled", seed=L)[0]
        a = frame_distances(v, frames, [], L)
        b = frame_distances(v, frames, [], L)
        assert torch.equal(bits(a), bits(b)), "two runs"
        c = frame_distances(v, frames[::-1], [], L)
        assert torch.equal(bits(a), bits(c)), "reversed lists: other tiles, other slots"
        d = frame_distances(v, frames[:7], frames[7:], L)
        e = frame_distances(v, frames[7:][::-1], frames[:7], L, out=d)
        assert e is d and torch.equal(bits(a), bits(d)), "split into new and cand, then the rest"
        inc, done = FrameDistanceCache(L), []
        for k in (3, 1, 10, 17, 9):
            done = done + frames[len(done):len(done) + k]
            m = inc.update(v, done)
        assert sorted(inc.cached) == sorted(frames) and torch.equal(bits(m), bits(a)), "incremental against one-shot"
        # the same videos one float off a 16-byte boundary: scalar loads, the same bits
        buf = torch.zeros(v.numel() + 1, device="cuda")
        off = buf[1:].view(v.shape)
        off.copy_(v)
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        assert torch.equal(bits(frame_distances(off, frames, [], L)), bits(a)), "scalar against vector loads"


def test_module_refusals_on_the_device():
    from improved_diffusion.frame_select import frame_distances
    v = case_videos((4, 8, 8), 2).cuda()
    with pytest.raises(ValueError, match="float32"):
        frame_distances(v.double(), [0], [1], 1)
    with pytest.raises(ValueError, match="strided"):
        frame_distances(v.transpose(3, 4), [0], [1], 1)
    with pytest.raises(ValueError, match="out must be"):
        frame_distances(v, [0], [1], 1, out=torch.zeros(2, T_ROWS, T_ROWS, dtype=torch.float64, device="cuda"))


# ------------------------------------------------------------------------------------------------ selection
def host_loop(dist, cand, n, forced):
    """The scheme's host loop on the device's own matrix -> positions per video."""
    from improved_diffusion.frame_select import _host_select
    sub = dist.cpu()[:, cand][:, :, cand].numpy()
    return [_host_select(lambda p, b=b: sub[b, p], len(cand), n, list(forced)[:n]) for b in range(sub.shape[0])]


def launch_fps(dist, cand, n, forced):
    from improved_diffusion import _native as nat
    B, T = dist.shape[:2]
    ci = torch.tensor(cand, dtype=torch.int32, device="cuda")
    fi = torch.tensor(forced, dtype=torch.int32, device="cuda")
    buf = torch.full((B * n + 2 * 64,), -7, dtype=torch.int32, device="cuda")
    picks = buf[64:64 + B * n].view(B, n)
    nat.fps_select(dist, B, T, ci, fi, n, picks)
    torch.cuda.synchronize()
    assert bool((buf[:64] == -7).all()) and bool((buf[64 + B * n:] == -7).all())
    return picks.cpu().tolist()


def sym_matrix(B, T, seed, levels=None):
    """Random symmetric (B, T, T) float32 with a zero diagonal; ``levels``: values quantised to that many levels (ties)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(B, T, T, generator=g)
    if levels:
        m = torch.floor(m * levels) / levels
    m = torch.triu(m, 1)
    return (m + m.transpose(1, 2)).contiguous().cuda()


FPS_CASES = [  # (B, T, n_cand, n, forced, tie levels)
    (1, 1000, 1000, 12, [0], None),
    (3, 1000, 1000, 10, [999, 0, 500], 3),
    (2, 300, 257, 9, [256], None),
    (2, 300, 257, 6, [5, 4, 3, 2, 1, 0], 2),
    (3, 300, 257, 40, [7], 4),
    (2, 40, 5, 9, [2], None),          # n > n_cand
    (3, 40, 1, 4, [0], None),
    (1, 40, 1, 1, [0], None),
    (2, 40, 30, 3, [1, 2, 3, 4, 5], 2),     # more forced positions than picks
]


@pytest.mark.parametrize("B,T,n_cand,n,forced,levels", FPS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_selection_launch_equals_the_host_loop_on_the_same_matrix(B, T, n_cand, n, forced, levels):
    from improved_diffusion.frame_select import farthest_point_select
    dist = sym_matrix(B, T, seed=n_cand + n, levels=levels)
    cand = np.random.RandomState(n).permutation(T)[:n_cand].tolist()
    want = host_loop(dist, cand, n, forced)
    got = launch_fps(dist, cand, n, forced)
    assert got == want
    if levels:
        assert any(len(set(r)) > 1 for r in want)
    frames = farthest_point_select(dist, cand, n, forced)
    assert frames == [[cand[p] for p in r] for r in want]
    assert farthest_point_select(dist.cpu().double(), cand, n, forced) == frames


def test_selection_constructed_ties_and_nan():
    dist = torch.zeros(2, 8, 8, device="cuda")
    for i, j, val in ((0, 2, 5.0), (0, 4, 5.0), (0, 6, 5.0), (2, 4, 1.0), (2, 6, 3.0), (4, 6, 3.0)):
        dist[:, i, j] = dist[:, j, i] = val
    for cand in ([0, 1, 2, 3, 4, 5, 6, 7], [0, 7, 6, 5, 4, 3, 2, 1], [4, 6, 0, 2]):
        want = host_loop(dist, cand, 4, [cand.index(0)])
        assert launch_fps(dist, cand, 4, [cand.index(0)]) == want
        assert want[0][1] == min(cand.index(2), cand.index(4), cand.index(6)), "the lowest position of the maximum"
    # numpy's treatment of NaN: np.minimum propagates it, np.argmax returns the first one
    dist[1, 0, 5] = dist[1, 5, 0] = NAN
    cand = list(range(8))
    want = host_loop(dist, cand, 5, [0])
    assert launch_fps(dist, cand, 5, [0]) == want and want[1][1] == 5
    # positions and frames that cannot be used end the selection with -1, and nothing is read through them
    assert launch_fps(dist, [0, 2, 4], 4, [0, 3]) == [[0, -1, -1, -1]] * 2
    assert launch_fps(dist, [0, 9, 4], 3, [1]) == [[1, -1, -1]] * 2


# ------------------------------------------------------------------------------------------------ schemes, sample_video
@pytest.mark.parametrize("name,T,n_obs,K,step,seed", SCHEME_CASES, ids=[c[0] for c in SCHEME_CASES])
@pytest.mark.parametrize("shape,L", [((3, 4, 4), 1), ((4, 16, 16), 3)], ids=["3x4x4-L1", "4x16x16-L3"])
def test_schemes_on_the_device_equal_the_cpu(name, T, n_obs, K, step, seed, shape, L):
    B = 2
    v = walk(B, T, *shape, seed)
    ref = full_reference(B, T, *shape, seed, L)
    cpu = make_scheme(name, T, n_obs, K, step)
    cpu.set_frame_metric(f"msl2:{L}")
    margins = []
    want = run_adaptive(cpu, v, margin_checker(ref, rel_bound(int(np.prod(shape)), L), margins))
    dev = make_scheme(name, T, n_obs, K, step)
    dev.set_frame_metric(f"msl2:{L}")
    got = run_adaptive(dev, v.cuda())
    print(f"[frame select device {name} L={L}] {len(got)} windows, worst margin {min(margins):.2e}")
    assert got == want and len(got) > 4
    assert dev._dist_cache.dist.is_cuda and sorted(dev._dist_cache.cached) == sorted(cpu._dist_cache.cached)


def test_sample_video_on_the_device_with_adaptive_hierarchy(monkeypatch):
    import sys
    from improved_diffusion.video_sampler import default_sampling_args, sample_video
    monkeypatch.setitem(sys.modules, "lpips", None)
    B, T, n_obs, K, step = 2, 48, 4, 10, 5
    truth = walk(B, T, 4, 16, 16, 1)
    args = default_sampling_args(sampling_scheme="adaptive-hierarchy-2", n_obs=n_obs, max_frames=K, max_latent_frames=step,
                                 device="cuda", adaptive_metric="msl2:3")
    with contextlib.redirect_stdout(io.StringIO()):
        samples, used = sample_video(args, None, None, truth, just_get_indices=True, verbose=False)
    assert torch.equal(samples, truth)
    _check_windows(used, B, T, n_obs, K)
    # the same windows as the scheme driven by hand over the finished video (margin-checked against the float64 reference)
    ref = full_reference(B, T, 4, 16, 16, 1, 3)
    cpu = make_scheme("adaptive-hierarchy-2", T, n_obs, K, step)
    cpu.set_frame_metric("msl2:3")
    want = run_adaptive(cpu, truth, margin_checker(ref, rel_bound(1024, 3)))
    assert [([[int(i) for i in o] for o in obs], [int(i) for i in lat[0]]) for obs, lat in used] == want
    # a permuted but dense batch (channels-last storage): zeros_like would keep its strides; the metric path allocates row-major
    strided = truth.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    assert not strided.is_contiguous() and torch.equal(strided, truth)
    for b in (strided, strided.cuda()):
        with contextlib.redirect_stdout(io.StringIO()):
            samples2, used2 = sample_video(args, None, None, b, just_get_indices=True, verbose=False)
        assert torch.equal(samples2.cpu(), truth) and used2 == used
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(ValueError, match="float32"):
        sample_video(args, None, None, truth.double(), just_get_indices=True, verbose=False)
