"""The bouncing_shapes kernels on the MI355X against the host reference - every comparison BITWISE - and the dataset through
TrainLoop, sample_video and prediction_metrics.  The dataset seed (0) was chosen on the CPU reference so that the cases are
not vacuous; each test asserts from the reference what it relies on (bounces on all four walls, a re-draw, overlapping shapes)."""
import argparse
import functools

import numpy as np
import pytest
import torch

from oracle import recipe, unet_oracle as uo
from test_forward_gpu import build_native

pytestmark = pytest.mark.gpu

SEED = 0


def _sh():
    from improved_diffusion import shapes
    return shapes


def _source(params, split="train", batch_size=1, **kw):
    sh = _sh()
    return sh.ShapesBatches(sh.BouncingShapes(params, split, **kw), batch_size).device_source


@functools.lru_cache(maxsize=None)
def _reference(H, W, S, T, stochastic, split, items):
    """(traj, consts, bounced, uint8 videos) of dataset items (shard 0 of 1: item = video index), computed once per case."""
    sh = _sh()
    p = sh.ShapesParams(H=H, W=W, n_shapes=S, T=T, stochastic=stochastic, seed=SEED)
    traj, consts, bounced = sh.trajectories_ref(p, split, list(items), return_events=True)
    videos = np.stack([sh.render_ref(traj[n], consts[n], H, W) for n in range(len(items))])
    for a in (traj, consts, bounced, videos):
        a.setflags(write=False)
    return p, traj, consts, bounced, videos


def _walls_hit(p, traj, consts, bounced):
    rad = consts[..., 1][:, None, :]
    hit = set()
    for axis, L in ((0, p.W), (1, p.H)):
        pos, b = traj[..., axis], bounced[..., axis]
        # a reflected centre lies within one step (48) of the wall it came off; the walls are >= 128 apart
        hit |= {(axis, "low")} if (b & (pos - rad <= 48)).any() else set()
        hit |= {(axis, "high")} if (b & (16 * L - rad - pos <= 48)).any() else set()
    return hit


def _boxes_overlap(traj, consts):
    S = traj.shape[2]
    t = traj.astype(np.int64)
    for i in range(S):
        for j in range(i + 1, S):
            rr = (consts[:, i, 1] + consts[:, j, 1])[:, None]
            if ((abs(t[:, :, i, 0] - t[:, :, j, 0]) < rr) & (abs(t[:, :, i, 1] - t[:, :, j, 1]) < rr)).any():
                return True
    return False


@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_trajectory_table(S, stochastic):
    p, traj, consts, bounced, _ = _reference(16, 16, S, 40, stochastic, "train", (0, 1, 2))
    assert len(_walls_hit(p, traj, consts, bounced)) == 4, "the case must bounce off every wall"
    if stochastic:
        still = _reference(16, 16, S, 40, False, "train", (0, 1, 2))[1]
        assert not np.array_equal(traj, still), "the case must contain a re-draw that changes the motion"
    src = _source(p)
    got_traj, got_consts = src.trajectories(torch.tensor([0, 1, 2], device="cuda"))
    assert got_traj.dtype == torch.int32 and got_traj.shape == (3, 40, S, 2) and got_consts.shape == (3, S, 4)
    assert torch.equal(got_traj.cpu(), torch.from_numpy(traj.copy()))
    assert torch.equal(got_consts.cpu(), torch.from_numpy(consts.copy()))
    # the test split is another stream
    other = _source(p, "test").trajectories(torch.tensor([0, 1, 2], device="cuda"))[0]
    assert torch.equal(other.cpu(), torch.from_numpy(_reference(16, 16, S, 40, stochastic, "test", (0, 1, 2))[1].copy()))
    assert not torch.equal(other, got_traj)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("H,W,S,T,items", [(16, 16, 3, 12, (0, 1)), (16, 24, 3, 12, (0, 1)), (24, 16, 3, 12, (0, 1)),
                                          (20, 12, 3, 12, (0, 1)), (64, 64, 2, 100, (5,))])
def test_whole_videos(H, W, S, T, items, dtype):
    sh = _sh()
    p, traj, consts, _, videos = _reference(H, W, S, T, True, "train", items)
    if S == 3:
        assert _boxes_overlap(traj, consts), "the case must paint one shape over another"
    got = _source(p).render(list(items), "cuda", dtype)
    assert got.shape == (len(items), T, 3, H, W) and got.dtype == dtype
    want = torch.from_numpy(videos.copy())
    assert torch.equal(got.cpu(), want if dtype == torch.uint8 else sh.uint8_to_float(want))
    assert len(np.unique(videos)) > 2                               # shapes, antialiased edges, background


def test_table_mode_is_render_plus_prepare_batch():
    """F = 5 slots out of T = 8: frames out of order and repeated, rows >= T (the padding video), rows outside [0, 2 T)
    (clamped).  The batch is the reference's frames, and batch, indices and masks are what lfvdm_prepare_batch makes of the
    same table on a pool of the reference videos."""
    from improved_diffusion import _native as nat
    sh = _sh()
    T, F = 8, 5
    p, _, _, _, videos = _reference(16, 24, 2, T, True, "train", (0, 1, 2, 3))
    items1, items2 = [0, 1], [2, 3]
    table = np.array([[[5, 5, 1, 0], [2, 2, 0, 1], [5, 5, 1, 0], [T + 6, 6, 0, 0], [99, 3, 1, 1]],
                      [[7, 7, 0, 1], [T + 0, 0, 1, 0], [T + 7, 7, 0, 0], [0, 0, 0, 1], [-4, 1, 1, 0]]], dtype=np.int32)
    rows = np.clip(table[:, :, 0], 0, 2 * T - 1)
    pool_u8 = torch.from_numpy(np.concatenate([videos[items1], videos[items2]], axis=1))        # (2, 2 T, 3, H, W)
    want_u8 = torch.stack([pool_u8[b, rows[b]] for b in range(2)])
    src = _source(p)
    for dtype in (torch.float32, torch.uint8):
        batch, fi, obs, lat = src.render_batch(torch.tensor(items1), torch.tensor(items2), table, "cuda", dtype)
        assert batch.shape == (2, F, 3, 16, 24) and batch.dtype == dtype
        assert torch.equal(batch.cpu(), want_u8 if dtype == torch.uint8 else sh.uint8_to_float(want_u8))
        if dtype == torch.float32:
            pool = sh.uint8_to_float(pool_u8).cuda()
            b2 = torch.empty_like(batch)
            fi2, obs2, lat2 = torch.empty_like(fi), torch.empty_like(obs), torch.empty_like(lat)
            nat.prepare_batch(pool, torch.from_numpy(table).cuda(), b2, fi2, obs2, lat2)
            assert torch.equal(batch, b2) and torch.equal(fi, fi2) and torch.equal(obs, obs2) and torch.equal(lat, lat2)
            assert fi.dtype == torch.int64 and obs.shape == (2, F, 1, 1, 1)
    # without the index / mask tensors (the wavelet pool)
    pool_only = src.render_table(torch.tensor([[0, 2], [1, 3]], device="cuda"), torch.from_numpy(table).cuda(), torch.uint8, masks=False)
    assert pool_only[1] is None and torch.equal(pool_only[0].cpu(), want_u8)


def test_both_launches_replay_in_a_captured_graph():
    sh = _sh()
    p, _, _, _, videos = _reference(16, 16, 3, 12, True, "train", (0, 1, 2, 3))
    src = _source(p)
    src.lut("cuda")
    table = np.zeros((2, 3, 4), dtype=np.int32)
    table[:, :, 0] = [[1, 12 + 4, 11], [0, 3, 12 + 11]]
    table[:, :, 1] = table[:, :, 0] % 12
    static_idx = torch.tensor([[0, 1], [2, 3]], device="cuda")
    static_table = torch.from_numpy(table).cuda()
    src.render_table(static_idx, static_table)                      # eager warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = src.render_table(static_idx, static_table)
    for pairs in ([[0, 1], [2, 3]], [[3, 0], [1, 2]]):
        static_idx.copy_(torch.tensor(pairs))
        g.replay()
        torch.cuda.synchronize()
        want = torch.stack([torch.from_numpy(np.concatenate([videos[a], videos[b]])[table[i, :, 0]]) for i, (a, b) in enumerate(pairs)])
        assert torch.equal(out[0].cpu(), sh.uint8_to_float(want)), pairs
        assert torch.equal(out[1].cpu(), torch.from_numpy(table[:, :, 1].astype(np.int64)))


# ---------------------------------------------------------------------------------------------------- TrainLoop
@functools.lru_cache(maxsize=None)
def _pixel_model():
    cfg = uo.make_cfg(in_channels=3, model_channels=32, num_res_blocks=1, channel_mult=(1, 2), attention_resolutions=(1, 2),
                      num_heads=2)
    sd = {k: torch.from_numpy(v) for k, v in recipe.fill_state_dict(uo.param_shapes(cfg)).items()}
    return cfg, sd


def _make_loop(space, lr):
    from improved_diffusion import script_util as su, dist_util
    from improved_diffusion.train_util import TrainLoop
    sh = _sh()
    if space == "wavelet":
        import test_wavelet_model_gpu as wm
        _, cfg, sd, _ = wm.case()
        diffusion = wm.make_diffusion()
    else:
        cfg, sd = _pixel_model()
        diffusion = su.create_gaussian_diffusion(steps=1000, rescale_timesteps=True, rescale_learned_sigmas=True)
    model = build_native(cfg, sd).train()
    dist_util.setup_dist()
    data = sh.ShapesBatches(sh.BouncingShapes(sh.ShapesParams(H=16, W=16, T=12, seed=SEED), "train"), batch_size=2)
    return TrainLoop(model=model, diffusion=diffusion, data=data, batch_size=2, microbatch=-1, lr=lr, ema_rate="0.9",
                     log_interval=1000, save_interval=10 ** 9, resume_checkpoint="", use_fp16=False, diffusion_space_kwargs={},
                     fp16_scale_growth=1e-3, schedule_sampler=None, weight_decay=0.01, lr_anneal_steps=0, sample_interval=None,
                     pad_with_random_frames=True, max_frames=4, enc_dec_chunk_size=20, args=argparse.Namespace(resume_id=""))


def _step(loop):
    from improved_diffusion.logger import logger
    loop.forward_backward()
    torch.cuda.synchronize()
    grad = loop.arena.g.clone()
    loop.optimize_normal()
    loop._flush_loss_log()
    loss = logger.name2val["loss"]
    logger.dumpkvs()
    loop.step += 1
    return loss, grad


@pytest.mark.parametrize("space", ["pixel", "wavelet"])
def test_train_loop_renders_what_the_host_path_loads(space, monkeypatch):
    """Two loops from the same seeds, one rendering its batches inside the step, one taking the host batches
    (LFVDM_DEVICE_BATCH_PREP=0): the same first-step loss and gradients, compared as
    test_training_step_with_device_batch_preparation_equals_host_path compares the existing device path (losses rtol 1e-4,
    gradients 2e-5 of their largest element).  The first steps are eager, so both draw the same noise; three more steps of the
    rendering loop then go through the captured graph and stay finite."""
    from improved_diffusion.logger import logger
    from improved_diffusion import _native as nat
    calls = {"render": 0, "prepare": 0}
    real_render, real_prepare = nat.shapes_render, nat.prepare_batch

    def counted_render(*a, **k):
        calls["render"] += 1
        return real_render(*a, **k)

    def counted_prepare(*a, **k):
        calls["prepare"] += 1
        return real_prepare(*a, **k)
    monkeypatch.setattr(nat, "shapes_render", counted_render)
    monkeypatch.setattr(nat, "prepare_batch", counted_prepare)
    first, later = {}, []
    for mode in ("1", "0"):
        monkeypatch.setenv("LFVDM_DEVICE_BATCH_PREP", mode)
        loop = _make_loop(space, lr=1e-4)
        assert (loop._device_source() is not None) == (mode == "1")
        torch.manual_seed(4); np.random.seed(4)
        logger.dumpkvs()
        first[mode] = _step(loop)
        if mode == "1":
            assert calls["render"] == 1 and calls["prepare"] == 0
            later = [_step(loop)[0] for _ in range(3)]
            assert loop._graph_state.get("graph") is not None, "the rendering micro-step should run as a captured graph by now"
            calls["render"] = 0
    assert calls["render"] == 0                                       # the host path never renders on the device
    print(f"[shapes TrainLoop {space}] first loss rendered {first['1'][0]} host {first['0'][0]}; then {later}")
    assert np.allclose(first["1"][0], first["0"][0], rtol=1e-4), (first["1"][0], first["0"][0])
    a, b = first["1"][1], first["0"][1]
    scale = float(a.abs().max())
    assert scale > 0 and float((a - b).abs().max()) < 2e-5 * scale, (float((a - b).abs().max()), scale)
    assert len(later) == 3 and np.isfinite(later).all(), later


def test_train_sample_score_end_to_end():
    """A few optimizer steps on rendered batches, then sample_video on two test-split videos with a short respaced chain and
    prediction_metrics against the dataset's own continuation.  No threshold on quality: a few steps train nothing."""
    from improved_diffusion import script_util as su
    from improved_diffusion.video_sampler import default_sampling_args, sample_video
    from improved_diffusion.video_metrics import prediction_metrics
    sh = _sh()
    loop = _make_loop("pixel", lr=1e-4)
    torch.manual_seed(5); np.random.seed(5)
    losses = [_step(loop)[0] for _ in range(4)]
    assert np.isfinite(losses).all()
    model = loop.model.eval()
    test = sh.BouncingShapes(sh.ShapesParams(H=16, W=16, T=12, seed=SEED), "test")
    test.set_test()
    truth = torch.stack([test[i][0] for i in range(2)])
    diff = su.create_gaussian_diffusion(steps=1000, timestep_respacing="4", rescale_timesteps=True, rescale_learned_sigmas=True)
    n_obs, K = 4, 2
    args = default_sampling_args(sampling_scheme="autoreg", n_obs=n_obs, max_frames=4, max_latent_frames=2, device="cuda")
    torch.manual_seed(6)
    samples = torch.stack([sample_video(args, model, diff, truth, verbose=False)[0] for _ in range(K)])
    assert samples.shape == (K,) + tuple(truth.shape) and torch.equal(samples[:, :, :n_obs], truth[None, :, :n_obs].expand(K, -1, -1, -1, -1, -1))
    m = prediction_metrics(samples.cuda().clamp(-1, 1), truth.cuda(), n_obs)
    assert m["n_samples"] == K and m["n_videos"] == 2 and m["best_index"].shape == (2,)
    for key in ("mean_psnr", "best_psnr", "mean_ssim", "best_ssim", "mean_mse", "best_mse"):
        assert m[key].shape == (12 - n_obs,) and bool(torch.isfinite(m[key]).all()), key
        assert np.isfinite(m[key + "_avg"])
    assert m["best_ssim_avg"] >= m["mean_ssim_avg"] - 1e-6
