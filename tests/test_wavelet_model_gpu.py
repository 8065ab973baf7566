"""A level-1 wavelet-space model on the MI355X: 12 input and 12 output channels (RGB frames of 16 x 16 as 8 x 8 coefficient
maps), model_channels 64, one ResBlock per level, T = 4, B = 2 - through the native forward, the training forward + backward,
the ancestral and DDIM sampling loops with the decode at their end, and two TrainLoop steps with the batch prepared on the
device (lfvdm_prepare_batch_wavelet) and on the host.

Tolerances are those of the existing tests of the same quantities, not measured on this model:
  forward    |d| <= 1e-4 + 1e-3 |ref| against the CPU oracle (test_forward_gpu.py, the contract of SURVEY 8c);
  gradients  per tensor max|d| / (max|ref| + 1e-3 gmax) < 2e-3 against autograd on the oracle
             (test_backward_gpu.py::test_parameter_gradients_match_oracle), loss 1e-4 relative (the smoke run's)."""
import argparse
import functools

import numpy as np
import pytest
import torch

from oracle import recipe, unet_oracle as uo, diffusion_oracle as do
from test_forward_gpu import build_native

pytestmark = pytest.mark.gpu

B, T, C_PIX, H_PIX = 2, 4, 3, 16


@functools.lru_cache(maxsize=None)
def case():
    from improved_diffusion.wavelet import space_args
    sp = space_args(H_PIX, channels=C_PIX, levels=1)
    assert sp["in_channels"] == 12 and sp["image_size"] == 8
    cfg = uo.make_cfg(in_channels=sp["in_channels"], model_channels=64, num_res_blocks=1, channel_mult=(1, 2),
                      attention_resolutions=(1, 2), num_heads=4)
    sd = {k: torch.from_numpy(v) for k, v in recipe.fill_state_dict(uo.param_shapes(cfg)).items()}
    inp = {k: torch.from_numpy(v) for k, v in
           recipe.make_inputs("wavelet_l1", B, T, cfg["in_channels"], sp["image_size"], sp["image_size"], n_pad=1).items()}
    return sp, cfg, sd, inp


def make_diffusion(resp=""):
    from improved_diffusion import script_util as su
    sp = case()[0]
    return su.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, rescale_timesteps=True, rescale_learned_sigmas=True,
                                        diffusion_space_kwargs=sp["diffusion_space_kwargs"])


def test_forward_matches_the_oracle():
    _, cfg, sd, inp = case()
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    with torch.no_grad():
        out, _ = model(d["x"], x0=d["x0"], timesteps=d["t"].float(), frame_indices=d["frame_indices"], obs_mask=d["obs_mask"],
                       latent_mask=d["latent_mask"])
        ref, _ = uo.unet_forward(sd, cfg, inp["x"], inp["x0"], inp["t"].float(), inp["frame_indices"], inp["obs_mask"],
                                 inp["latent_mask"])
    assert out.shape == (B, T, 12, 8, 8)
    err = float((out.cpu() - ref).abs().max())
    print(f"[wavelet l1 forward] max|hip - oracle| = {err:.3e} (max|ref| {float(ref.abs().max()):.3f})")
    assert torch.allclose(out.cpu(), ref, atol=1e-4, rtol=1e-3), err


def test_training_losses_and_gradients_match_the_oracle():
    _, cfg, sd, inp = case()
    model = build_native(cfg, sd).train()
    d = {k: v.cuda() for k, v in inp.items()}
    diff = make_diffusion()
    tab = do.Tables(do.linear_betas(1000))
    tt = torch.tensor([700, 120])
    noise = torch.from_numpy(recipe.gaussianish("wavelet_l1/noise", inp["x"].numel()).reshape(inp["x"].shape).astype(np.float32))
    lat = 1.0 - inp["obs_mask"]
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    terms = diff.training_losses(model, d["x0"], tt.cuda(), model_kwargs=mk, noise=noise.cuda(), latent_mask=lat.cuda(),
                                 eval_mask=lat.cuda())
    terms["loss"].mean().backward()
    torch.cuda.synchronize()
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}

    def oracle_eps(x_t, ts):
        return uo.unet_forward(sdo, cfg, x_t, inp["x0"], ts, inp["frame_indices"], inp["obs_mask"], inp["latent_mask"])[0]
    oterms = do.training_losses(tab, oracle_eps, inp["x0"], tt, noise, lat, lat)
    oterms["loss"].mean().backward()
    lerr = float((terms["loss"].detach().cpu() - oterms["loss"].detach()).abs().max())
    assert lerr < 1e-4 * float(oterms["loss"].detach().abs().max()) + 1e-6, lerr
    gmax = max(float(v.grad.abs().max()) for v in sdo.values() if v.grad is not None)
    worst, worst_key = 0.0, None
    for k, p in model.named_parameters():
        ref = sdo[k].grad
        if ref is None:
            continue
        assert p.grad is not None, k
        err = float((p.grad.cpu() - ref).abs().max()) / (float(ref.abs().max()) + 1e-3 * gmax)
        if err > worst:
            worst, worst_key = err, k
    print(f"[wavelet l1 training] loss max|d| = {lerr:.2e}; worst relative gradient error {worst:.2e} ({worst_key})")
    assert worst < 2e-3, (worst, worst_key)


@pytest.mark.parametrize("sampler", ["ancestral", "ddim"])
def test_sampling_loops_decode_to_pixels(sampler):
    from improved_diffusion.wavelet import wavelet_decode
    _, cfg, sd, inp = case()
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    shape = tuple(inp["x"].shape)

    def run(decoded):
        diff = make_diffusion("5")
        torch.manual_seed(17)
        if sampler == "ancestral":
            return diff.p_sample_loop(model, shape, noise=d["x"].clone(), clip_denoised=True, model_kwargs=mk,
                                      return_decoded=decoded)[0]
        return diff.ddim_sample_loop(model, shape, noise=d["x"].clone(), clip_denoised=True, model_kwargs=mk, eta=0.5,
                                     return_decoded=decoded)
    pix, coef = run(True), run(False)
    assert coef.shape == shape and pix.shape == (B, T, C_PIX, H_PIX, H_PIX)
    assert bool(torch.isfinite(pix).all()) and bool(torch.isfinite(coef).all())
    assert torch.equal(pix, wavelet_decode(coef, 1, "range"))


def test_two_level_engine_is_refused_with_the_limit_and_the_way_out():
    """48 input channels (L = 2 on RGB) exceed the LDS of the native input convolution: the engine says so, and names
    wavelet_levels=1, before anything runs."""
    cfg = uo.make_cfg(in_channels=48, model_channels=64, num_res_blocks=1, channel_mult=(1, 2), attention_resolutions=(1, 2),
                      num_heads=4)
    sd = {k: torch.from_numpy(v) for k, v in recipe.fill_state_dict(uo.param_shapes(cfg)).items()}
    model = build_native(cfg, sd)
    inp = {k: torch.from_numpy(v).cuda() for k, v in recipe.make_inputs("wavelet_l2", 1, 2, 48, 4, 4, n_pad=0).items()}
    with torch.no_grad(), pytest.raises(NotImplementedError, match=r"64 KiB.*wavelet_levels=1"):
        model(inp["x"], x0=inp["x0"], timesteps=inp["t"].float(), frame_indices=inp["frame_indices"], obs_mask=inp["obs_mask"],
              latent_mask=inp["latent_mask"])


def _pixel_data(seed=0):
    g = torch.Generator().manual_seed(seed)
    while True:
        yield (torch.rand(B, 12, C_PIX, H_PIX, H_PIX, generator=g) * 2 - 1, {})


def test_train_loop_device_and_host_batch_preparation_give_the_same_losses(monkeypatch):
    """Two TrainLoop steps in wavelet space with the batch prepared on the device (lfvdm_prepare_batch_wavelet inside the
    step) and on the host (diffusion.encode of the gathered frames): the losses are equal bit for bit.  Eager micro-steps
    (LFVDM_TRAIN_GRAPH=0: the same noise draws) and LFVDM_DETERMINISTIC=1 (ordered gradient sums, so that the parameters
    after the first step are the same bits in both runs)."""
    from improved_diffusion import dist_util
    from improved_diffusion.logger import logger
    from improved_diffusion.train_util import TrainLoop
    monkeypatch.setenv("LFVDM_TRAIN_GRAPH", "0")
    monkeypatch.setenv("LFVDM_DETERMINISTIC", "1")
    _, cfg, sd, _ = case()
    calls = {"device": 0}
    from improved_diffusion import _native as nat
    real = nat.prepare_batch_wavelet

    def counted(*a, **k):
        calls["device"] += 1
        return real(*a, **k)
    monkeypatch.setattr(nat, "prepare_batch_wavelet", counted)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("LFVDM_DEVICE_BATCH_PREP", mode)
        model = build_native(cfg, sd).train()
        dist_util.setup_dist()
        loop = TrainLoop(model=model, diffusion=make_diffusion(), data=_pixel_data(), batch_size=B, microbatch=-1, lr=1e-3,
                         ema_rate="0.9", log_interval=1000, save_interval=10 ** 9, resume_checkpoint="", use_fp16=False,
                         diffusion_space_kwargs={}, fp16_scale_growth=1e-3, schedule_sampler=None, weight_decay=0.01,
                         lr_anneal_steps=0, sample_interval=None, pad_with_random_frames=True, max_frames=T,
                         enc_dec_chunk_size=20, args=argparse.Namespace(resume_id=""))
        torch.manual_seed(4); np.random.seed(4)
        logger.dumpkvs()
        losses = []
        for _ in range(2):
            loop.forward_backward()
            loop.optimize_normal()
            loop._flush_loss_log()
            losses.append(logger.name2val["loss"])
            logger.dumpkvs()
            loop.step += 1
        outs[mode] = losses
        assert calls["device"] == 2, calls      # one launch per step of the first pass, none in the host-prepared pass
    print(f"[wavelet l1 TrainLoop] losses device prep {outs['1']}  host prep {outs['0']}")
    assert all(np.isfinite(v) for v in outs["1"])
    assert outs["1"] == outs["0"], (outs["1"], outs["0"])
