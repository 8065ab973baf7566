"""Global-norm gradient clipping, host side (no GPU): the C ABI of csrc/grad_clip.hip is declared, bound and exported, the
optimizer's argument struct and the ABI version are what they were, ``TrainLoop`` resolves ``max_grad_norm`` as keyword >
``args`` > LFVDM_MAX_GRAD_NORM > off, and ``TrainLoop.optimize_normal`` on arenas in host memory follows
``clip_grad_norm_`` + ``torch.optim.AdamW`` + EMA.

The U-Net executes on the device only (tests/test_host_cpu.py::test_cpu_forward_fails_loudly), so the two host-memory steps
take their gradients from the CPU oracle (oracle/unet_oracle.py, the arithmetic ``__graft_entry__.smoke`` checks the native
backward pass against) evaluated on the loop's own parameters: same model (the micro config), same loss, and everything
after ``loss.backward()`` is ``TrainLoop``'s."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import recipe, unet_oracle as uo, diffusion_oracle as do
from conftest import ROOT
from test_oracle_golden import load_case
from test_host_cpu import native_model

NEW_EXPORTS = ("lfvdm_grad_norm_nparts", "lfvdm_grad_norm_partials", "lfvdm_grad_norm_finalize", "lfvdm_adamw_ema_clip")


@pytest.fixture(autouse=True)
def _leave_the_logger_clean():
    """``TrainLoop`` logs running means into the process-wide logger; a loop that is never dumped would leave its losses in
    the means the next test's loop reports (tests/test_train_gpu.py compares them)."""
    yield
    from improved_diffusion.logger import logger
    logger.dumpkvs()


# lfvdm_adamw_args as the fused optimizer has always taken it (include/lfvdm_hip.h): the clip entry adds no field
ADAMW_ARGS_FIELDS = ["float* p", "const float* g", "float* m", "float* v", "float* ema[4]", "float ema_rate[4]", "int32_t n_ema",
                     "int64_t n", "float lr, beta1, beta2, eps, weight_decay", "float bias_corr1, bias_corr2_sqrt",
                     "float grad_scale", "float* grad_sqsum", "const int32_t* skip_flag", "const int32_t* skip_flag2"]


def test_exports_declared_bound_and_abi_unchanged():
    from improved_diffusion import _native as nat
    hdr = open(os.path.join(ROOT, "include", "lfvdm_hip.h")).read()
    declared = set(re.findall(r"\b(lfvdm_[a-z0-9_]+)\s*\(", hdr))
    assert os.path.exists(nat.LIB_PATH), "run `python __graft_entry__.py` (build) first"
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW_EXPORTS:
        assert name in declared, f"{name} is not declared in include/lfvdm_hip.h"
        assert name in nat.EXPORTS, f"{name} is not bound in _native"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.lfvdm_abi_version() == 9
    # the struct: same fields in the same order in the header, same size and offsets in the binding
    body = re.search(r"typedef struct lfvdm_adamw_args \{(.*?)\} lfvdm_adamw_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ADAMW_ARGS_FIELDS
    assert ctypes.sizeof(nat.AdamWArgs) == 152
    assert [(n, getattr(nat.AdamWArgs, n).offset) for n in ("ema", "n_ema", "n", "grad_scale", "grad_sqsum", "skip_flag2")] == \
        [("ema", 32), ("n_ema", 80), ("n", 88), ("grad_scale", 124), ("grad_sqsum", 128), ("skip_flag2", 144)]
    # the grid of the norm launch is a function of n alone, within the documented bound (host-only call)
    lib.lfvdm_grad_norm_nparts.argtypes, lib.lfvdm_grad_norm_nparts.restype = [ctypes.c_int64], ctypes.c_int
    cap = int(re.search(r"#define LFVDM_GRAD_NORM_MAX_PARTS (\d+)", hdr).group(1))
    parts = [lib.lfvdm_grad_norm_nparts(n) for n in (1, 3, 1023, 262147, 10 ** 8, 2 ** 33)]
    assert parts[0] == parts[1] == parts[2] == 1 and 1 < parts[3] <= parts[4] <= parts[5] == cap
    assert lib.lfvdm_grad_norm_nparts(0) == 0


def _data(B, T, C, H, seed):
    g = torch.Generator().manual_seed(seed)
    while True:
        yield (torch.randn(B, T, C, H, H, generator=g).clamp(-1, 1), {})


def make_host_loop(sd, cfg, args=None, lr=1e-3, weight_decay=0.01, ema_rate="0.9", **kw):
    """A ``TrainLoop`` at the micro config whose model - hence every arena - lives in host memory."""
    from improved_diffusion import script_util as su
    from improved_diffusion.train_util import TrainLoop
    model = native_model(cfg)
    model.load_state_dict(sd)
    diffusion = su.create_gaussian_diffusion(steps=1000, rescale_timesteps=True, rescale_learned_sigmas=True)
    return TrainLoop(model=model.train(), diffusion=diffusion, data=_data(2, 12, 4, 16, 0), batch_size=2, microbatch=-1, lr=lr,
                     ema_rate=ema_rate, log_interval=1000, save_interval=10 ** 9, resume_checkpoint="", use_fp16=False,
                     diffusion_space_kwargs={}, fp16_scale_growth=1e-3, schedule_sampler=None, weight_decay=weight_decay,
                     lr_anneal_steps=0, sample_interval=None, pad_with_random_frames=True, max_frames=4, enc_dec_chunk_size=20,
                     args=args if args is not None else argparse.Namespace(resume_id=""), **kw)


def test_max_grad_norm_precedence_and_validation(monkeypatch):
    cfg, sd, _ = load_case("micro")
    ns = argparse.Namespace
    monkeypatch.delenv("LFVDM_MAX_GRAD_NORM", raising=False)
    assert make_host_loop(sd, cfg).max_grad_norm == 0.0                                   # nothing set: off
    monkeypatch.setenv("LFVDM_MAX_GRAD_NORM", "4")
    assert make_host_loop(sd, cfg).max_grad_norm == 4.0                                   # the environment, last resort
    assert make_host_loop(sd, cfg, args=ns(resume_id="", max_grad_norm=None)).max_grad_norm == 4.0
    assert make_host_loop(sd, cfg, args=ns(resume_id="", max_grad_norm=3.0)).max_grad_norm == 3.0       # args beat it
    assert make_host_loop(sd, cfg, args=ns(resume_id="", max_grad_norm=3.0), max_grad_norm=2.0).max_grad_norm == 2.0
    assert make_host_loop(sd, cfg, args=ns(resume_id="", max_grad_norm=3.0), max_grad_norm=0).max_grad_norm == 0.0   # keyword 0 = off
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            make_host_loop(sd, cfg, max_grad_norm=bad)
        with pytest.raises(ValueError):
            make_host_loop(sd, cfg, args=ns(resume_id="", max_grad_norm=bad))
    for bad in ("-0.5", "inf", "soon"):
        monkeypatch.setenv("LFVDM_MAX_GRAD_NORM", bad)
        with pytest.raises(ValueError):
            make_host_loop(sd, cfg)


def _oracle_backward(params, cfg, inp, tab, t, noise):
    """reference train_util.py:320-328 with uniform weights: training_losses -> loss.mean().backward(), through the oracle."""
    lat = 1.0 - inp["obs_mask"]

    def eps(x_t, ts):
        return uo.unet_forward(params, cfg, x_t, inp["x0"], ts, inp["frame_indices"], inp["obs_mask"], inp["latent_mask"])[0]
    do.training_losses(tab, eps, inp["x0"], t, noise, lat, lat)["loss"].mean().backward()


@pytest.mark.parametrize("max_grad_norm", [1e-3, 0.0], ids=["clip_1e-3", "off"])
def test_host_memory_steps_match_clip_grad_norm_adamw_ema(max_grad_norm, monkeypatch):
    """Two optimizer steps, ``TrainLoop.optimize_normal`` against the hand-written loop backward -> clip_grad_norm_ ->
    torch.optim.AdamW -> EMA on the same gradients; atol 1e-6 / rtol 1e-5, the tolerance of
    tests/test_train_gpu.py::test_fused_adamw_ema_matches_torch."""
    monkeypatch.delenv("LFVDM_MAX_GRAD_NORM", raising=False)
    cfg, sd, inp = load_case("micro")
    loop = make_host_loop(sd, cfg, max_grad_norm=max_grad_norm)
    assert not loop.arena.p.is_cuda
    names = [k for k, _ in loop.model.named_parameters()]
    ref = {k: torch.nn.Parameter(sd[k].clone()) for k in names}
    ref_ema = {k: sd[k].clone() for k in names}
    opt = torch.optim.AdamW(list(ref.values()), lr=1e-3, weight_decay=0.01)
    tab = do.Tables(do.linear_betas(1000))
    for step, t in enumerate((torch.tensor([700, 120]), torch.tensor([31, 905]))):
        noise = torch.from_numpy(recipe.gaussianish(f"clip/noise{step}", inp["x"].numel()).reshape(inp["x"].shape).astype(np.float32))
        loop.arena.zero_grad()
        _oracle_backward(dict(loop.model.named_parameters()), cfg, inp, tab, t, noise)
        assert float(loop.arena.g.abs().max()) > 0, "the gradients must have landed in the arena"
        norm_before = float(loop.arena.g.double().norm())
        loop.optimize_normal()
        loop.step += 1
        opt.zero_grad(set_to_none=True)
        _oracle_backward(ref, cfg, inp, tab, t, noise)
        if max_grad_norm > 0:
            torch.nn.utils.clip_grad_norm_(list(ref.values()), max_grad_norm, error_if_nonfinite=False)
        opt.step()
        for k in names:
            ref_ema[k].mul_(0.9).add_(ref[k].detach(), alpha=0.1)
        if max_grad_norm > 0:
            assert norm_before > max_grad_norm, "the case is meant to clip"
            assert abs(float(loop.clip_stat[0]) ** 0.5 - norm_before) <= 1e-5 * norm_before
            assert 0.0 < float(loop.clip_stat[1]) < 1.0 and loop.clip_stat.view(torch.int32)[2:].tolist() == [0, 0]
        for (k, p), e in zip(loop.model.named_parameters(), loop.ema_params[0]):
            assert torch.allclose(p.detach(), ref[k].detach(), atol=1e-6, rtol=1e-5), (step, k)
            assert torch.allclose(e, ref_ema[k], atol=1e-6, rtol=1e-5), (step, k)
    moved = max(float((p.detach() - sd[k]).abs().max()) for k, p in loop.model.named_parameters())
    assert moved > 1e-4, "the optimizer must have moved the parameters"


def test_host_memory_step_skips_a_nonfinite_gradient(monkeypatch):
    """Same semantics as the device path: an inf or NaN gradient norm leaves parameters, moments and EMA untouched and is
    counted; the next clean step updates."""
    monkeypatch.delenv("LFVDM_MAX_GRAD_NORM", raising=False)
    cfg, sd, _ = load_case("micro")
    loop = make_host_loop(sd, cfg, max_grad_norm=1.0)
    g = torch.Generator().manual_seed(5)
    before = [t.clone() for t in (loop.arena.p, loop.exp_avg, loop.exp_avg_sq, loop.ema_flat[0])]
    for k, poison in enumerate((float("inf"), float("nan"))):
        loop.arena.g.copy_(torch.randn(loop.arena.numel, generator=g) * 1e-3)
        loop.arena.g[-1] = poison
        loop.optimize_normal()
        assert loop.clip_stat.view(torch.int32)[2:].tolist() == [1, k + 1]
        for a, b in zip(before, (loop.arena.p, loop.exp_avg, loop.exp_avg_sq, loop.ema_flat[0])):
            assert torch.equal(a, b)
    loop.arena.g.copy_(torch.randn(loop.arena.numel, generator=g) * 1e-3)
    loop.optimize_normal()
    assert loop.clip_stat.view(torch.int32)[2:].tolist() == [0, 2]
    assert float((loop.arena.p - before[0]).abs().max()) > 1e-4 and loop.opt_step == 3      # Adam's counter ran on
