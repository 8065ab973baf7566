"""Timestep loss weighting, host side (no GPU): the float64 weight tables of ``GaussianDiffusion.set_loss_weighting`` against a
restatement of the formulas written out here, the setter's and the parser's behaviour, the two new C entries declared, bound
and exported, and ``TrainLoop`` resolving ``loss_weighting`` as keyword > ``args`` > LFVDM_LOSS_WEIGHTING > "none".

The formulas (Min-SNR-gamma, Hang et al. 2023; P2, Choi et al. 2022), with snr = abar / (1 - abar):
  epsilon prediction   min_snr: min(snr, gamma) / snr        p2: (k + snr)^-gamma
  x0 prediction        snr times the epsilon weight."""
import argparse
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_oracle_golden import load_case
from test_host_cpu import native_model

NEW_EXPORTS = ("lfvdm_train_loss", "lfvdm_train_loss_bwd")


@pytest.fixture(autouse=True)
def _leave_the_logger_clean():
    """``TrainLoop`` logs running means into the process-wide logger (see tests/test_grad_clip_cpu.py)."""
    yield
    from improved_diffusion.logger import logger
    logger.dumpkvs()


def make_diffusion(schedule="linear", respacing="", **kw):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=1000, noise_schedule=schedule, timestep_respacing=respacing, rescale_timesteps=True,
                                        rescale_learned_sigmas=True, **kw)


def _abar(schedule, keep=None):
    """alphas_cumprod restated: the linear / cosine schedule over 1000 steps, optionally only the timesteps in ``keep``
    (respacing keeps the cumulative product of the steps it retains)."""
    if schedule == "linear":
        betas = np.linspace(1e-4, 0.02, 1000, dtype=np.float64)
    else:
        f = lambda u: math.cos((u + 0.008) / 1.008 * math.pi / 2) ** 2      # noqa: E731
        betas = np.array([min(1 - f((i + 1) / 1000) / f(i / 1000), 0.999) for i in range(1000)])
    abar = np.cumprod(1.0 - betas)
    return abar if keep is None else abar[np.asarray(sorted(keep))]


def _restated(abar, spec, x0):
    snr = abar / (1.0 - abar)
    if spec == "min_snr:5":
        eps = np.array([min(s, 5.0) / s if s > 0 else 1.0 for s in snr])
    else:
        assert spec == "p2:1:1"
        eps = 1.0 / (1.0 + snr)
    return snr * eps if x0 else eps


DIFFUSIONS = {"linear1000": ("linear", ""), "cosine1000": ("cosine", ""), "linear_respaced250": ("linear", "250")}


@pytest.mark.parametrize("spec", ["min_snr:5", "p2:1:1"])
@pytest.mark.parametrize("name", list(DIFFUSIONS))
def test_tables_match_the_restated_formulas(name, spec):
    from improved_diffusion.gaussian_diffusion import parse_loss_weighting
    schedule, respacing = DIFFUSIONS[name]
    tables = {}
    for x0 in (False, True):
        diff = make_diffusion(schedule, respacing, predict_xstart=x0)
        n = diff.num_timesteps
        assert n == (250 if respacing else 1000)
        abar = _abar(schedule, diff.use_timesteps if respacing else None)
        np.testing.assert_allclose(diff.alphas_cumprod, abar, rtol=1e-12)
        assert np.array_equal(diff.loss_weights(), np.ones(n))                        # the default
        diff.set_loss_weighting(**parse_loss_weighting(spec))
        w = diff.loss_weights()
        assert w.dtype == np.float64 and w.shape == (n,)
        assert np.isfinite(w).all() and (w >= 0).all()
        np.testing.assert_allclose(w, _restated(abar, spec, x0), rtol=1e-12, atol=0)
        dev = diff.loss_weight_table("cpu")
        assert dev.dtype == torch.float32 and tuple(dev.shape) == (n,) and dev.device.type == "cpu"
        assert np.array_equal(dev.numpy(), w.astype(np.float32))
        assert diff.loss_weight_table("cpu") is dev, "cached like tables(device)"
        w[0] = -1.0
        assert diff.loss_weights()[0] >= 0, "loss_weights() hands out a copy"
        tables[x0] = diff.loss_weights()
    snr = abar / (1.0 - abar)
    np.testing.assert_allclose(tables[True], snr * tables[False], rtol=1e-12, atol=0)


def test_linear_1000_anchors():
    diff = make_diffusion()
    assert abs(diff.alphas_cumprod[0] - 0.9999) < 1e-15
    snr0 = diff.alphas_cumprod[0] / (1.0 - diff.alphas_cumprod[0])
    assert abs(snr0 / 9999.0 - 1) < 1e-9
    diff.set_loss_weighting("min_snr", gamma=5)
    w = diff.loss_weights()
    assert abs(w[0] / (5.0 / 9999.0) - 1) < 1e-9
    assert w[-1] == 1.0                                   # snr < gamma: snr / snr
    assert (w <= 1.0).all() and (np.diff(w) >= 0).all()   # the cap only ever lowers a weight, and less so as snr falls
    x0 = make_diffusion(predict_xstart=True)
    x0.set_loss_weighting("min_snr")                      # gamma defaults to 5
    assert x0.loss_weights()[0] == 5.0 and x0.loss_weights().max() == 5.0


def test_setter_defaults_and_table_kind():
    diff = make_diffusion()
    assert diff.loss_weighting == "none"
    diff.set_loss_weighting("p2")
    assert diff.loss_weighting == "p2:1:1"
    diff.set_loss_weighting("p2", gamma=0)                # gamma = 0 is allowed for P2: every weight 1
    assert np.array_equal(diff.loss_weights(), np.ones(1000))
    tab = np.linspace(0.0, 2.0, 1000)
    for d in (diff, make_diffusion(predict_xstart=True)):
        d.set_loss_weighting("table", table=tab)
        assert d.loss_weighting == "table" and np.array_equal(d.loss_weights(), tab)      # the same array for both mean types
    before = diff.loss_weight_table("cpu")
    diff.set_loss_weighting()                             # back to the default, and the device copy is rebuilt
    assert diff.loss_weighting == "none" and np.array_equal(diff.loss_weights(), np.ones(1000))
    assert diff.loss_weight_table("cpu") is not before and float(diff.loss_weight_table("cpu").min()) == 1.0


def test_parser_round_trips():
    from improved_diffusion.gaussian_diffusion import parse_loss_weighting
    assert parse_loss_weighting("none") == {"kind": "none"}
    assert parse_loss_weighting("min_snr:5") == {"kind": "min_snr", "gamma": 5.0}
    assert parse_loss_weighting("min_snr") == {"kind": "min_snr"}
    assert parse_loss_weighting("p2:1:1") == {"kind": "p2", "k": 1.0, "gamma": 1.0}
    assert parse_loss_weighting(" p2:0.5 ") == {"kind": "p2", "k": 0.5}
    assert parse_loss_weighting({"kind": "table", "table": [1.0]}) == {"kind": "table", "table": [1.0]}
    diff = make_diffusion()
    for spec, canonical in (("none", "none"), ("min_snr:5", "min_snr:5"), ("min_snr", "min_snr:5"), ("p2:1:1", "p2:1:1"),
                            ("p2:0.5", "p2:0.5:1"), ("min_snr:0.1", "min_snr:0.1"), ("p2:2:0.25", "p2:2:0.25")):
        diff.set_loss_weighting(**parse_loss_weighting(spec))
        assert diff.loss_weighting == canonical
        w = diff.loss_weights()
        diff.set_loss_weighting(**parse_loss_weighting(diff.loss_weighting))      # what it reports parses back to itself
        assert diff.loss_weighting == canonical and np.array_equal(diff.loss_weights(), w)
    for bad in ("", "snr", "min-snr:5", "min_snr:five", "min_snr:5:1", "p2:1:1:1", "none:1", "table", 5, None):
        with pytest.raises(ValueError):
            parse_loss_weighting(bad)


def test_every_bad_setting_raises_value_error():
    diff = make_diffusion()
    diff.set_loss_weighting("min_snr", gamma=3)
    good = np.ones(1000)
    cases = [dict(kind="snr"), dict(kind=None),
             dict(kind="min_snr", gamma=0), dict(kind="min_snr", gamma=-1), dict(kind="min_snr", gamma=float("inf")),
             dict(kind="min_snr", gamma=float("nan")), dict(kind="min_snr", gamma="soon"),
             dict(kind="p2", k=0), dict(kind="p2", k=-1), dict(kind="p2", k=float("inf")), dict(kind="p2", k=float("nan")),
             dict(kind="p2", gamma=-0.5), dict(kind="p2", gamma=float("inf")), dict(kind="p2", gamma=float("nan")),
             dict(kind="table"), dict(kind="table", table=good[:999]), dict(kind="table", table=np.ones(1001)),
             dict(kind="table", table=np.ones((1000, 1))), dict(kind="table", table=np.where(np.arange(1000) == 7, -1e-9, good)),
             dict(kind="table", table=np.where(np.arange(1000) == 7, np.nan, good)),
             dict(kind="table", table=np.where(np.arange(1000) == 7, np.inf, good)),
             dict(kind="table", table=np.where(np.arange(1000) == 7, 1e39, good)),       # finite, but not in float32
             dict(kind="none", gamma=5), dict(kind="min_snr", k=1), dict(kind="min_snr", table=good), dict(kind="p2", table=good)]
    for kw in cases:
        with pytest.raises(ValueError):
            diff.set_loss_weighting(**kw)
        assert diff.loss_weighting == "min_snr:3", "a refused setting leaves the one in force untouched"
    respaced = make_diffusion(respacing="250")
    with pytest.raises(ValueError):
        respaced.set_loss_weighting("table", table=good)          # the table has the RESPACED length
    respaced.set_loss_weighting("table", table=good[:250])


def test_kl_loss_types_take_no_weighting():
    from improved_diffusion.gaussian_diffusion import LossType
    kl = make_diffusion(use_kl=True)
    assert kl.loss_type == LossType.RESCALED_KL and kl.loss_weighting == "none"
    kl.set_loss_weighting("none")
    for kw in (dict(kind="min_snr"), dict(kind="p2"), dict(kind="table", table=np.ones(1000))):
        with pytest.raises(ValueError):
            kl.set_loss_weighting(**kw)
    plain_kl = make_diffusion()
    plain_kl.loss_type = LossType.KL
    with pytest.raises(ValueError):
        plain_kl.set_loss_weighting("min_snr")


def test_public_signatures_are_untouched():
    """No constructor or factory argument was added for this: a method on the diffusion and a trailing keyword on TrainLoop."""
    import inspect
    from improved_diffusion import script_util as su
    from improved_diffusion.gaussian_diffusion import GaussianDiffusion
    from improved_diffusion.train_util import TrainLoop
    assert list(inspect.signature(GaussianDiffusion.__init__).parameters) == [
        "self", "betas", "model_mean_type", "model_var_type", "loss_type", "rescale_timesteps", "diffusion_space_kwargs"]
    assert len(su.model_and_diffusion_defaults()) == 22
    assert "loss_weighting" not in inspect.signature(su.create_gaussian_diffusion).parameters
    sig = inspect.signature(GaussianDiffusion.set_loss_weighting).parameters
    assert list(sig) == ["self", "kind", "gamma", "k", "table"] and sig["kind"].default == "none"
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY and sig[n].default is None for n in ("gamma", "k", "table"))
    loop = inspect.signature(TrainLoop.__init__).parameters
    assert list(loop)[-2:] == ["max_grad_norm", "loss_weighting"] and loop["loss_weighting"].default is None


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
    assert "LFVDM_LOSS_WEIGHTING" in hdr
    # host-side refusals of the entries need no device: nothing is launched for a bad shape or a missing pointer
    L = nat.lib()
    assert L.lfvdm_train_loss(None, None, None, None, None, None, 1000, None, None, None, 2, 4, 64, None) == 1
    assert L.lfvdm_train_loss_bwd(None, None, None, None, None, 1000, None, None, 2, 4, 64, None) == 1


def _data(B, T, C, H, seed):
    g = torch.Generator().manual_seed(seed)
    while True:
        yield (torch.randn(B, T, C, H, H, generator=g).clamp(-1, 1), {})


def make_host_loop(sd, cfg, args=None, diffusion=None, **kw):
    """A ``TrainLoop`` at the micro config whose model - hence every arena - lives in host memory (the helper of
    tests/test_grad_clip_cpu.py)."""
    from improved_diffusion.train_util import TrainLoop
    model = native_model(cfg)
    model.load_state_dict(sd)
    diffusion = diffusion if diffusion is not None else make_diffusion()
    return TrainLoop(model=model.train(), diffusion=diffusion, data=_data(2, 12, 4, 16, 0), batch_size=2, microbatch=-1, lr=1e-3,
                     ema_rate="0.9", log_interval=1000, save_interval=10 ** 9, resume_checkpoint="", use_fp16=False,
                     diffusion_space_kwargs={}, fp16_scale_growth=1e-3, schedule_sampler=None, weight_decay=0.01,
                     lr_anneal_steps=0, sample_interval=None, pad_with_random_frames=True, max_frames=4, enc_dec_chunk_size=20,
                     args=args if args is not None else argparse.Namespace(resume_id=""), **kw)


def test_trainloop_precedence_and_validation(monkeypatch):
    cfg, sd, _ = load_case("micro")
    ns = argparse.Namespace
    monkeypatch.delenv("LFVDM_LOSS_WEIGHTING", raising=False)
    loop = make_host_loop(sd, cfg)
    assert loop.loss_weighting == "none" and loop.diffusion.loss_weighting == "none"           # nothing set: the default
    monkeypatch.setenv("LFVDM_LOSS_WEIGHTING", "p2:1:1")
    assert make_host_loop(sd, cfg).loss_weighting == "p2:1:1"                                   # the environment, last resort
    assert make_host_loop(sd, cfg, args=ns(resume_id="", loss_weighting=None)).loss_weighting == "p2:1:1"
    assert make_host_loop(sd, cfg, args=ns(resume_id="", loss_weighting="min_snr:3")).loss_weighting == "min_snr:3"    # args beat it
    loop = make_host_loop(sd, cfg, args=ns(resume_id="", loss_weighting="min_snr:3"), loss_weighting="min_snr:5")
    assert loop.loss_weighting == "min_snr:5" and loop.diffusion.loss_weighting == "min_snr:5"  # the keyword beats both
    assert abs(loop.diffusion.loss_weights()[0] / (5.0 / 9999.0) - 1) < 1e-9
    assert make_host_loop(sd, cfg, args=ns(resume_id="", loss_weighting="min_snr:3"), loss_weighting="none").loss_weighting == "none"
    tab = np.full(1000, 0.25)
    loop = make_host_loop(sd, cfg, loss_weighting={"kind": "table", "table": tab})              # a table: the setter's arguments
    assert loop.loss_weighting == "table" and np.array_equal(loop.diffusion.loss_weights(), tab)
    for bad in ("min_snr:0", "min_snr:-1", "p2:0", "p2:1:-1", "snr", "min_snr:soon", "table", 7):
        with pytest.raises(ValueError):
            make_host_loop(sd, cfg, loss_weighting=bad)
    for bad in ("min_snr:inf", "p2:nan", "warm"):
        with pytest.raises(ValueError):
            make_host_loop(sd, cfg, args=ns(resume_id="", loss_weighting=bad))
        monkeypatch.setenv("LFVDM_LOSS_WEIGHTING", bad)
        with pytest.raises(ValueError):
            make_host_loop(sd, cfg)
    monkeypatch.setenv("LFVDM_LOSS_WEIGHTING", "min_snr:5")
    with pytest.raises(ValueError):
        make_host_loop(sd, cfg, diffusion=make_diffusion(use_kl=True))                          # the KL loss takes no weighting
    assert make_host_loop(sd, cfg, diffusion=make_diffusion(use_kl=True), loss_weighting="none").loss_weighting == "none"


def test_log_loss_dict_logs_mse_and_loss_with_separate_quartiles():
    """With a weighting on, 'loss' and 'mse' are distinct per-sample tensors: the log carries the mean and the timestep
    quartiles of each."""
    from improved_diffusion.logger import logger
    from improved_diffusion.train_util import log_loss_dict
    logger.dumpkvs()
    diff = make_diffusion()
    ts = np.array([10.0, 990.0], dtype=np.float32)
    log_loss_dict(diff, ts, {"mse": np.array([0.5, 0.25], dtype=np.float32), "eval-mse": np.array([0.5, 0.25], dtype=np.float32),
                             "loss": np.array([0.125, 0.25], dtype=np.float32)})
    got = logger.dumpkvs()
    for key, q0, q3 in (("mse", 0.5, 0.25), ("loss", 0.125, 0.25)):
        assert got[key] == pytest.approx((q0 + q3) / 2) and got[f"{key}_q0"] == pytest.approx(q0) and got[f"{key}_q3"] == pytest.approx(q3)
