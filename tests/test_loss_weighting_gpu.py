"""Timestep loss weighting on the MI355X (csrc/train_loss.hip): the fused loss launch and its backward against float64 torch
autograd and - bitwise - against ``lfvdm_masked_mse``; ``training_losses`` with min-SNR weighting for both mean types against
the oracle's fp32 autograd; the captured micro-step gathering the weight of THIS step's ``t``; exact power-of-two scaling of the
gradient arena; bitwise repeatability in deterministic mode.  GPU only."""
import argparse

import numpy as np
import pytest
import torch

from oracle import recipe, unet_oracle as uo, diffusion_oracle as do
from test_oracle_golden import load_case
from test_forward_gpu import build_native
from test_dist_gpu import _data

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _leave_the_logger_clean():
    """``TrainLoop`` logs running means into the process-wide logger (see tests/test_grad_clip_gpu.py)."""
    yield
    from improved_diffusion.logger import logger
    logger.dumpkvs()


def close(got, ref, atol, rtol):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    bad = (got - ref).abs() > atol + rtol * ref.abs()
    assert not bool(bad.any()), (float((got - ref).abs().max()), float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------ the op
N_T, ZERO_AT = 50, 17      # table length; the one entry that is exactly 0

# frame_inner 75: scalar path, B = 3 | float4 path, 96 quads < 1024 threads | float4 path, 1280 quads: a second sweep
SHAPES = [(3, 2, 3, 5, 5), (2, 3, 4, 4, 4), (1, 5, 4, 16, 16)]
# timestep vectors per batch size: 0, n_t - 1, the zero entry, a repeated value
T_CASES = {3: [[0, N_T - 1, ZERO_AT], [ZERO_AT, ZERO_AT, 0]], 2: [[0, N_T - 1], [ZERO_AT, ZERO_AT], [31, 31]],
           1: [[0], [N_T - 1], [ZERO_AT]]}


def _weights():
    w = torch.rand(N_T, generator=torch.Generator().manual_seed(99), dtype=torch.float64) * 3 + 0.05
    w[ZERO_AT] = 0.0
    return w


def _masks(case, B, T, gen):
    """(mask, eval_mask) as (B, T, 1, 1, 1) tensors or None"""
    draw = lambda: (torch.rand(B, T, 1, 1, 1, generator=gen) < 0.6).float()      # noqa: E731
    if case == "no_masks":
        return None, None
    if case == "latent_mask_only":
        m = draw()
        m[0, 0] = 1.0
        return m, None
    m, e = draw(), draw()
    m[0, 0], e[0, -1] = 1.0, 1.0
    e[0, 0] = 1.0 - m[0, 0]          # the two masks differ
    if case == "all_zero_row":
        m[B - 1] = 0.0
    return m, e


@pytest.mark.parametrize("case", ["no_masks", "latent_mask_only", "two_masks", "all_zero_row"])
@pytest.mark.parametrize("shape", SHAPES, ids=["scalar_75", "quads_96", "quads_1280"])
def test_train_loss_forward_and_backward(shape, case):
    """lfvdm_train_loss / lfvdm_train_loss_bwd and the autograd bridge.  Values within 1e-6 + 1e-5 |ref| and gradients within
    1e-7 + 1e-5 |ref| of float64 autograd (the bounds of test_ops_gpu.py::test_masked_mse_forward_and_backward; the table's
    rounding to float32 adds at most 2^-24 = 6e-8 relative); mse / eval_mse bitwise lfvdm_masked_mse; loss bitwise the float32
    product mse * wtab[t]; NaN-prefilled outputs fully written; a second run bitwise the first; an all-zero mask row and the
    zero table entry give exact zeros."""
    from improved_diffusion import _native as nat
    from improved_diffusion._autograd import train_loss
    B, T = shape[:2]
    gen = torch.Generator().manual_seed(1000 * shape[0] + shape[-1])
    tgt, prd = torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen)
    mask, emask = _masks(case, B, T, gen)
    w64 = _weights()
    wtab = w64.float().cuda()
    seed = torch.tensor([0.7, -1.3, 2.1])[:B]
    dt, dp = tgt.cuda(), prd.cuda()
    m2 = None if mask is None else mask.reshape(B, T).cuda()
    e2 = None if emask is None else emask.reshape(B, T).cuda()
    for tv in T_CASES[B]:
        t = torch.tensor(tv)
        # float64 reference
        pr = prd.double().requires_grad_(True)
        d2 = (tgt.double() - pr) ** 2
        ref_mse = (d2 if mask is None else d2 * mask.double()).flatten(1).mean(1)
        ref_eval = (d2 if emask is None else d2 * emask.double()).flatten(1).mean(1)
        ref_loss = ref_mse * w64[t]
        (ref_loss * seed.double()).sum().backward()
        # the raw entries on NaN-prefilled outputs
        outs = [torch.full((B,), float("nan"), device="cuda") for _ in range(3)]
        nat.train_loss(dt, dp, m2, e2, t.cuda(), wtab, *outs)
        grad = torch.full(shape, float("nan"), device="cuda")
        nat.train_loss_bwd(dt, dp, m2, t.cuda(), wtab, seed.cuda(), grad)
        mse, eval_mse, loss = outs
        assert all(bool(torch.isfinite(o).all()) for o in outs) and bool(torch.isfinite(grad).all()), "an output element was not written"
        for name, got, ref in (("mse", mse, ref_mse), ("eval_mse", eval_mse, ref_eval), ("loss", loss, ref_loss)):
            err = float((got.cpu().double() - ref.detach()).abs().max())
            print(f"[{shape} {case} t={tv}] {name} {got.cpu().numpy()} max|d| {err:.2e}")
            close(got, ref, 1e-6, 1e-5)
        close(grad, pr.grad, 1e-7, 1e-5)
        # bitwise: the two means are lfvdm_masked_mse's, the loss is one float32 product
        for got, mk in ((mse, m2), (eval_mse, e2)):
            plain = torch.full((B,), float("nan"), device="cuda")
            nat.masked_mse(dt, dp, mk, plain, B, T, tgt[0, 0].numel())
            assert torch.equal(got, plain), (got, plain)
        assert torch.equal(loss, mse * wtab[t.cuda()])
        # exact zeros: the zero table entry, and a row whose mask is all zero
        for b in range(B):
            if tv[b] == ZERO_AT:
                assert float(loss[b]) == 0.0 and float(grad[b].abs().max()) == 0.0
            if case == "all_zero_row" and b == B - 1:
                assert float(mse[b]) == 0.0 and float(loss[b]) == 0.0 and float(grad[b].abs().max()) == 0.0
        # the autograd bridge: the same launches, only 'loss' differentiable; a second run is bitwise the first
        pg = dp.clone().requires_grad_(True)
        a_mse, a_eval, a_loss = train_loss(dt, pg, mask if mask is None else mask.cuda(), emask if emask is None else emask.cuda(),
                                           t.cuda(), wtab)
        assert a_loss.requires_grad and not a_mse.requires_grad and not a_eval.requires_grad
        (a_loss * seed.cuda()).sum().backward()
        assert torch.equal(a_mse, mse) and torch.equal(a_eval, eval_mse) and torch.equal(a_loss, loss)
        assert torch.equal(pg.grad, grad)


def test_table_index_is_clamped():
    """A timestep outside the table reads its nearest end, never memory outside it (the kernels clamp the index)."""
    from improved_diffusion import _native as nat
    shape = (3, 2, 4, 4, 4)
    gen = torch.Generator().manual_seed(5)
    tgt, prd = torch.randn(*shape, generator=gen).cuda(), torch.randn(*shape, generator=gen).cuda()
    wtab = _weights().float().cuda()
    res = {}
    for name, tv in (("outside", [-3, N_T, 10 ** 12]), ("ends", [0, N_T - 1, N_T - 1])):
        outs = [torch.empty(3, device="cuda") for _ in range(3)]
        grad = torch.empty(shape, device="cuda")
        nat.train_loss(tgt, prd, None, None, torch.tensor(tv).cuda(), wtab, *outs)
        nat.train_loss_bwd(tgt, prd, None, torch.tensor(tv).cuda(), wtab, torch.ones(3, device="cuda"), grad)
        res[name] = outs + [grad]
    for a, b in zip(res["outside"], res["ends"]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ training_losses
def make_diffusion(**kw):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=1000, rescale_timesteps=True, rescale_learned_sigmas=True, **kw)


def _oracle_weighted_losses(sdo, cfg, inp, tab, t, noise, lat, ev, w64, x0_mode):
    """The oracle's ``training_losses`` - fp32 tensor math on the CPU, as tests/test_backward_gpu.py and ``smoke()`` use it -
    with its per-sample loss multiplied by the float64 weight before autograd.  Epsilon prediction is
    ``diffusion_oracle.training_losses`` itself; for x0 prediction the same steps (q_sample, the timestep map, the U-Net oracle,
    masked_mean_flat) regress on x_start, as reference gaussian_diffusion.py:779-785 does."""
    def net(x_t, ts):
        return uo.unet_forward(sdo, cfg, x_t, inp["x0"], ts, inp["frame_indices"], inp["obs_mask"], inp["latent_mask"])[0]
    if not x0_mode:
        terms = do.training_losses(tab, net, inp["x0"], t, noise, lat, ev)
    else:
        sq = (inp["x0"] - net(do.q_sample(tab, inp["x0"], t, noise), do.model_timesteps(tab, t))) ** 2
        terms = {"mse": do.masked_mean_flat(sq, lat), "eval-mse": do.masked_mean_flat(sq, ev)}
    terms["loss"] = terms["mse"].double() * torch.from_numpy(w64)[t]
    return terms


@pytest.mark.parametrize("x0_mode", [False, True], ids=["EPSILON", "START_X"])
def test_training_losses_min_snr_match_the_oracle(x0_mode):
    """min_snr:5 at t = [0, n_t - 1] on the micro model: mse, eval-mse and loss within rtol 1e-4 of the oracle, every parameter
    gradient of loss.mean() by the rule of tests/test_backward_gpu.py::test_parameter_gradients_match_oracle: against the
    oracle's fp32 autograd, |d| < 2e-3 (max|g_ref| of the tensor + 1e-3 gmax).  gmax is the largest oracle gradient of THIS
    loss (0.25 / 1.09), not that test's golden gmax (1.25e3, of its probe loss), under which the floor would swallow every
    gradient here.  With "none" the terms are the unweighted path's: 'loss' IS 'mse'.

    Why the oracle runs in its own fp32 and not in float64: the model is defined in fp32, timestep embedding included.  At
    t = n_t - 1 the sinusoid arguments reach 999, where one fp32 ulp of the argument is 6e-5; the oracle evaluated in float64
    differs from the same oracle in fp32 by 2.23e-3 under this very rule (input_blocks.1.1.temporal_attention.qkv.bias, CPU
    against CPU), so a float64 reference asks of the kernels what the reference arithmetic itself does not deliver (the
    native gradients sit at the same 2.2e-3 to 2.3e-3 from it, on the same tensor)."""
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd).train()
    d = {k: v.cuda() for k, v in inp.items()}
    diff = make_diffusion(predict_xstart=x0_mode)
    n = diff.num_timesteps
    t = torch.tensor([0, n - 1])
    noise = torch.from_numpy(recipe.gaussianish("lossWeighting/noise", inp["x0"].numel()).reshape(inp["x0"].shape).astype(np.float32))
    lat, ev = 1.0 - inp["obs_mask"], inp["latent_mask"]
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    call = lambda: diff.training_losses(model, d["x0"], t.cuda(), model_kwargs=mk, noise=noise.cuda(), latent_mask=lat.cuda(),      # noqa: E731
                                        eval_mask=ev.cuda())
    plain = call()
    assert diff.loss_weighting == "none" and plain["loss"] is plain["mse"]
    diff.set_loss_weighting("min_snr", gamma=5)
    w64 = diff.loss_weights()
    terms = call()
    assert list(terms) == ["mse", "eval-mse", "loss"] and terms["loss"] is not terms["mse"]
    assert terms["loss"].requires_grad and not terms["mse"].requires_grad and not terms["eval-mse"].requires_grad
    assert torch.equal(terms["loss"].detach(), terms["mse"] * diff.loss_weight_table("cuda")[t.cuda()])
    model.zero_grad(set_to_none=True)
    terms["loss"].mean().backward()
    torch.cuda.synchronize()
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    oterms = _oracle_weighted_losses(sdo, cfg, inp, do.Tables(do.linear_betas(1000)), t, noise, lat, ev, w64, x0_mode)
    oterms["loss"].mean().backward()
    for k in ("mse", "eval-mse", "loss"):
        got, ref = terms[k].detach().cpu().numpy(), oterms[k].detach().numpy()
        print(f"[min_snr:5 {'START_X' if x0_mode else 'EPSILON'}] {k}: {got} oracle {ref} rel {np.abs(got / ref - 1).max():.2e}")
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=0)
    gmax = max(float(v.grad.abs().max()) for v in sdo.values())
    worst, worst_key = 0.0, None
    for k, p in model.named_parameters():
        ref = sdo[k].grad
        assert p.grad is not None and ref is not None, k
        err = float((p.grad.cpu().double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-3 * gmax)
        if err > worst:
            worst, worst_key = err, k
    print(f"[min_snr:5 {'START_X' if x0_mode else 'EPSILON'}] worst relative gradient error vs oracle: {worst:.2e} ({worst_key}), "
          f"gmax {gmax:.2e}")
    assert gmax > 0 and worst < 2e-3, (worst, worst_key)


# ------------------------------------------------------------------------------------------------ TrainLoop
def _device_loop(cfg, sd, data_seed=0, **kw):
    """``TrainLoop`` at the micro config (ch32, 16 x 16, 4 frames, batch 2) on the device; ``kw``: loss_weighting or nothing."""
    from improved_diffusion.train_util import TrainLoop
    return TrainLoop(model=build_native(cfg, sd).train(), diffusion=make_diffusion(), data=_data(2, 12, 4, 16, data_seed),
                     batch_size=2, microbatch=-1, lr=1e-3, ema_rate="0.9", log_interval=1000, save_interval=10 ** 9,
                     resume_checkpoint="", use_fp16=False, diffusion_space_kwargs={}, fp16_scale_growth=1e-3, schedule_sampler=None,
                     weight_decay=0.01, lr_anneal_steps=0, sample_interval=None, pad_with_random_frames=True, max_frames=4,
                     enc_dec_chunk_size=20, args=argparse.Namespace(resume_id=""), **kw)


def test_captured_micro_step_gathers_the_weight_of_each_steps_t(monkeypatch):
    """Five optimizer steps with min_snr:5 and the training graph on: two eager warm-ups, the capture, two more replays.  In
    every step the returned loss is bitwise mse * wtab[t] for the ``t`` the device saw in THAT step; the steps draw different
    ``t`` with different weights, so a weight frozen at capture time fails here."""
    monkeypatch.delenv("LFVDM_LOSS_WEIGHTING", raising=False)
    monkeypatch.setenv("LFVDM_TRAIN_GRAPH", "1")
    cfg, sd, _ = load_case("micro")
    loop = _device_loop(cfg, sd, loss_weighting="min_snr:5")
    assert loop.diffusion.loss_weighting == "min_snr:5"
    wtab = loop.diffusion.loss_weight_table("cuda")
    seen = []
    inner = loop._graphed_micro_step

    def recording(*a, **k):
        weighted, raw = inner(*a, **k)
        torch.cuda.synchronize()
        t, sampler_w = loop._dev_inputs[2], loop._dev_inputs[3]
        assert t.dtype == torch.int64 and bool((sampler_w == 1).all()), "the uniform sampler's weights are exactly 1"
        seen.append({"t": t.clone(), "mse": weighted["mse"].clone(), "loss": weighted["loss"].clone(), "raw": raw.clone(),
                     "replayed": loop._graph_state.get("graph") is not None})
        return weighted, raw
    monkeypatch.setattr(loop, "_graphed_micro_step", recording)
    torch.manual_seed(1); np.random.seed(1)      # the host draws t: [92, 186] [878, 27] [800, 968] [878, 98] [18, 750]
    for _ in range(5):
        loop.forward_backward()
        loop.optimize_normal()
        loop.step += 1
    loop._flush_loss_log()
    torch.cuda.synchronize()
    assert [s["replayed"] for s in seen] == [False, False, True, True, True]
    for i, s in enumerate(seen):
        w = wtab[s["t"]]
        print(f"[captured weighted step {i}] t {s['t'].tolist()} w {w.tolist()} mse {s['mse'].tolist()} loss {s['raw'].tolist()}")
        assert bool(torch.isfinite(s["mse"]).all()) and float(s["mse"].min()) > 0
        assert torch.equal(s["raw"], s["mse"] * w) and torch.equal(s["loss"], s["raw"])
    ts = [tuple(s["t"].tolist()) for s in seen]
    assert len(set(ts)) > 1, "the steps must not all draw the same t"
    # the premise of the test: a later replay's weights differ from those of the step the graph was captured in
    cap = wtab[seen[2]["t"]]
    assert any(not torch.equal(wtab[s["t"]], cap) for s in seen[3:]), ts
    assert bool(torch.isfinite(loop.arena.p).all())


def _micro_step_arena(monkeypatch, **kw):
    cfg, sd, _ = load_case("micro")
    loop = _device_loop(cfg, sd, **kw)
    torch.manual_seed(11); np.random.seed(11)
    loop.forward_backward()
    torch.cuda.synchronize()
    return loop.arena.g.clone()


def test_quarter_weight_scales_the_gradient_arena_exactly(monkeypatch):
    """LFVDM_DETERMINISTIC=1, a table of 0.25 everywhere: the gradient arena after one micro-step is bitwise 0.25 x the arena of
    the same micro-step with "none" - the backward pass is linear in its seed and a power-of-two scale is exact.  (It also
    pins the new backward launch to lfvdm_masked_mse_bwd's arithmetic, element by element.)"""
    monkeypatch.delenv("LFVDM_LOSS_WEIGHTING", raising=False)
    monkeypatch.setenv("LFVDM_DETERMINISTIC", "1")
    plain = _micro_step_arena(monkeypatch)
    quarter = _micro_step_arena(monkeypatch, loss_weighting={"kind": "table", "table": np.full(1000, 0.25)})
    assert float(plain.abs().max()) > 0
    assert torch.equal(quarter, 0.25 * plain), float((quarter - 0.25 * plain).abs().max())


def _three_weighted_steps():
    cfg, sd, _ = load_case("micro")
    loop = _device_loop(cfg, sd, loss_weighting="min_snr:5")
    torch.manual_seed(17); np.random.seed(17)
    for _ in range(3):
        loop.forward_backward()
        loop.optimize_normal()
        loop.step += 1
    loop._flush_loss_log()
    torch.cuda.synchronize()
    return [loop.arena.p.clone(), loop.exp_avg.clone(), loop.ema_flat[0].clone()]


def test_weighted_training_is_bitwise_repeatable_in_deterministic_mode(monkeypatch):
    """LFVDM_DETERMINISTIC=1: three weighted optimizer steps (two eager, one captured and replayed), run twice from the same
    seeds, end with bitwise equal parameters, first moments and EMA."""
    monkeypatch.delenv("LFVDM_LOSS_WEIGHTING", raising=False)
    monkeypatch.setenv("LFVDM_DETERMINISTIC", "1")
    first, second = _three_weighted_steps(), _three_weighted_steps()
    assert bool(torch.isfinite(first[0]).all())
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    assert not torch.equal(first[0], first[2]), "the optimizer must have moved the parameters away from their EMA"
