"""The variational bound on the MI355X against the reference (tests/golden/vb_*.npz, written by tools/make_vb_golden.py from
the reference's own methods in float64): lfvdm_vb_terms / lfvdm_vb_terms_bwd through the C ABI and through _VbTerm, the branch
case, the closed-form gradient against float64 autograd, training_losses with use_kl=True and the captured micro-step, the
bits-per-dim loops replayed and eager.

Bounds: every comparison is against the float64 fixture, at max(floor, 3 x the fp32 reference's own deviation from it in that
case).  Floors, taken from the corresponding existing tests: relative 1e-4 on per-sample losses (test_xstart_gpu.py's
losses), 2e-4 absolute on x0-hat (its update kernels), and for gradients 2e-3 of the largest reference gradient (its
training gradients).  Every comparison prints error / bound."""
import os

import numpy as np
import pytest
import torch

from oracle import recipe
from conftest import GOLDEN
from test_oracle_golden import load_case
from test_forward_gpu import build_native
from test_vb_cpu import BPD_KEYS, SCHEDULES, make_diffusion, term_cases, vb_float64

pytestmark = pytest.mark.gpu

REL, ATOL, GREL = 1e-4, 2e-4, 2e-3


def _bound(floor, g, key):
    return max(floor, 3.0 * float(g[key]))


def _rel(got, want):
    return float(np.abs(got.double().cpu().numpy() / want - 1).max())


def _grad_err(got, want):
    """worst over the batch rows of max|d| / max|g_ref| of the row"""
    got = got.double().cpu().numpy()
    return max(float(np.abs(got[b] - want[b]).max() / np.abs(want[b]).max()) for b in range(want.shape[0]))


def _launch(diff, xs, xt, out, nz, t, clip, mask, want_pred=True):
    from improved_diffusion import _native as nat
    B = xs.shape[0]
    vb, xm, em = (torch.full((B,), float("nan"), device="cuda") for _ in range(3))
    pred = torch.full_like(xs, float("nan")) if want_pred else None
    x0 = diff.predicts_xstart
    recip, recipm1, c1, c2, post, lv = diff._vb_tables("cuda")
    nat.vb_terms(xs, xt, out, nz, t, recip, recipm1, c1, c2, post, lv, mask, nat.MEAN_X0 if x0 else nat.MEAN_EPS, clip, vb, xm, em, pred)
    return vb, xm, em, pred


def _launch_bwd(diff, xs, xt, out, t, mask, gvec):
    from improved_diffusion import _native as nat
    x0 = diff.predicts_xstart
    recip, recipm1, c1, c2, _, lv = diff._vb_tables("cuda")
    d = torch.full_like(xs, float("nan"))
    # x0 mode: NULL sqrt_recip tables, as lfvdm_update_x0 allows
    nat.vb_terms_bwd(xs, xt, out, t, None if x0 else recip, None if x0 else recipm1, c1, c2, lv, mask, gvec,
                     nat.MEAN_X0 if x0 else nat.MEAN_EPS, 0, d)
    return d


# ------------------------------------------------------------------------------------------------ the two kernels
@pytest.mark.parametrize("tag,resp", SCHEDULES)
def test_kernels_match_the_reference(tag, resp):
    """Term-only cases: epsilon and x0 mean types, FIXED_LARGE and FIXED_SMALL, t = 0, 1, middle, last, clip 0 and 1, with and
    without the per-frame mask - vb, xstart_mse, mse and the dense x0-hat from one launch through the C ABI, the gradient of
    sum(vb) from lfvdm_vb_terms_bwd and from _VbTerm (autograd through _vb_terms_bpd)."""
    g = np.load(os.path.join(GOLDEN, f"vb_terms_{tag}.npz"))
    mask5 = torch.from_numpy(g["mask"]).float().view(3, 2, 1, 1, 1).cuda()
    worst = {}

    def note(name, err, bound, where):
        r = err / bound
        if r > worst.get(name, (0.0,))[0]:
            worst[name] = (r, err, bound, where)
        assert err <= bound, (name, where, err, bound)
    for case, x0 in term_cases(tag):
        xs, xt, nz, out = (torch.from_numpy(g[f"{case}/{k}"]).cuda() for k in ("x_start", "x_t", "noise", "out"))
        t = torch.from_numpy(g[f"{case}/t"]).cuda()
        B = xs.shape[0]
        for small in (False, True):
            diff = make_diffusion(resp, predict_xstart=x0, sigma_small=small)
            for clip in (0, 1):
                for mname, mk in (("nomask", None), ("mask", mask5)):
                    key = f"{case}/{'small' if small else 'large'}/clip{clip}/{mname}"
                    m2 = None if mk is None else mk.reshape(B, 2).contiguous()
                    vb, xm, em, pred = _launch(diff, xs, xt, out, nz, t, clip, m2)
                    torch.cuda.synchronize()
                    for name, got in (("vb", vb), ("xstart_mse", xm), ("mse", em)):
                        note(name, _rel(got, g[f"{key}/{name}"]), _bound(REL, g, f"{key}/ref32_dev/{name}"), key)
                    ep = float((pred.double().cpu() - torch.from_numpy(g[f"{case}/clip{clip}/pred_xstart"])).abs().max())
                    note("pred_xstart", ep, _bound(ATOL, g, f"{case}/clip{clip}/ref32_dev/pred_xstart"), key)
                    # the method: one model call + the same launch; under no_grad the clamp is allowed
                    with torch.no_grad():
                        r = diff._vb_terms_bpd(lambda *a, **k: (out, None), xs, xt, t, clip_denoised=bool(clip), model_kwargs={},
                                               latent_mask=mk)
                    assert torch.equal(r["output"], vb) and torch.equal(r["pred_xstart"], pred) and sorted(r) == ["output", "pred_xstart"]
                    if clip:
                        continue
                    want = g[f"{key}/grad"]
                    gb = _bound(GREL, g, f"{key}/ref32_dev/grad")
                    d = _launch_bwd(diff, xs, xt, out, t, m2, torch.ones(B, device="cuda"))
                    note("grad (C ABI)", _grad_err(d, want), gb, key)
                    o = out.clone().requires_grad_(True)
                    r = diff._vb_terms_bpd(lambda *a, **k: (o, None), xs, xt, t, clip_denoised=False, model_kwargs={}, latent_mask=mk)
                    assert torch.equal(r["output"].detach(), vb)
                    r["output"].sum().backward()
                    assert torch.equal(o.grad, d), "_VbTerm's backward is the one launch"
                    # g[b] scales row b
                    w = torch.tensor([0.5, -2.0, 3.0], device="cuda")
                    d2 = _launch_bwd(diff, xs, xt, out, t, m2, w)
                    assert torch.allclose(d2, d * w.view(B, 1, 1, 1, 1), rtol=1e-6, atol=0)
    for name, (r, err, bound, where) in sorted(worst.items()):
        print(f"[vb kernels {tag}] {name}: worst {err:.2e} of bound {bound:.2e} ({r:.3f}) at {where}")


def test_branch_case():
    """Every branch of the decoder term: exact +-1 and values just inside +-0.999, elements within 3 standard deviations or
    beyond 12 (clamped at 1e-12 in any precision).  vb and the gradient against the reference; the gradient under a clamp is
    exactly zero."""
    g = np.load(os.path.join(GOLDEN, "vb_branch.npz"))
    t = torch.from_numpy(g["t"]).cuda()
    for m in ("eps", "x0"):
        diff = make_diffusion("", predict_xstart=(m == "x0"))
        xs, xt, out = (torch.from_numpy(g[f"{m}/{k}"]).cuda() for k in ("x_start", "x_t", "out"))
        vb, _, _, _ = _launch(diff, xs, xt, out, xt, t, 0, None, want_pred=False)
        d = _launch_bwd(diff, xs, xt, out, t, None, torch.ones(3, device="cuda"))
        torch.cuda.synchronize()
        ev, bv = _rel(vb, g[f"{m}/vb"]), _bound(REL, g, f"{m}/ref32_dev/vb")
        eg, bg = _grad_err(d, g[f"{m}/grad"]), _bound(GREL, g, f"{m}/ref32_dev/grad")
        cl = torch.from_numpy(g[f"{m}/clamped"]).cuda()
        print(f"[vb branch {m}] vb {ev:.2e} ({ev / bv:.3f} of bound {bv:.1e})  grad {eg:.2e} ({eg / bg:.3f} of bound {bg:.1e})  "
              f"clamped share {float(cl.float().mean()):.2f}, largest gradient under a clamp {float(d[cl].abs().max()):.1e}")
        assert ev <= bv and eg <= bg
        assert float(d[cl].abs().max()) == 0.0 and torch.isfinite(d).all()


def _off(x):
    """a contiguous copy of ``x`` whose first element sits one float past a 16-byte boundary"""
    buf = torch.full((x.numel() + 1,), float("nan"), device=x.device, dtype=x.dtype)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("shape,unaligned", [((3, 2, 4, 4, 4), False), ((3, 3, 3, 5, 5), False), ((3, 2, 4, 4, 4), True)],
                         ids=["vector", "scalar", "unaligned"])
def test_every_path_agrees_with_float64_torch(shape, unaligned):
    """gradcheck-style, on the 16-byte path, on a shape whose frames are not a multiple of four floats, and on operands AND
    destinations that start one float past a 16-byte boundary (both fall back to the scalar path): all four forward results
    (vb, xstart_mse, eps_mse, the dense x0-hat; clip 0 and 1) and the closed-form gradient (clip 0, random upstream
    gradients) against a float64 torch evaluation of the reference formula ON THE DEVICE INPUTS, both mean types and
    variance types, t = 0 / 1 / a middle step, masked.  Bounds: max(floor, 3 x the deviation of the same formula evaluated
    by torch in fp32), floors 1e-4 relative (per-row results), 2e-4 (x0-hat), 2e-3 of each row's largest gradient."""
    B = shape[0]
    n = int(np.prod(shape))
    tag = "unaligned" if unaligned else "aligned"
    place = _off if unaligned else (lambda a: a.contiguous())
    gz = lambda k: torch.from_numpy(recipe.gaussianish(f"vbcheck/{shape}/{k}", n).reshape(shape).astype(np.float32)).cuda()      # noqa: E731
    xs, nz, miss = place(0.8 * gz("x0")), place(gz("noise")), gz("miss")
    mask = torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0], [1.0, 1.0, 0.0]], device="cuda")[:, :shape[1]].contiguous()
    w = torch.tensor([1.5, -0.5, 2.0], device="cuda")
    from improved_diffusion.nn import mean_flat

    def mses(diff, p0, xs_, xt_, nz_, t, m5):
        v = lambda a: torch.from_numpy(a).to(p0.device, p0.dtype)[t].view(B, 1, 1, 1, 1)      # noqa: E731
        eps = (v(diff.sqrt_recip_alphas_cumprod) * xt_ - p0) / v(diff.sqrt_recipm1_alphas_cumprod)
        return mean_flat((p0 - xs_) ** 2, m5), mean_flat((eps - nz_) ** 2, m5)
    for x0 in (False, True):
        for small in (False, True):
            diff = make_diffusion("", predict_xstart=x0, sigma_small=small)
            name = f"{shape} {tag} {'x0' if x0 else 'eps'} {'small' if small else 'large'}"
            t = torch.tensor([0, 1, 500], device="cuda")
            ab = torch.from_numpy(diff.alphas_cumprod).float().cuda()[t].view(B, 1, 1, 1, 1)
            xt = place(ab.sqrt() * xs + (1 - ab).sqrt() * nz)
            # the miss is large enough for the clamp to bite in part of the elements
            out = place((xs + 0.2 * (1 - ab).sqrt() * miss) if x0 else (nz + 0.2 * miss))
            m5 = mask.view(B, shape[1], 1, 1, 1)
            for clip in (0, 1):
                o64 = out.double().requires_grad_(True)
                vb64, p64 = vb_float64(diff, xs.double(), xt.double(), o64, t, clip, m5.double())
                xm64, em64 = mses(diff, p64.detach(), xs.double(), xt.double(), nz.double(), t, m5.double())
                o32 = out.clone().requires_grad_(True)
                vb32, p32 = vb_float64(diff, xs, xt, o32, t, clip, m5)       # the same formula, torch fp32 (fp32 table values)
                xm32, em32 = mses(diff, p32.detach(), xs, xt, nz, t, m5)
                from improved_diffusion import _native as nat
                vb, xm, em = (torch.full((B,), float("nan"), device="cuda") for _ in range(3))
                pred = place(torch.full_like(xs, float("nan")))
                recip, recipm1, c1, c2, post, lv = diff._vb_tables("cuda")
                nat.vb_terms(xs, xt, out, nz, t, recip, recipm1, c1, c2, post, lv, mask, nat.MEAN_X0 if x0 else nat.MEAN_EPS, clip,
                             vb, xm, em, pred)
                torch.cuda.synchronize()
                assert pred.data_ptr() % 16 == (4 if unaligned else 0)
                for what, got, w64, w32 in (("vb", vb, vb64, vb32), ("xstart_mse", xm, xm64, xm32), ("eps_mse", em, em64, em32)):
                    want = w64.detach().cpu().numpy()
                    e, b = _rel(got, want), max(REL, 3 * _rel(w32.detach(), want))
                    print(f"[vb paths {name} clip={clip}] {what} {e:.2e} ({e / b:.3f} of bound {b:.1e})")
                    assert e <= b, (name, clip, what, e, b)
                ep = float((pred.double() - p64.detach()).abs().max())
                bp = max(ATOL, 3 * float((p32.detach().double() - p64.detach()).abs().max()))
                print(f"[vb paths {name} clip={clip}] pred_xstart {ep:.2e} ({ep / bp:.3f} of bound {bp:.1e})")
                assert ep <= bp
                if clip:
                    share = float((p64.detach().abs() >= 1).double().mean())
                    assert 0.02 < share < 0.6, share
                    continue
                (vb64 * w.double()).sum().backward()
                (vb32 * w).sum().backward()
                d = place(torch.full_like(xs, float("nan")))
                nat.vb_terms_bwd(xs, xt, out, t, None if x0 else recip, None if x0 else recipm1, c1, c2, lv, mask, w,
                                 nat.MEAN_X0 if x0 else nat.MEAN_EPS, 0, d)
                torch.cuda.synchronize()
                want = o64.grad.cpu().numpy()
                dev32 = _grad_err(o32.grad, want)
                eg, bg = _grad_err(d, want), max(GREL, 3 * dev32)
                print(f"[vb paths {name}] gradient {eg:.2e} ({eg / bg:.3f} of bound {bg:.1e}; torch fp32: {dev32:.2e})")
                assert eg <= bg


def test_refusals():
    from improved_diffusion import _native as nat
    diff = make_diffusion("")
    x = torch.zeros(2, 2, 4, 4, 4, device="cuda")
    t = torch.zeros(2, dtype=torch.int64, device="cuda")
    recip, recipm1, c1, c2, post, lv = diff._vb_tables("cuda")
    vb = torch.zeros(2, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported configuration"):      # the backward is for clip_denoised=False
        nat.vb_terms_bwd(x, x, x, t, recip, recipm1, c1, c2, lv, None, vb, nat.MEAN_EPS, 1, torch.empty_like(x))
    with pytest.raises(RuntimeError, match="invalid shape"):                  # epsilon mode needs its two tables
        nat.vb_terms(x, x, x, None, t, None, None, c1, c2, post, lv, None, nat.MEAN_EPS, 0, vb)
    with pytest.raises(RuntimeError, match="invalid shape"):                  # eps_mse needs the noise (and the tables)
        nat.vb_terms(x, x, x, None, t, recip, recipm1, c1, c2, post, lv, None, nat.MEAN_X0, 0, vb, None, vb.clone())
    with pytest.raises(RuntimeError, match="invalid shape"):
        nat.vb_terms(x, x, x, None, t, recip, recipm1, c1, c2, post, lv, None, 5, 0, vb)
    nat.vb_terms(x, x, x, None, t, None, None, c1, c2, post, lv, None, nat.MEAN_X0, 0, vb)      # x0 mode: NULL tables are fine
    o = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="clip_denoised=False"):
        diff._vb_terms_bpd(lambda *a, **k: (o, None), x, x, t, clip_denoised=True, model_kwargs={})
    torch.cuda.synchronize()


def test_spaced_diffusion_wraps_the_model():
    """_vb_terms_bpd of a SpacedDiffusion hands the model the base process's (rescaled) timesteps, as p_mean_variance does."""
    diff = make_diffusion("50")
    seen = []
    x = torch.zeros(2, 2, 4, 4, 4, device="cuda")

    def model(x_, timesteps=None, **kw):
        seen.append(timesteps.clone())
        return x_, None
    t = torch.tensor([49, 3], device="cuda")
    with torch.no_grad():
        diff._vb_terms_bpd(model, x, x, t, model_kwargs={})
    tm = torch.tensor(diff.timestep_map, device="cuda")[t].float()
    assert torch.equal(seen[0], tm * (1000.0 / 1000)) and float(seen[0][0]) == float(diff.timestep_map[49])


# ------------------------------------------------------------------------------------------------ training
def _train_inputs():
    g = np.load(os.path.join(GOLDEN, "vb_train_micro.npz"))
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd).train()
    d = {k: v.cuda() for k, v in inp.items()}
    noise = torch.from_numpy(recipe.gaussianish("vbTrain/noise", inp["x0"].numel()).reshape(inp["x0"].shape).astype(np.float32)).cuda()
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    return g, model, d, noise, mk, inp


@pytest.mark.parametrize("inplace", [False, True], ids=["autograd", "inplace"])
def test_kl_training_losses_match_the_reference(inplace):
    """training_losses(use_kl=True) -> (loss * weights).mean().backward() at the micro configuration against the reference
    (RESCALED_KL: the term times num_timesteps, clip_denoised=False, the masks ignored), both gradient delivery modes.
    Loss at max(1e-4, 3 x ref32); gradients at the bounds of test_xstart_gpu.py::test_training_losses_match_the_reference
    (2e-3 / 3e-3), or 3 x the fp32 reference's own deviation where that is larger."""
    g, model, d, noise, mk, inp = _train_inputs()
    model.native_grad_accumulation = inplace
    diff = make_diffusion("", use_kl=True)
    terms = diff.training_losses(model, d["x0"], torch.from_numpy(g["t"]).cuda(), model_kwargs=mk, noise=noise,
                                 latent_mask=1 - d["obs_mask"], eval_mask=d["latent_mask"])
    assert list(terms) == ["loss"] and terms["loss"].shape == (2,)
    (terms["loss"] * torch.ones(2, device="cuda")).mean().backward()
    torch.cuda.synchronize()
    el, bl = _rel(terms["loss"].detach(), g["loss"]), _bound(REL, g, "ref32_dev_loss")
    mode = "inplace" if inplace else "autograd"
    print(f"[kl train micro {mode}] loss {terms['loss'].detach().cpu().numpy()} rel {el:.2e} ({el / bl:.3f} of bound {bl:.1e})")
    assert el <= bl
    gmax = float(g["gmax"])
    keys = [str(k) for k in g["keys"]]
    bg, bn = _bound(2e-3, g, "ref32_dev_grad"), _bound(3e-3, g, "ref32_dev_grad")
    worst, worst_n = (0.0, None), (0.0, None)
    for i, (k, p) in enumerate(model.named_parameters()):
        assert k == keys[i] and p.grad is not None, k
        n = min(16, p.numel())
        err = float(np.abs(p.grad.flatten()[:n].double().cpu().numpy() - g["grad_head"][i][:n]).max()) / \
            (float(g["grad_absmax"][i]) + 1e-3 * gmax)
        en = abs(float(p.grad.double().norm()) - float(g["grad_norm"][i])) / \
            (float(g["grad_norm"][i]) + 1e-3 * gmax * np.sqrt(p.numel()))
        worst, worst_n = max(worst, (err, k)), max(worst_n, (en, k))
    print(f"[kl train micro {mode}] worst relative gradient error {worst[0]:.2e} ({worst[0] / bg:.3f} of bound {bg:.1e}, {worst[1]}); "
          f"worst norm deviation {worst_n[0]:.2e} ({worst_n[0] / bn:.3f} of bound {bn:.1e}, {worst_n[1]}); the fp32 reference "
          f"itself: {float(g['ref32_dev_grad']):.2e}")
    assert worst[0] <= bg and worst_n[0] <= bn, (worst, worst_n)


def test_captured_kl_micro_step_replays_the_eager_step(monkeypatch):
    """TrainLoop with a use_kl diffusion, LFVDM_DETERMINISTIC=1: the same micro-batch with the same noise four times - two
    eager steps, the capture, one more replay - at the rule of test_xstart_gpu.py's captured micro-step (2e-5 of the largest
    gradient, losses 1e-6 relative, replay against replay bitwise); then TrainLoop.run_step trains, eager and replayed, and
    logs the loss."""
    from test_train_gpu import make_loop
    from improved_diffusion.logger import logger
    monkeypatch.setenv("LFVDM_DETERMINISTIC", "1")
    g, model, d, noise, mk, inp = _train_inputs()
    loop = make_loop(model, max_frames=inp["x0"].shape[1])
    loop.diffusion = make_diffusion("", use_kl=True)
    orig = loop.diffusion.training_losses
    loop.diffusion.training_losses = lambda *a, **k: orig(*a, noise=noise, **k)
    inputs = (d["x0"], d["frame_indices"], d["obs_mask"], d["latent_mask"], torch.from_numpy(g["t"]).cuda(), torch.ones(2, device="cuda"))
    runs = []
    for n in range(4):
        loop.arena.zero_grad()
        weighted, raw = loop._graphed_micro_step(inputs)
        loop.exchange.micro_step_done()
        torch.cuda.synchronize()
        assert list(weighted) == ["loss"]
        runs.append((raw.clone(), loop.arena.g.clone()))
        assert (loop._graph_state.get("graph") is not None) == (n >= 2)
    el, bl = _rel(runs[0][0], g["loss"]), _bound(REL, g, "ref32_dev_loss")
    scale = float(runs[0][1].abs().max())
    dg_, dl = float((runs[2][1] - runs[0][1]).abs().max()), float((runs[2][0] - runs[0][0]).abs().max())
    print(f"[captured kl micro-step] loss vs reference {el:.2e} ({el / bl:.3f} of bound); replay vs eager: gradients {dg_:.2e} "
          f"({dg_ / (2e-5 * scale):.3f} of bound), losses {dl:.2e}")
    assert el <= bl and scale > 0 and dg_ < 2e-5 * scale and dl <= 1e-6 * float(runs[0][0].abs().max())
    assert torch.equal(runs[2][1], runs[3][1]) and torch.equal(runs[2][0], runs[3][0]), "the replay is bitwise repeatable"
    loop.diffusion.training_losses = orig
    p0 = loop.arena.p.clone()
    torch.manual_seed(3); np.random.seed(3)
    for n in range(4):
        loop.run_step()
        loop._flush_loss_log()
        assert np.isfinite(logger.name2val["loss"]) and logger.name2val["loss"] > 0
        logger.dumpkvs()
        loop.step += 1
    torch.cuda.synchronize()
    assert loop._graph_state.get("graph") is not None
    assert torch.isfinite(loop.arena.p).all() and torch.isfinite(loop.arena.g).all() and not torch.equal(loop.arena.p, p0)


# ------------------------------------------------------------------------------------------------ bits-per-dim loops
def _cfgB():
    cfg, sd, inp = load_case("cfgB")
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    return model, d, mk


def _noise(name, j, shape):
    return torch.from_numpy(recipe.gaussianish(f"vbB/{name}/noise{j}", int(np.prod(shape))).reshape(shape).astype(np.float32)).cuda()


class _given_noise:
    """torch.randn_like returns the recorded draws (the eager route draws its noise there, as the reference does)."""

    def __init__(self, name, shape):
        self.name, self.shape, self.j, self.real = name, shape, 0, torch.randn_like

    def __enter__(self):
        def fake(x):
            z = _noise(self.name, self.j, self.shape)
            self.j += 1
            return z
        torch.randn_like = fake
        return self

    def __exit__(self, *a):
        torch.randn_like = self.real


def _check_bpd(tag, res, g, name):
    ratios = {}
    for k in BPD_KEYS:
        want = g[f"{name}/{k}"]
        assert tuple(res[k].shape) == want.shape, k
        e, b = _rel(res[k], want), _bound(REL, g, f"{name}/ref32_dev/{k}")
        ratios[k] = e / b
        print(f"[bpd {tag}] {k}: {e:.2e} ({e / b:.3f} of bound {b:.1e})")
        assert e <= b, (tag, k, e, b)
    return ratios


def test_bpd_loop_replayed_and_eager_follow_the_reference():
    """calc_bpd_loop on the 50-step schedule at cfg B with the fixture's per-step noise: the replayed evaluation step
    (BpdEvaluator, inject_noise) and the eager per-step route against the reference's five results, and against each
    other within the same bounds."""
    from improved_diffusion.gaussian_diffusion import BpdEvaluator
    g = np.load(os.path.join(GOLDEN, "vb_bpd_cfgB.npz"))
    model, d, mk = _cfgB()
    diff = make_diffusion("50")
    assert np.array_equal(np.array(diff.timestep_map), g["timestep_map"])
    shape = tuple(d["x0"].shape)
    lat = 1 - d["obs_mask"]
    ev = BpdEvaluator(diff, model, shape, True, inject_noise=True)
    ev.begin(d["x0"], mk, lat)
    assert ev.plan.time_steps == 50
    for j, i in enumerate(range(49, -1, -1)):
        ev.noise.copy_(_noise("loop", j, shape))
        ev.step(i)
    torch.cuda.synchronize()
    assert not ev.chain_timed_out()
    prior = diff._prior_bpd(d["x0"], latent_mask=lat)
    rep = {"vb": ev.vb.clone(), "xstart_mse": ev.xstart_mse.clone(), "mse": ev.mse.clone(), "prior_bpd": prior,
           "total_bpd": ev.vb.sum(dim=1) + prior}
    _check_bpd("replayed", rep, g, "loop")
    with _given_noise("loop", shape) as gn:
        eager = diff.calc_bpd_loop(lambda *a, **k: model(*a, **k), d["x0"], clip_denoised=True, model_kwargs=mk, latent_mask=lat)
    assert gn.j == 50 and sorted(eager) == sorted(BPD_KEYS), "a plain callable takes the eager per-step route"
    _check_bpd("eager", eager, g, "loop")
    for k in BPD_KEYS:
        e = float(((rep[k] - eager[k]) / eager[k]).abs().max())
        b = _bound(REL, g, f"loop/ref32_dev/{k}")
        print(f"[bpd replayed vs eager] {k}: {e:.2e} ({e / b:.3f} of bound {b:.1e})")
        assert e <= b


def test_bpd_loop_fast_path_and_2d_t_seq():
    """The public loop on a native model takes the replayed path (its own noise: seeded runs repeat bitwise, another seed
    differs, the values are those of the injected-noise run up to the noise); the 2-D t_seq call - one row of timesteps per
    batch element - runs eagerly and follows the reference."""
    g = np.load(os.path.join(GOLDEN, "vb_bpd_cfgB.npz"))
    model, d, mk = _cfgB()
    diff = make_diffusion("50")
    shape = tuple(d["x0"].shape)
    lat = 1 - d["obs_mask"]
    res = []
    for sd in (5, 5, 6):
        torch.manual_seed(sd)
        res.append(diff.calc_bpd_loop(model, d["x0"], clip_denoised=True, model_kwargs=mk, latent_mask=lat))
    assert len(diff._bpd_evals) == 1 and next(iter(diff._bpd_evals.values())).graph is not None
    for k in BPD_KEYS:
        assert torch.equal(res[0][k], res[1][k]), k
        assert tuple(res[0][k].shape) == g[f"loop/{k}"].shape and torch.isfinite(res[0][k]).all()
    assert not torch.equal(res[0]["vb"], res[2]["vb"])
    assert torch.equal(res[0]["total_bpd"], res[0]["vb"].sum(dim=1) + res[0]["prior_bpd"])
    ratio = (res[0]["total_bpd"].double().cpu().numpy() / g["loop/total_bpd"])      # (reported, not asserted: other noise)
    print(f"[bpd fast path] total_bpd {res[0]['total_bpd'].cpu().numpy()} (own noise) / reference (recorded noise) = {ratio}")
    assert float(res[0]["vb"].min()) > 0
    t2 = g["t_seq_2d"]
    with _given_noise("sub2d", shape) as gn:
        sub = diff.calc_bpd_loop_subsampled(model, d["x0"], clip_denoised=True, model_kwargs=mk, latent_mask=lat, t_seq=t2)
    assert gn.j == t2.shape[1]
    _check_bpd("2-D t_seq", sub, g, "sub2d")


def test_deterministic_mode_is_bitwise_reproducible(monkeypatch):
    """LFVDM_DETERMINISTIC=1: two runs of the forward kernel, of the backward kernel, of training_losses + backward and of the
    seeded loop are bitwise equal."""
    monkeypatch.setenv("LFVDM_DETERMINISTIC", "1")
    g, model, d, noise, mk, inp = _train_inputs()
    diff = make_diffusion("", use_kl=True)
    t = torch.from_numpy(g["t"]).cuda()
    runs = []
    for _ in range(2):
        for p in model.parameters():
            p.grad = None
        terms = diff.training_losses(model, d["x0"], t, model_kwargs=mk, noise=noise)
        terms["loss"].sum().backward()
        torch.cuda.synchronize()
        runs.append((terms["loss"].detach().clone(), [p.grad.clone() for p in model.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    d50 = make_diffusion("50")
    res = []
    for _ in range(2):
        torch.manual_seed(9)
        res.append(d50.calc_bpd_loop(model.eval(), d["x0"], model_kwargs=mk))
    assert all(torch.equal(res[0][k], res[1][k]) for k in BPD_KEYS)


def test_mse_path_and_sampler_are_untouched_by_a_kl_run_in_between():
    """training_losses of an MSE diffusion before and after a KL training step and a bits-per-dim loop on the same model:
    bitwise the same losses; the sampler's plan and launch count are what they were."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    g, model, d, noise, mk, inp = _train_inputs()
    mse, kl = make_diffusion(""), make_diffusion("", use_kl=True)
    t = torch.from_numpy(g["t"]).cuda()
    shape = tuple(d["x0"].shape)

    def mse_terms():
        with torch.no_grad():
            r = mse.training_losses(model, d["x0"], t, model_kwargs=mk, noise=noise, latent_mask=1 - d["obs_mask"], eval_mask=d["latent_mask"])
        return {k: v.clone() for k, v in r.items()}

    def launches():
        s = GraphSampler(make_diffusion("50"), model, shape, True)
        s.begin(d["x"].clone(), mk)
        return len(s.plan.steps), s.extra_launches
    before, n_before = mse_terms(), launches()
    kl.training_losses(model, d["x0"], t, model_kwargs=mk, noise=noise)["loss"].sum().backward()
    make_diffusion("50").calc_bpd_loop(model, d["x0"], model_kwargs=mk)
    after, n_after = mse_terms(), launches()
    print(f"[untouched] sampler (plan launches, extra launches) before {n_before} after {n_after}")
    assert sorted(before) == ["eval-mse", "loss", "mse"] and all(torch.equal(before[k], after[k]) for k in before)
    assert n_before == n_after


def test_chain_timeout_reruns_the_walk(monkeypatch):
    """The persistent-chain timeout protocol without a fault: the plan's abort read-back is stubbed to say "timed out" once.
    evaluate() then says so, switches its plan to one launch per stage, captures the step again and walks a second time;
    the results are complete, and a later walk stays on the per-launch plan."""
    model, d, mk = _cfgB()
    diff = make_diffusion("50")
    shape = tuple(d["x0"].shape)
    ev = diff._bpd_evaluator(model, shape, True)
    torch.manual_seed(1)
    first = ev.evaluate(d["x0"], mk)
    assert ev.plan.chains and ev.chain_timeouts == 0
    calls = []

    def aborted_once():
        calls.append(1)
        return len(calls) == 1
    monkeypatch.setattr(ev.plan, "chains_aborted", aborted_once)
    begins = []
    real_begin = ev.begin
    monkeypatch.setattr(ev, "begin", lambda *a, **k: (begins.append(1), real_begin(*a, **k))[1])
    torch.manual_seed(1)
    again = ev.evaluate(d["x0"], mk)
    assert len(begins) == 2 and ev.chain_timeouts == 1 and not ev.plan.chains and ev.graph is not None
    for a, b in zip(first, again):
        assert a.shape == b.shape == (2, 50) and torch.isfinite(b).all() and float(b.min()) > 0
    ev.evaluate(d["x0"], mk)
    assert len(begins) == 3 and ev.chain_timeouts == 1
