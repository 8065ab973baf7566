"""Generate tests/golden/vb_*.npz by IMPORTING the real reference (development machine only, never the GPU machine; no
test imports this file).

    python tools/make_vb_golden.py [terms] [branch] [train] [bpd]

TEST INFRASTRUCTURE, as oracle/make_golden.py, tools/make_ddim_golden.py and tools/make_xstart_golden.py: nothing of the
reference's source is copied.  The reference's own ``_vb_terms_bpd``, ``training_losses`` (``use_kl=True``),
``calc_bpd_loop`` and ``calc_bpd_loop_subsampled`` and the functions of its ``losses`` module are driven on float64 CPU
tensors with the table gather kept in float64 (``float64_tables``) and, where a network is needed, the float64 oracle
forward.  The reference's plain float32 run from the same inputs is stored next to every float64 result (``ref32_dev``):
the error one correct fp32 implementation has.

Conditioning (asserted here, see ``gen_terms`` / ``gen_branch``): the decoder term at t = 0 has a standard deviation near
0.01, and a probability between fp32 resolution and the 1e-12 clamp is where an fp32 evaluation of 1 + tanh loses
everything.  The parity cases keep every t = 0 element's float64 cdf_delta above 1e-5 (x0 mode: the output's miss is
scaled by sqrt(1 - alphas_cumprod[t])); the branch case puts every element either well inside (within 3 standard
deviations) or far outside (beyond 12: clamped in any precision) and holds exact +-1 and values just inside +-0.999.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import make_golden as mg  # noqa: E402  (puts the reference on sys.path and imports it)
from oracle import recipe, unet_oracle as uo  # noqa: E402
import make_ddim_golden as dg  # noqa: E402  (float64_tables, patched_randn_like, Oracle64: the same helpers)
from improved_diffusion import losses as rl  # noqa: E402  (the REFERENCE's module: its directory is first on sys.path)

OUT = mg.OUT
MISS = 0.2          # the "network" misses its target by 0.2 sigma (the measured well-conditioned range is 0.05 - 0.5)
DEAD = (1e-14, 1e-5)


def make_diffusion(resp="", x0=False, small=False, use_kl=False):
    d = mg.rsu.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, rescale_timesteps=True, rescale_learned_sigmas=True,
                                         predict_xstart=x0, sigma_small=small, use_kl=use_kl,
                                         diffusion_space_kwargs=dict(dg.PIXEL))
    assert d.model_mean_type == (mg.rgd.ModelMeanType.START_X if x0 else mg.rgd.ModelMeanType.EPSILON)
    assert d.model_var_type == (mg.rgd.ModelVarType.FIXED_SMALL if small else mg.rgd.ModelVarType.FIXED_LARGE)
    return d


def rel(a32, a64):
    return float(((a32.double() - a64) / a64).abs().max())


def term_quantities(diff, model, x_start, x_t, noise, t, clip, mask):
    """What one step of the reference's calc_bpd_loop_subsampled computes (:853-868), from its own methods."""
    out = diff._vb_terms_bpd(model, x_start=x_start, x_t=x_t, t=t, clip_denoised=bool(clip), model_kwargs={}, latent_mask=mask)
    pred = out["pred_xstart"]
    xm = mg.rgd.mean_flat((pred - x_start) ** 2, mask=mask)
    eps = diff._predict_eps_from_xstart(x_t, t, pred)
    em = mg.rgd.mean_flat((eps - noise) ** 2, mask=mask)
    return out["output"], xm, em, pred


def decoder_probabilities(diff, x_start, x_t, out, t, x0, clip):
    """float64 cdf_plus, 1 - cdf_min, cdf_delta of the decoder term, from the reference's own functions."""
    v = lambda a: torch.from_numpy(a)[t].view(-1, 1, 1, 1, 1)      # noqa: E731
    p0 = out if x0 else v(diff.sqrt_recip_alphas_cumprod) * x_t - v(diff.sqrt_recipm1_alphas_cumprod) * out
    if clip:
        p0 = p0.clamp(-1, 1)
    mean = v(diff.posterior_mean_coef1) * p0 + v(diff.posterior_mean_coef2) * x_t
    lv = np.log(np.append(diff.posterior_variance[1], diff.betas[1:])) if diff.model_var_type == mg.rgd.ModelVarType.FIXED_LARGE \
        else diff.posterior_log_variance_clipped
    inv = torch.exp(-0.5 * v(lv))
    c = x_start - mean
    cp = rl.approx_standard_normal_cdf(inv * (c + 1.0 / 255.0))
    cm = rl.approx_standard_normal_cdf(inv * (c - 1.0 / 255.0))
    return cp, 1.0 - cm, cp - cm, c * inv


def gen_terms():
    """Term-only cases (no network: the model returns a given tensor): epsilon and x0 mean types, FIXED_LARGE and
    FIXED_SMALL, the 1000-step and a 50-step schedule, t containing 0, 1, a middle step and T - 1, clip 0 and 1, with and
    without a per-frame mask."""
    B, shape = 3, (3, 2, 4, 4, 4)
    n = int(np.prod(shape))
    mask = torch.tensor([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], dtype=torch.float64).view(B, 2, 1, 1, 1)
    worst = {}
    for tag, resp in (("d1000", ""), ("s50", "50")):      # one file per schedule (each within the size of the other fixtures)
        out = {"shape": np.array(shape, dtype=np.int64), "mask": mask.numpy().reshape(B, 2)}
        for x0 in (False, True):
            mname = "x0" if x0 else "eps"
            nt = make_diffusion(resp).num_timesteps
            out[f"{tag}/num_timesteps"] = np.int64(nt)
            for ti, tvec in enumerate(([0, 1, nt // 2], [nt - 1, 0, nt // 3])):
                case = f"{tag}/{mname}/t{ti}"
                t = torch.tensor(tvec)
                g1, g2, g3 = (recipe.gaussianish(f"vb/{case}/{k}", n).reshape(shape) for k in ("x0", "noise", "miss"))
                ab = make_diffusion(resp).alphas_cumprod[tvec].reshape(B, 1, 1, 1, 1)
                xs = (0.8 * g1).astype(np.float32)
                nz = g2.astype(np.float32)
                xt = (np.sqrt(ab) * xs.astype(np.float64) + np.sqrt(1 - ab) * nz.astype(np.float64)).astype(np.float32)
                mo = (xs + MISS * np.sqrt(1 - ab) * g3 if x0 else nz + MISS * g3).astype(np.float32)
                out[f"{case}/t"] = t.numpy()
                out[f"{case}/x_start"], out[f"{case}/x_t"], out[f"{case}/noise"], out[f"{case}/out"] = xs, xt, nz, mo
                xs32, xt32, nz32, mo32 = (torch.from_numpy(a) for a in (xs, xt, nz, mo))
                xs64, xt64, nz64, mo64 = (a.double() for a in (xs32, xt32, nz32, mo32))
                for small in (False, True):
                    diff = make_diffusion(resp, x0, small)
                    vname = "small" if small else "large"
                    dec = t == 0
                    _, _, delta, _ = decoder_probabilities(diff, xs64, xt64, mo64, t, x0, 0)
                    dmin = float(delta[dec].min())
                    assert dmin >= 1e-5, (case, vname, dmin)      # the share below 1e-5 is ZERO
                    out[f"{case}/{vname}/min_cdf_delta_t0"] = np.float64(dmin)
                    for clip in (0, 1):
                        for mk_name, mk in (("nomask", None), ("mask", mask)):
                            key = f"{case}/{vname}/clip{clip}/{mk_name}"
                            m64 = lambda *a, **k: (mo64, None)      # noqa: E731
                            m32 = lambda *a, **k: (mo32, None)      # noqa: E731
                            with dg.float64_tables():
                                r64 = term_quantities(diff, m64, xs64, xt64, nz64, t, clip, mk)
                            r32 = term_quantities(diff, m32, xs32, xt32, nz32, t, clip, None if mk is None else mk.float())
                            assert all(a.dtype == torch.float64 for a in r64)
                            for name, a64, a32 in zip(("vb", "xstart_mse", "mse"), r64, r32):
                                out[f"{key}/{name}"] = a64.numpy()
                                out[f"{key}/ref32_dev/{name}"] = np.float64(rel(a32, a64))
                                worst[name] = max(worst.get(name, 0.0), rel(a32, a64))
                            if mk is None and not small:      # x0-hat depends on neither the variance type nor the mask
                                out[f"{case}/clip{clip}/pred_xstart"] = r64[3].numpy()
                                out[f"{case}/clip{clip}/ref32_dev/pred_xstart"] = np.float64((r32[3].double() - r64[3]).abs().max())
                                if clip:
                                    share = float((r64[3].abs() >= 1).double().mean())
                                    assert 0.02 < share < 0.6, (case, share)
                                    out[f"{case}/clamp_share"] = np.float64(share)
                            else:
                                assert torch.equal(r64[3], torch.from_numpy(out[f"{case}/clip{clip}/pred_xstart"]))
                            if clip == 0:      # d sum(vb) / d out
                                o64 = mo64.clone().requires_grad_(True)
                                with dg.float64_tables():
                                    diff._vb_terms_bpd(lambda *a, **k: (o64, None), x_start=xs64, x_t=xt64, t=t, clip_denoised=False,
                                                       model_kwargs={}, latent_mask=mk)["output"].sum().backward()
                                o32 = mo32.clone().requires_grad_(True)
                                diff._vb_terms_bpd(lambda *a, **k: (o32, None), x_start=xs32, x_t=xt32, t=t, clip_denoised=False,
                                                   model_kwargs={}, latent_mask=None if mk is None else mk.float())["output"].sum().backward()
                                gdev = max(float((o32.grad[b].double() - o64.grad[b]).abs().max() / o64.grad[b].abs().max())
                                           for b in range(B))
                                out[f"{key}/grad"] = o64.grad.numpy()
                                out[f"{key}/ref32_dev/grad"] = np.float64(gdev)      # of each row's largest gradient
                                worst["grad"] = max(worst.get("grad", 0.0), gdev)
                print(f"[terms {case}] t = {tvec}: ok")
        path = os.path.join(OUT, f"vb_terms_{tag}.npz")
        np.savez_compressed(path, **out)
        print(f"[terms {tag}] ok", os.path.getsize(path), "bytes")
    print("[terms] fp32 reference vs float64, worst over all cases:", {k: f"{v:.2e}" for k, v in worst.items()})


def gen_branch():
    """Every branch of the decoder term at t = 0: x_start holds exact +-1 (the open-ended bins), values just inside +-0.999
    and ordinary values; the model mean sits within 3 standard deviations of x_start or beyond 12.  No probability that
    the term takes a logarithm of lies in the dead zone [1e-14, 1e-5]: the clamped elements are clamped in any precision."""
    B, shape = 3, (3, 2, 4, 4, 4)
    n = int(np.prod(shape))
    t = torch.tensor([0, 0, 0])
    out = {"shape": np.array(shape, dtype=np.int64), "t": t.numpy()}
    u = recipe.gaussianish("vb/branch/u", n).reshape(-1)
    special = np.array([1.0, -1.0, 0.9989, -0.9989, 0.9985, -0.9985])
    xs = (0.6 * np.tanh(recipe.gaussianish("vb/branch/x0", n))).reshape(-1)
    xs[::4] = special[np.arange(len(xs[::4])) % 6]
    xs = xs.reshape(shape).astype(np.float32)
    # in units of the decoder's standard deviation: even positions within 3, odd positions beyond 12 (either side)
    k = np.where(np.arange(n) % 2 == 0, 3.0 * np.tanh(u), np.sign(u + 1e-9) * (12.0 + 4.0 * np.abs(np.tanh(u))))
    k = np.roll(k, 1)[:n].reshape(shape)      # decouple the pattern from the stride of the special values
    for x0 in (False, True):
        mname = "x0" if x0 else "eps"
        diff = make_diffusion("", x0, False)
        std = np.sqrt(diff.posterior_variance[1])
        r, rm1 = diff.sqrt_recip_alphas_cumprod[0], diff.sqrt_recipm1_alphas_cumprod[0]
        nz = recipe.gaussianish(f"vb/branch/{mname}/noise", n).reshape(shape).astype(np.float32)
        xt = (np.sqrt(diff.alphas_cumprod[0]) * xs.astype(np.float64) + np.sqrt(1 - diff.alphas_cumprod[0]) * nz).astype(np.float32)
        p0 = xs.astype(np.float64) - k * std      # posterior_mean_coef1[0] = 1, coef2[0] = 0: the mean IS x0-hat
        mo = (p0 if x0 else (r * xt.astype(np.float64) - p0) / rm1).astype(np.float32)
        xs64, xt64, mo64 = (torch.from_numpy(a).double() for a in (xs, xt, mo))
        cp, om, delta, kk = decoder_probabilities(diff, xs64, xt64, mo64, t, x0, 0)
        used = torch.where(xs64 < -0.999, cp, torch.where(xs64 > 0.999, om, delta))
        dead = (used >= DEAD[0]) & (used <= DEAD[1])
        assert not bool(dead.any()), (mname, int(dead.sum()))
        assert bool(((kk.abs() < 3.2) | (kk.abs() > 11.5)).all()), float(kk.abs().max())
        clamped = used < 1e-12
        low, high = xs64 < -0.999, xs64 > 0.999
        for name, sel in (("low", low), ("high", high), ("mid", ~low & ~high)):
            assert bool((sel & clamped).any()) and bool((sel & ~clamped).any()), (mname, name)
        o64 = mo64.clone().requires_grad_(True)
        with dg.float64_tables():
            vb = diff._vb_terms_bpd(lambda *a, **kw: (o64, None), x_start=xs64, x_t=xt64, t=t, clip_denoised=False, model_kwargs={})["output"]
        vb.sum().backward()
        assert float(o64.grad[clamped].abs().max()) == 0.0, "the gradient under a clamp is zero"
        o32 = mo64.float().requires_grad_(True)
        vb32 = diff._vb_terms_bpd(lambda *a, **kw: (o32, None), x_start=xs64.float(), x_t=xt64.float(), t=t, clip_denoised=False,
                                  model_kwargs={})["output"]
        vb32.sum().backward()
        gdev = max(float((o32.grad[b].double() - o64.grad[b]).abs().max() / o64.grad[b].abs().max()) for b in range(B))
        out[f"{mname}/x_start"], out[f"{mname}/x_t"], out[f"{mname}/out"] = xs, xt, mo
        out[f"{mname}/vb"], out[f"{mname}/grad"], out[f"{mname}/clamped"] = vb.detach().numpy(), o64.grad.numpy(), clamped.numpy()
        out[f"{mname}/ref32_dev/vb"], out[f"{mname}/ref32_dev/grad"] = np.float64(rel(vb32.detach(), vb.detach())), np.float64(gdev)
        print(f"[branch {mname}] vb {vb.detach().numpy()}  clamped share {float(clamped.double().mean()):.2f}  low / high / mid "
              f"{int(low.sum())} / {int(high.sum())} / {int((~low & ~high).sum())}  fp32 reference: vb {rel(vb32.detach(), vb.detach()):.2e} "
              f"grad {gdev:.2e}")
    path = os.path.join(OUT, "vb_branch.npz")
    np.savez_compressed(path, **out)
    print("[branch] ok", os.path.getsize(path), "bytes")


def gen_train():
    """training_losses with use_kl=True (RESCALED_KL) -> (loss * weights).mean().backward() at the micro configuration,
    float64 through the oracle's autograd; the reference's fp32 model next to it (the layout of xstart_train_micro.npz)."""
    kw, B, T, H, n_pad = mg.CONFIGS["micro"]
    cfg = uo.make_cfg(**kw)
    model32, sd = mg.build_reference_model(cfg)
    model32.train()
    inp = mg.tt(recipe.make_inputs("micro", B, T, cfg["in_channels"], H, H, n_pad=n_pad))
    diff = make_diffusion("", use_kl=True)
    assert diff.loss_type == mg.rgd.LossType.RESCALED_KL
    t = torch.tensor([700, 123])
    noise = torch.from_numpy(recipe.gaussianish("vbTrain/noise", inp["x0"].numel()).reshape(inp["x0"].shape).astype(np.float32))
    mk = dict(frame_indices=inp["frame_indices"], obs_mask=inp["obs_mask"], latent_mask=inp["latent_mask"], x0=inp["x0"])
    lat, ev = 1 - inp["obs_mask"], inp["latent_mask"]
    sd64 = {k: p.double().requires_grad_(True) for k, p in sd.items()}
    m64 = dg.Oracle64(cfg, sd)
    m64.sd = sd64
    with dg.float64_tables():
        l64 = diff.training_losses(m64, inp["x0"].double(), t, model_kwargs=mk, noise=noise.double(), latent_mask=lat.double(),
                                   eval_mask=ev.double())
    assert list(l64) == ["loss"] and l64["loss"].dtype == torch.float64
    (l64["loss"] * torch.ones(B, dtype=torch.float64)).mean().backward()
    l32 = diff.training_losses(model32, inp["x0"], t, model_kwargs=mk, noise=noise, latent_mask=lat, eval_mask=ev)
    (l32["loss"] * torch.ones(B)).mean().backward()
    keys = [n for n, _ in model32.named_parameters()]
    g64 = [sd64[k].grad for k in keys]
    g32 = [p.grad for p in model32.parameters()]
    assert all(g is not None for g in g64)
    gmax = max(float(g.abs().max()) for g in g64)
    grel = max(float((a.double() - b).abs().max()) / (float(b.abs().max()) + 1e-3 * gmax) for a, b in zip(g32, g64))
    ldev = rel(l32["loss"].detach(), l64["loss"].detach())
    print(f"[train micro] loss {l64['loss'].detach().numpy()}  fp32 reference vs float64: loss rel {ldev:.2e}, "
          f"worst relative gradient deviation {grel:.2e}")
    head = lambda ts_: np.stack([np.resize(x.flatten()[:16].numpy(), 16) for x in ts_])      # noqa: E731
    path = os.path.join(OUT, "vb_train_micro.npz")
    np.savez_compressed(
        path, keys=np.array(keys), t=t.numpy(), loss=l64["loss"].detach().numpy(),
        grad_norm=np.array([float(g.norm()) for g in g64]), grad_head=head(g64),
        grad_absmax=np.array([float(g.abs().max()) for g in g64]), gmax=np.float64(gmax),
        ref32_dev_loss=np.float64(ldev), ref32_dev_grad=np.float64(grel))
    print("[train] ok", os.path.getsize(path), "bytes")


BPD_KEYS = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")
T_SEQ_2D = np.array([[49, 10, 0, 33], [30, 1, 25, 49]])


def gen_bpd():
    """calc_bpd_loop on the 50-step schedule at cfg B with recorded per-step noise, and one calc_bpd_loop_subsampled call
    with a 2-D t_seq (one row of timesteps per batch element)."""
    cfg, sd, model32, inp, mk = dg.cfgB()
    shape = tuple(inp["x0"].shape)
    diff = make_diffusion("50")
    assert diff.num_timesteps == 50
    m64 = dg.Oracle64(cfg, sd)
    lat = 1 - inp["obs_mask"]
    body = {"timestep_map": np.array(diff.timestep_map, dtype=np.int64), "t_seq_2d": T_SEQ_2D}

    def noises(tag, count):
        return [torch.from_numpy(recipe.gaussianish(f"{tag}/noise{j}", int(np.prod(shape))).reshape(shape).astype(np.float32))
                for j in range(count)]
    for name, count, call in (
            ("loop", 50, lambda m, x, l: diff.calc_bpd_loop(m, x, clip_denoised=True, model_kwargs=mk, latent_mask=l)),
            ("sub2d", T_SEQ_2D.shape[1], lambda m, x, l: diff.calc_bpd_loop_subsampled(m, x, clip_denoised=True, model_kwargs=mk,
                                                                                        latent_mask=l, t_seq=T_SEQ_2D))):
        with dg.patched_randn_like(noises(f"vbB/{name}", count)), dg.float64_tables(), torch.no_grad():
            r64 = call(m64, inp["x0"].double(), lat.double())
        with dg.patched_randn_like(noises(f"vbB/{name}", count)), torch.no_grad():
            r32 = call(model32, inp["x0"].clone(), lat)
        assert sorted(r64) == sorted(BPD_KEYS) and all(r64[k].dtype == torch.float64 for k in BPD_KEYS)
        assert float((r64["total_bpd"] - r64["vb"].sum(dim=1) - r64["prior_bpd"]).abs().max()) < 1e-12
        for k in BPD_KEYS:
            body[f"{name}/{k}"] = r64[k].numpy()
            body[f"{name}/ref32_dev/{k}"] = np.float64(rel(r32[k], r64[k]))
        print(f"[bpd {name}] total_bpd {r64['total_bpd'].numpy()} prior_bpd {r64['prior_bpd'].numpy()}; fp32 reference vs float64:",
              {k: f"{float(body[f'{name}/ref32_dev/{k}']):.2e}" for k in BPD_KEYS})
    path = os.path.join(OUT, "vb_bpd_cfgB.npz")
    np.savez_compressed(path, **body)
    print("[bpd] ok", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    todo = sys.argv[1:] or ["terms", "branch", "train", "bpd"]
    for name in todo:
        {"terms": gen_terms, "branch": gen_branch, "train": gen_train, "bpd": gen_bpd}[name]()
