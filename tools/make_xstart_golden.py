"""Generate tests/golden/xstart_*.npz by IMPORTING the real reference built with ``predict_xstart=True`` (development
machine only, never the GPU machine; no test imports this file).

    python tools/make_xstart_golden.py [update] [traj] [window] [train]

TEST INFRASTRUCTURE, as oracle/make_golden.py and tools/make_ddim_golden.py: nothing of the reference's source is copied.
The reference's own ``GaussianDiffusion`` / ``SpacedDiffusion`` methods (``p_sample``, ``p_mean_variance``, ``ddim_sample``,
``ddim_reverse_sample``, ``ddim_sample_loop_progressive``, ``training_losses``) of a diffusion object whose
``model_mean_type`` is START_X are driven on float64 CPU tensors with their table gather kept in float64
(``float64_tables``) and the float64 oracle forward as the network.  The reference's plain float32 run from the same inputs
is stored next to every fixture (``ref32_dev``): the error one correct fp32 implementation has.
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
import make_ddim_golden as dg  # noqa: E402  (float64_tables, patched_randn_like, Oracle64, folded: the same helpers)

OUT = mg.OUT
ETAS = dg.ETAS
CLAMP_SHARE = (0.02, 0.6)      # every update case: the clamp bites in a real share of the elements, and leaves a real share


def make_diffusion(resp):
    d = mg.rsu.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, rescale_timesteps=True, rescale_learned_sigmas=True,
                                         predict_xstart=True, diffusion_space_kwargs=dict(dg.PIXEL))
    assert d.model_mean_type == mg.rgd.ModelMeanType.START_X
    return d


def gen_update():
    """Update-only cases (no network): p_sample / p_mean_variance, ddim_sample at eta 0 / 0.5 / 1 and ddim_reverse_sample on
    a model that returns a given x0-hat, scaled so that the clamp bites in part of the elements."""
    B, shape = 3, (3, 2, 4, 4, 4)
    n = int(np.prod(shape))
    v = lambda a: torch.from_numpy(a).view(B, 1, 1, 1, 1)      # noqa: E731
    out = {"shape": np.array(shape, dtype=np.int64), "etas": np.array(ETAS)}
    for tag, resp in (("d1000", ""), ("ddim50", "ddim50")):
        diff = make_diffusion(resp)
        nt = diff.num_timesteps
        out[f"{tag}/num_timesteps"] = np.int64(nt)
        for eta in ETAS:
            out[f"{tag}/eta{eta}/sigma"] = dg.folded(diff, eta, False)[2]
        out[f"{tag}/p/sigma"] = np.exp(0.5 * np.log(np.append(diff.posterior_variance[1], diff.betas[1:])))
        for ti, tvec in enumerate(([0, 1, nt // 2], [nt - 1, nt // 3, 1])):
            case = f"{tag}/t{ti}"
            t = torch.tensor(tvec)
            g1, g2, g3 = (recipe.gaussianish(f"xstart/{case}/{k}", n).reshape(shape) for k in ("x0", "noise", "miss"))
            z = recipe.gaussianish(f"xstart/{case}/z", n).reshape(shape).astype(np.float32)
            ab = diff.alphas_cumprod[tvec].reshape(B, 1, 1, 1, 1)
            x = (np.sqrt(ab) * 0.8 * g1 + np.sqrt(1 - ab) * g2).astype(np.float32)
            mo = (0.8 * g1 + 0.15 * g3).astype(np.float32)      # the "network": the clean 0.8-sigma x0, missed by 0.15 sigma
            out[f"{case}/t"], out[f"{case}/x"], out[f"{case}/out"], out[f"{case}/z"] = t.numpy(), x, mo, z
            x64, mo64, z64 = (torch.from_numpy(a).double() for a in (x, mo, z))
            model = lambda x_, timesteps=None, **kw: (mo64, None)      # noqa: E731
            share = float((mo64.abs() > 1).double().mean())
            assert CLAMP_SHARE[0] < share < CLAMP_SHARE[1], (case, share)
            out[f"{case}/clamp_share"] = np.float64(share)
            print(f"[update {case}] t = {tvec}: clamp bites in {100 * share:.1f} % of the elements")
            nz = (t != 0).double().view(B, 1, 1, 1, 1)
            for clip in (0, 1):
                with dg.patched_randn_like([z64]), dg.float64_tables():
                    r = diff.p_sample(model, x64, t, clip_denoised=bool(clip), model_kwargs={})
                    m = diff.p_mean_variance(model, x64, t, clip_denoised=bool(clip), model_kwargs={})
                assert r["sample"].dtype == torch.float64 and m["mean"].dtype == torch.float64
                want_pred = mo64.clamp(-1, 1) if clip else mo64
                assert torch.equal(r["pred_xstart"], want_pred) and torch.equal(m["pred_xstart"], want_pred)
                out[f"{case}/clip{clip}/p/sample"], out[f"{case}/clip{clip}/p/mean"] = r["sample"].numpy(), m["mean"].numpy()
                out[f"{case}/clip{clip}/pred_xstart"] = want_pred.numpy()
                out[f"{case}/clip{clip}/p/variance"] = m["variance"][:, 0, 0, 0, 0].numpy()
                out[f"{case}/clip{clip}/p/log_variance"] = m["log_variance"][:, 0, 0, 0, 0].numpy()
                d = float((m["mean"] + nz * v(out[f"{tag}/p/sigma"][tvec]) * z64 - r["sample"]).abs().max())
                assert d < 1e-13 * max(1.0, float(r["sample"].abs().max())), (case, clip, "p", d)
                for eta in ETAS:
                    with dg.patched_randn_like([z64]), dg.float64_tables():
                        r = diff.ddim_sample(model, x64, t, clip_denoised=bool(clip), model_kwargs={}, eta=eta)
                    assert torch.equal(r["pred_xstart"], want_pred)
                    out[f"{case}/clip{clip}/eta{eta}/sample"] = r["sample"].numpy()
                    # the folded form of the epsilon mode IS the reference's rule in this mode too: checked in float64
                    k1, k2, sg = (v(a[tvec]) for a in dg.folded(diff, eta, False))
                    d = float((k1 * want_pred + k2 * x64 + nz * sg * z64 - r["sample"]).abs().max())
                    assert d < 1e-12 * max(1.0, float(r["sample"].abs().max())), (case, clip, eta, d)
                with dg.float64_tables():
                    r = diff.ddim_reverse_sample(model, x64, t, clip_denoised=bool(clip), model_kwargs={}, eta=0.0)
                out[f"{case}/clip{clip}/reverse/sample"] = r["sample"].numpy()
                k1, k2, _ = (v(a[tvec]) for a in dg.folded(diff, 0.0, True))
                d = float((k1 * want_pred + k2 * x64 - r["sample"]).abs().max())
                assert d < 1e-12 * max(1.0, float(r["sample"].abs().max())), (case, clip, "reverse", d)
    path = os.path.join(OUT, "xstart_update.npz")
    np.savez_compressed(path, **out)
    print("[update] ok", os.path.getsize(path), "bytes")


def _store(body, prefix, t64, t32, stride=(4, 8)):
    """sample / pred_xstart of the float64 steps, compact, and the fp32 reference's per-step deviation from them."""
    for key in ("sample", "pred_xstart"):
        full = torch.stack([o[key] for o in t64])
        assert full.dtype == torch.float64
        for k, val in mg._compact(full, stride).items():
            body[f"{prefix}/{key}/{k}"] = val
        dev = np.array([float((a[key].double() - b[key]).abs().max()) for a, b in zip(t32, t64)])
        body[f"{prefix}/ref32_dev/{key}"] = dev
        print(f"[{prefix}] {key}: fp32 reference vs float64, per step:", " ".join(f"{x:.2e}" for x in dev))


def p_steps(diff, model, x, mk, steps, noises):
    """The reference's p_sample for the timestep indices ``steps`` from ``x`` with the given per-step noise."""
    outs = []
    B = x.shape[0]
    for i, z in zip(steps, noises):
        with dg.patched_randn_like([z]), torch.no_grad():
            o = diff.p_sample(model, x, torch.tensor([i] * B), clip_denoised=True, model_kwargs=mk)
        outs.append(o)
        x = o["sample"]
    return outs


def _noises(tag, n_steps, shape):
    return [torch.from_numpy(recipe.gaussianish(f"{tag}/noise{j}", int(np.prod(shape))).reshape(shape).astype(np.float32))
            for j in range(n_steps)]


def gen_traj():
    """cfg B: three p_sample steps from t = 999 with recorded noise; ddim10 at eta = 0 (all 10 steps) and at eta = 1 (4 steps,
    recorded noise)."""
    cfg, sd, model32, inp, mk = dg.cfgB()
    shape = tuple(inp["x"].shape)
    m64 = dg.Oracle64(cfg, sd)
    body = {}
    diff = make_diffusion("")
    nz = _noises("xstartB/p", 3, shape)
    with dg.float64_tables():
        t64 = p_steps(diff, m64, inp["x"].double(), mk, (999, 998, 997), nz)
    t32 = p_steps(diff, model32, inp["x"].clone(), mk, (999, 998, 997), nz)
    _store(body, "p", t64, t32)
    diff = make_diffusion("ddim10")
    assert diff.num_timesteps == 10
    for name, eta, n_steps in (("eta0", 0.0, 10), ("eta1", 1.0, 4)):
        nz = _noises(f"xstartB/{name}", n_steps, shape)
        with dg.float64_tables():
            t64 = dg.chain(diff, m64, inp["x"].double(), mk, eta, nz, n_steps)
        t32 = dg.chain(diff, model32, inp["x"].clone(), mk, eta, nz, n_steps)
        _store(body, name, t64, t32)
    body["timestep_map"] = np.array(diff.timestep_map, dtype=np.int64)
    path = os.path.join(OUT, "xstart_traj_cfgB.npz")
    np.savez_compressed(path, **body)
    print("[traj] ok", os.path.getsize(path), "bytes")


def gen_window():
    """The K = 14 window of cfg D (oracle/make_golden.py::gen_sampler_cfgD_window's inputs and legs) on 250-step respacing:
    the first three and the last two p_sample steps with recorded noise."""
    import json
    kw, _, _, H, _ = mg.CONFIGS["cfgB"]
    cfg = uo.make_cfg(**kw)
    model32, sd = mg.build_reference_model(cfg)
    with open(os.path.join(OUT, "schemes.json")) as f:
        case = next(c for c in json.load(f) if (c["scheme"], c["video_length"], c["n_obs"], c["max_frames"], c["step_size"])
                    == ("hierarchy-2", 1000, 36, 20, 10))
    K = 14
    obs_idx, lat_idx = next(w for w in case["windows"] if len(w[0]) + len(w[1]) == K)
    tag = f"cfgD_w{K}"
    inp = mg.tt(recipe.make_inputs(tag, 1, K, cfg["in_channels"], H, H))
    fi = torch.tensor([list(obs_idx) + list(lat_idx)], dtype=torch.long)
    obs = torch.zeros(1, K, 1, 1, 1)
    obs[:, :len(obs_idx)] = 1.0
    mk = dict(frame_indices=fi, obs_mask=obs, latent_mask=1 - obs, x0=inp["x0"])
    diff = make_diffusion("250")
    assert diff.num_timesteps == 250
    shape = tuple(inp["x"].shape)
    body = {"frame_indices": fi.numpy(), "n_obs": np.int64(len(obs_idx))}
    m64 = dg.Oracle64(cfg, sd)
    for leg, steps, x in (("top", (249, 248, 247), inp["x"].clone()), ("bottom", (1, 0), (0.5 * inp["x"] + 0.5 * inp["x0"]).clone())):
        nz = _noises(f"xstartD/{leg}", len(steps), shape)
        with dg.float64_tables():
            t64 = p_steps(diff, m64, x.double(), mk, steps, nz)
        t32 = p_steps(diff, model32, x.clone(), mk, steps, nz)
        _store(body, leg, t64, t32, stride=(2, 2))
    path = os.path.join(OUT, "xstart_window_cfgD.npz")
    np.savez_compressed(path, **body)
    print("[window] ok", os.path.getsize(path), "bytes")


def gen_train():
    """One optimizer step's worth of training_losses -> (loss * weights).mean().backward() at the micro configuration: the
    regression target is x_start.  float64 through the oracle's autograd; the reference's fp32 model next to it."""
    kw, B, T, H, n_pad = mg.CONFIGS["micro"]
    cfg = uo.make_cfg(**kw)
    model32, sd = mg.build_reference_model(cfg)
    model32.train()
    inp = mg.tt(recipe.make_inputs("micro", B, T, cfg["in_channels"], H, H, n_pad=n_pad))
    diff = make_diffusion("")
    t = torch.tensor([700, 123])
    noise = torch.from_numpy(recipe.gaussianish("xstartTrain/noise", inp["x0"].numel()).reshape(inp["x0"].shape).astype(np.float32))
    mk = dict(frame_indices=inp["frame_indices"], obs_mask=inp["obs_mask"], latent_mask=inp["latent_mask"], x0=inp["x0"])
    lat, ev = 1 - inp["obs_mask"], inp["latent_mask"]
    sd64 = {k: p.double().requires_grad_(True) for k, p in sd.items()}
    m64 = dg.Oracle64(cfg, sd)
    m64.sd = sd64
    with dg.float64_tables():
        l64 = diff.training_losses(m64, inp["x0"].double(), t, model_kwargs=mk, noise=noise.double(), latent_mask=lat.double(),
                                   eval_mask=ev.double())
    assert l64["loss"].dtype == torch.float64
    (l64["loss"] * torch.ones(B, dtype=torch.float64)).mean().backward()
    l32 = diff.training_losses(model32, inp["x0"], t, model_kwargs=mk, noise=noise, latent_mask=lat, eval_mask=ev)
    (l32["loss"] * torch.ones(B)).mean().backward()
    keys = [n for n, _ in model32.named_parameters()]
    g64 = [sd64[k].grad for k in keys]
    g32 = [p.grad for p in model32.parameters()]
    assert all(g is not None for g in g64)
    gmax = max(float(g.abs().max()) for g in g64)
    rel = max(float((a.double() - b).abs().max()) / (float(b.abs().max()) + 1e-3 * gmax) for a, b in zip(g32, g64))
    ldev = max(float(((l32[k].double() - l64[k]) / l64[k]).detach().abs().max()) for k in ("mse", "eval-mse", "loss"))
    print(f"[train micro] loss {l64['loss'].detach().numpy()}  fp32 reference vs float64: losses rel {ldev:.2e}, "
          f"worst relative gradient deviation {rel:.2e}")
    head = lambda ts_: np.stack([np.resize(x.flatten()[:16].numpy(), 16) for x in ts_])      # noqa: E731
    path = os.path.join(OUT, "xstart_train_micro.npz")
    np.savez_compressed(
        path, keys=np.array(keys), t=t.numpy(), **{k: l64[k].detach().numpy() for k in ("mse", "eval-mse", "loss")},
        grad_norm=np.array([float(g.norm()) for g in g64]), grad_head=head(g64),
        grad_absmax=np.array([float(g.abs().max()) for g in g64]), gmax=np.float64(gmax),
        ref32_dev_loss=np.float64(ldev), ref32_dev_grad=np.float64(rel))
    print("[train] ok", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    todo = sys.argv[1:] or ["update", "traj", "window", "train"]
    for name in todo:
        {"update": gen_update, "traj": gen_traj, "window": gen_window, "train": gen_train}[name]()
