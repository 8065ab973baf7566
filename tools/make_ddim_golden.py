"""Generate tests/golden/ddim_*.npz by IMPORTING the real reference (development machine only, never the GPU machine;
no test imports this file).

    python tools/make_ddim_golden.py [update] [traj] [window] [roundtrip]

TEST INFRASTRUCTURE, as oracle/make_golden.py: nothing of the reference's source is copied.  The reference's own
``GaussianDiffusion`` / ``SpacedDiffusion`` methods (``ddim_sample``, ``ddim_reverse_sample``,
``ddim_sample_loop[_progressive]``, gaussian_diffusion.py:524-685) are driven on float64 tensors on the CPU, with their
table gather kept in float64 (``float64_tables``).  The network
under them is the float64 oracle forward (oracle/unet_oracle.py with the recipe's weights), as in
oracle/make_golden.py::gen_forward_nonsquare: the reference's network casts to float32 internally (nn.py:19, rpe.py:163),
so it cannot produce a float64 truth.  The reference's network in float32 is run next to it from the same inputs and its
per-step deviation from the float64 trajectory is stored with the fixture (``ref32_*``): that is the error one correct fp32
implementation has, which the GPU tests may use as their yardstick.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as mg  # noqa: E402  (puts the reference on sys.path and imports it)
from oracle import recipe, unet_oracle as uo  # noqa: E402

OUT = mg.OUT
PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
ETAS = (0.0, 0.5, 1.0)


def make_diffusion(resp):
    return mg.rsu.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, rescale_timesteps=True,
                                            rescale_learned_sigmas=True, diffusion_space_kwargs=dict(PIXEL))


class patched_randn_like:
    """torch.randn_like returns the given tensors one after the other (the reference draws its noise there)."""

    def __init__(self, tensors):
        self.tensors, self.real = list(tensors), torch.randn_like

    def __enter__(self):
        def fake(x):
            z = self.tensors.pop(0) if len(self.tensors) > 1 else self.tensors[0]
            return z.to(x.dtype)
        torch.randn_like = fake

    def __exit__(self, *a):
        torch.randn_like = self.real


class float64_tables:
    """The reference gathers its float64 tables as float32 (``_extract_into_tensor``, gaussian_diffusion.py:950-963).  On
    float64 tensors that leaves the fp32 rounding of the coefficients in what is meant to be the truth, and DDIM amplifies it
    (1 - alphas_cumprod_prev = 1e-4 at t = 1 loses 3e-4 of its value: up to 4.5e-5 on the sample of the update cases).
    Inside this context the reference's methods gather the same tables WITHOUT the cast; nothing else is changed.  The
    float32 runs (``ref32_dev``) use the reference exactly as it is."""

    def __enter__(self):
        self.real = mg.rgd._extract_into_tensor

        def gather(arr, timesteps, broadcast_shape):
            res = torch.from_numpy(arr)[timesteps]
            while res.dim() < len(broadcast_shape):
                res = res[..., None]
            return res.expand(broadcast_shape)
        mg.rgd._extract_into_tensor = gather

    def __exit__(self, *a):
        mg.rgd._extract_into_tensor = self.real


def folded(diff, eta, reverse):
    """k1, k2, sigma (float64) from the REFERENCE object's own tables: sample = k1 p0 + k2 x + sigma z."""
    abar, r, rm1 = diff.alphas_cumprod, diff.sqrt_recip_alphas_cumprod, diff.sqrt_recipm1_alphas_cumprod
    if reverse:
        to, sigma = diff.alphas_cumprod_next, np.zeros_like(abar)
    else:
        to = diff.alphas_cumprod_prev
        sigma = eta * np.sqrt((1 - to) / (1 - abar)) * np.sqrt(1 - abar / to)
    c = np.sqrt(1 - to - sigma ** 2)
    return np.sqrt(to) - c / rm1, c * r / rm1, sigma


def gen_update():
    """Update-only cases (no network): the reference's ddim_sample / ddim_reverse_sample on a model that returns a given
    eps.  x is built so that x0-hat leaves [-1, 1] in a recorded share of the elements."""
    B, shape = 3, (3, 2, 4, 4, 4)
    n = int(np.prod(shape))
    out = {"shape": np.array(shape, dtype=np.int64), "etas": np.array(ETAS)}
    for tag, resp in (("d1000", ""), ("ddim50", "ddim50")):
        diff = make_diffusion(resp)
        nt = diff.num_timesteps
        out[f"{tag}/num_timesteps"] = np.int64(nt)
        for eta in ETAS:
            k1, k2, sg = folded(diff, eta, False)
            out[f"{tag}/eta{eta}/k1"], out[f"{tag}/eta{eta}/k2"], out[f"{tag}/eta{eta}/sigma"] = k1, k2, sg
        out[f"{tag}/reverse/k1"], out[f"{tag}/reverse/k2"], _ = folded(diff, 0.0, True)
        for name in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "alphas_cumprod_prev", "alphas_cumprod_next"):
            out[f"{tag}/{name}"] = getattr(diff, name)
        for ti, tvec in enumerate(([0, 1, nt // 2], [nt - 1, nt // 3, 1])):
            case = f"{tag}/t{ti}"
            t = torch.tensor(tvec)
            g1, g2 = (recipe.gaussianish(f"ddim/{case}/{k}", n).reshape(shape) for k in ("x0", "d"))
            eps = recipe.gaussianish(f"ddim/{case}/eps", n).reshape(shape).astype(np.float32)
            z = recipe.gaussianish(f"ddim/{case}/z", n).reshape(shape).astype(np.float32)
            ab = diff.alphas_cumprod[tvec].reshape(B, 1, 1, 1, 1)
            # x_t of a clean 0.8-sigma x0 whose noise the "network" misses by 2 %: x0-hat = 0.8 g1 - 0.02 rm1 g2
            x = (np.sqrt(ab) * 0.8 * g1 + np.sqrt(1 - ab) * (eps + 0.02 * g2)).astype(np.float32)
            out[f"{case}/t"], out[f"{case}/x"], out[f"{case}/eps"], out[f"{case}/z"] = t.numpy(), x, eps, z
            x64, eps64, z64 = (torch.from_numpy(a).double() for a in (x, eps, z))
            model = lambda x_, timesteps=None, **kw: (eps64, None)      # noqa: E731
            raw = torch.from_numpy(diff.sqrt_recip_alphas_cumprod[tvec]).view(B, 1, 1, 1, 1) * x64 - \
                torch.from_numpy(diff.sqrt_recipm1_alphas_cumprod[tvec]).view(B, 1, 1, 1, 1) * eps64
            share = float((raw.abs() > 1).double().mean())
            out[f"{case}/clamp_share"] = np.float64(share)
            print(f"[update {case}] t = {tvec}: clamp bites in {100 * share:.1f} % of the elements "
                  f"(per row {[round(float(v), 3) for v in (raw.abs() > 1).double().mean(dim=(1, 2, 3, 4))]})")
            for clip in (0, 1):
                for eta in ETAS:
                    with patched_randn_like([z64]), float64_tables():
                        r = diff.ddim_sample(model, x64, t, clip_denoised=bool(clip), model_kwargs={}, eta=eta)
                    assert r["sample"].dtype == torch.float64
                    out[f"{case}/clip{clip}/eta{eta}/sample"] = r["sample"].numpy()
                    if eta == 0.0:
                        out[f"{case}/clip{clip}/pred_xstart"] = r["pred_xstart"].numpy()
                    # the folded form IS the reference's rule: checked here in float64
                    k1, k2, sg = (torch.from_numpy(v[tvec]).view(B, 1, 1, 1, 1) for v in folded(diff, eta, False))
                    nz = (t != 0).double().view(B, 1, 1, 1, 1)
                    d = float((k1 * r["pred_xstart"] + k2 * x64 + nz * sg * z64 - r["sample"]).abs().max())
                    assert d < 1e-13 * max(1.0, float(r["sample"].abs().max())), (case, clip, eta, d)
                with float64_tables():
                    r = diff.ddim_reverse_sample(model, x64, t, clip_denoised=bool(clip), model_kwargs={}, eta=0.0)
                out[f"{case}/clip{clip}/reverse/sample"] = r["sample"].numpy()
                k1, k2, _ = (torch.from_numpy(v[tvec]).view(B, 1, 1, 1, 1) for v in folded(diff, 0.0, True))
                d = float((k1 * r["pred_xstart"] + k2 * x64 - r["sample"]).abs().max())
                assert d < 1e-13 * max(1.0, float(r["sample"].abs().max())), (case, clip, "reverse", d)
    path = os.path.join(OUT, "ddim_update.npz")
    np.savez_compressed(path, **out)
    print("[update] ok", os.path.getsize(path), "bytes")


class Oracle64:
    """The float64 oracle forward behind the reference's model calling convention."""

    def __init__(self, cfg, sd):
        self.cfg, self.sd = cfg, {k: v.double() for k, v in sd.items()}

    def __call__(self, x, timesteps, return_attn_weights=False, **kw):
        f64 = lambda t: t.double() if t.is_floating_point() else t      # noqa: E731
        out, _ = uo.unet_forward(self.sd, self.cfg, x.double(), f64(kw["x0"]), timesteps.double(), kw["frame_indices"],
                                 f64(kw["obs_mask"]), f64(kw["latent_mask"]))
        assert out.dtype == torch.float64
        return out, None


def cfgB():
    kw, B, T, H, n_pad = mg.CONFIGS["cfgB"]
    cfg = uo.make_cfg(**kw)
    model32, sd = mg.build_reference_model(cfg)
    inp = mg.tt(recipe.make_inputs("cfgB", B, T, cfg["in_channels"], H, H, n_pad=n_pad))
    mk = dict(frame_indices=inp["frame_indices"], obs_mask=inp["obs_mask"], latent_mask=inp["latent_mask"], x0=inp["x0"])
    return cfg, sd, model32, inp, mk


def chain(diff, model, x, mk, eta, noises, n_steps):
    """The reference's ddim_sample_loop_progressive from ``x``; the first n_steps dicts."""
    outs = []
    with patched_randn_like(noises), torch.no_grad():
        for j, o in enumerate(diff.ddim_sample_loop_progressive(model, tuple(x.shape), noise=x, clip_denoised=True,
                                                                model_kwargs=mk, device="cpu", eta=eta)):
            outs.append(o)
            if j + 1 == n_steps:
                break
    return outs


def gen_traj():
    """cfg B on ddim10: all 10 steps at eta = 0 and 4 steps at eta = 1 with recorded per-step noise."""
    cfg, sd, model32, inp, mk = cfgB()
    shape = inp["x"].shape
    diff = make_diffusion("ddim10")
    assert diff.num_timesteps == 10
    m64 = Oracle64(cfg, sd)
    for name, eta, n_steps in (("eta0", 0.0, 10), ("eta1", 1.0, 4)):
        noises = [torch.from_numpy(recipe.gaussianish(f"ddimB/{name}/noise{j}", inp["x"].numel()).reshape(shape).astype(np.float32))
                  for j in range(n_steps)]
        with float64_tables():
            t64 = chain(diff, m64, inp["x"].double(), mk, eta, noises, n_steps)
        t32 = chain(diff, model32, inp["x"].clone(), mk, eta, noises, n_steps)
        body = {}
        for key in ("sample", "pred_xstart"):
            full = torch.stack([o[key] for o in t64])
            assert full.dtype == torch.float64
            for k, v in mg._compact(full, (4, 4)).items():
                body[f"{key}/{k}"] = v
            dev = np.array([float((a[key].double() - b[key]).abs().max()) for a, b in zip(t32, t64)])
            body[f"ref32_dev/{key}"] = dev
            print(f"[traj {name}] {key}: fp32 reference vs float64, per step:", " ".join(f"{v:.2e}" for v in dev))
        body["timestep_map"] = np.array(diff.timestep_map, dtype=np.int64)
        body["eta"] = np.float64(eta)
        path = os.path.join(OUT, f"ddim_traj_cfgB_{name}.npz")
        np.savez_compressed(path, **body)
        print(f"[traj {name}] ok", os.path.getsize(path), "bytes")


def gen_window():
    """One K = 14 window of cfg D (oracle/make_golden.py::gen_sampler_cfgD_window's inputs) on ddim25, final sample only."""
    import json
    kw, _, _, H, _ = mg.CONFIGS["cfgB"]
    cfg = uo.make_cfg(**kw)
    model32, sd = mg.build_reference_model(cfg)
    with open(os.path.join(OUT, "schemes.json")) as f:
        case = next(c for c in json.load(f) if (c["scheme"], c["video_length"], c["n_obs"], c["max_frames"], c["step_size"])
                    == ("hierarchy-2", 1000, 36, 20, 10))
    K = 14
    obs_idx, lat_idx = next(w for w in case["windows"] if len(w[0]) + len(w[1]) == K)
    inp = mg.tt(recipe.make_inputs(f"cfgD_w{K}", 1, K, cfg["in_channels"], H, H))
    fi = torch.tensor([list(obs_idx) + list(lat_idx)], dtype=torch.long)
    obs = torch.zeros(1, K, 1, 1, 1)
    obs[:, :len(obs_idx)] = 1.0
    mk = dict(frame_indices=fi, obs_mask=obs, latent_mask=1 - obs, x0=inp["x0"])
    diff = make_diffusion("ddim25")
    assert diff.num_timesteps == 25
    with torch.no_grad():
        with float64_tables():
            out64 = diff.ddim_sample_loop(Oracle64(cfg, sd), tuple(inp["x"].shape), noise=inp["x"].double(),
                                          clip_denoised=True, model_kwargs=mk, device="cpu", eta=0.0)
        out32 = diff.ddim_sample_loop(model32, tuple(inp["x"].shape), noise=inp["x"].clone(), clip_denoised=True,
                                      model_kwargs=mk, device="cpu", eta=0.0)
    assert out64.dtype == torch.float64
    dev = float((out32.double() - out64).abs().max())
    print(f"[window K={K} ddim25] final sample: fp32 reference vs float64 {dev:.2e}")
    path = os.path.join(OUT, "ddim_window_cfgD.npz")
    np.savez_compressed(path, out=out64.numpy(), frame_indices=fi.numpy(), n_obs=np.int64(len(obs_idx)),
                        ref32_dev=np.float64(dev))
    print("[window] ok", os.path.getsize(path), "bytes")


def gen_roundtrip():
    """cfg B on ddim10: ddim_reverse_sample for t = 0 .. 9 from the clean latent x0, then ddim_sample_loop from the result."""
    cfg, sd, model32, inp, mk = cfgB()
    diff = make_diffusion("ddim10")
    B = inp["x"].shape[0]

    def trip(model, x):
        with torch.no_grad():
            for i in range(diff.num_timesteps):
                x = diff.ddim_reverse_sample(model, x, torch.tensor([i] * B), clip_denoised=True, model_kwargs=mk)["sample"]
            back = diff.ddim_sample_loop(model, tuple(x.shape), noise=x, clip_denoised=True, model_kwargs=mk, device="cpu")
        return x, back
    with float64_tables():
        e64, b64 = trip(Oracle64(cfg, sd), inp["x0"].double())
    e32, b32 = trip(model32, inp["x0"].clone())
    body = {}
    for key, v64, v32 in (("encoded", e64, e32), ("decoded", b64, b32)):
        assert v64.dtype == torch.float64
        for k, v in mg._compact(v64, (2, 2)).items():
            body[f"{key}/{k}"] = v
        body[f"ref32_dev/{key}"] = np.float64((v32.double() - v64).abs().max())
        print(f"[roundtrip] {key}: fp32 reference vs float64 {float(body[f'ref32_dev/{key}']):.2e}; "
              f"|decoded - start| max {float((b64 - inp['x0'].double()).abs().max()):.3f}")
    path = os.path.join(OUT, "ddim_roundtrip_cfgB.npz")
    np.savez_compressed(path, **body)
    print("[roundtrip] ok", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    todo = sys.argv[1:] or ["update", "traj", "window", "roundtrip"]
    for name in todo:
        {"update": gen_update, "traj": gen_traj, "window": gen_window, "roundtrip": gen_roundtrip}[name]()
