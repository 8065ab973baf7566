"""Full ``UNetVideoModel.forward`` on the MI355X vs the golden vectors of the REAL reference and
vs the CPU oracle (same seeded inputs, closed-form parameters).  GPU only.

Stated fp32 tolerance for one forward: |d| <= 1e-4 + 1e-3*|ref| (the reference's
own fp32 CPU result sits 4e-5..1.4e-4 from an fp64 evaluation of the same network).
"""
import os

import numpy as np
import pytest
import torch

from oracle import recipe, unet_oracle as uo
from conftest import GOLDEN
from test_oracle_golden import CONFIGS, NONSQUARE, compare_to_fixture, load_case, load_nonsquare

pytestmark = pytest.mark.gpu


def build_native(cfg, sd):
    from improved_diffusion.unet import UNetVideoModel
    m = UNetVideoModel(in_channels=cfg["in_channels"], model_channels=cfg["model_channels"],
                       out_channels=cfg["out_channels"], num_res_blocks=cfg["num_res_blocks"],
                       attention_resolutions=cfg["attention_resolutions"], dropout=cfg.get("dropout", 0.0), channel_mult=cfg["channel_mult"],
                       num_heads=cfg["num_heads"], use_scale_shift_norm=True, use_rpe_net=True)
    assert [k for k, _ in m.named_parameters()] == list(sd.keys())
    m.load_state_dict(sd)
    return m.cuda().eval()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_vs_reference_golden(name):
    g = np.load(os.path.join(GOLDEN, f"forward_{name}.npz"))
    cfg, sd, inp = load_case(name)
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    with torch.no_grad():
        out, attn = model(d["x"], x0=d["x0"], timesteps=d["t"].float(), frame_indices=d["frame_indices"],
                          obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], return_attn_weights=True)
        out2, none = model(d["x"], x0=d["x0"], timesteps=d["t"].float(), frame_indices=d["frame_indices"],
                           obs_mask=d["obs_mask"], latent_mask=d["latent_mask"])
        out3, _ = model(d["x"], x0=d["x0"], timesteps=d["t"].float(), frame_indices=d["frame_indices"],
                        obs_mask=d["obs_mask"], latent_mask=d["latent_mask"])
    assert none is None
    assert torch.equal(out2, out3), "forward must be deterministic run to run"
    # (the plan that also returns attention maps keeps the two-launch spatial attention: same math, other summation order)
    assert torch.allclose(out, out2, atol=5e-5, rtol=1e-4), float((out - out2).abs().max())
    ref = torch.from_numpy(g["out"])
    err = float((out.cpu() - ref).abs().max())
    print(f"[{name}] max|hip - reference| = {err:.3e} (max|ref| {float(ref.abs().max()):.3f})")
    assert torch.allclose(out.cpu(), ref, atol=1e-4, rtol=1e-3), err          # the contract of SURVEY §8c
    np.testing.assert_allclose(attn["temporal"][0].cpu().numpy()[:8], g["attn_t0"], atol=1e-4)
    np.testing.assert_allclose(attn["spatial"][0].cpu().numpy()[:1, :32, :32], g["attn_s0"], atol=1e-4)
    assert len(attn["temporal"]) == len(attn["spatial"]) and attn["mixed"] == []


@pytest.mark.parametrize("name", list(NONSQUARE))
def test_nonsquare_forward_vs_fp64_fixture(name):
    """``model(x)`` at latents whose levels are not square (16x32, 32x16: down to 2x4 / 4x2; 8x24: 8x24 ... 1x3, no level a
    power of two) and at the reference's defaults for 4x32x32 latents (ch128, two ResBlocks per level, attention at 16x16
    and 8x8) against fp64 fixtures (oracle/make_golden.py::gen_forward_nonsquare), at the contract tolerance."""
    g = np.load(os.path.join(GOLDEN, f"forward_{name}.npz"))
    cfg, sd, inp = load_nonsquare(name)
    assert int(g["n_params"]) == sum(v.numel() for v in sd.values())
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    with torch.no_grad():
        out, _ = model(d["x"], x0=d["x0"], timesteps=d["t"].float(), frame_indices=d["frame_indices"],
                       obs_mask=d["obs_mask"], latent_mask=d["latent_mask"])
    assert out.shape == inp["x"].shape[:2] + (cfg["out_channels"],) + inp["x"].shape[3:]
    err = compare_to_fixture(out, g, atol=1e-4, rtol=1e-3)
    print(f"[{name}] model(x) max|hip - fp64| = {err:.3e} (max|ref| {float(g['absmax']):.3f})")


def test_forward_error_vs_fp64_truth():
    """The HIP result must be as close to an fp64 evaluation as the fp32 CPU oracle is (x3)."""
    name = "cfgB"
    cfg, sd, inp = load_case(name)
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    with torch.no_grad():
        out, _ = model(d["x"], x0=d["x0"], timesteps=d["t"].float(), frame_indices=d["frame_indices"],
                       obs_mask=d["obs_mask"], latent_mask=d["latent_mask"])
        sd64 = {k: v.double() for k, v in sd.items()}
        f64 = lambda t: t.double() if t.is_floating_point() else t
        t64, _ = uo.unet_forward(sd64, cfg, f64(inp["x"]), f64(inp["x0"]), inp["t"].double(), inp["frame_indices"],
                                 f64(inp["obs_mask"]), f64(inp["latent_mask"]))
        o32, _ = uo.unet_forward(sd, cfg, inp["x"], inp["x0"], inp["t"].float(), inp["frame_indices"],
                                 inp["obs_mask"], inp["latent_mask"])
    e_hip = float((out.cpu().double() - t64).abs().max())
    e_cpu = float((o32.double() - t64).abs().max())
    print(f"error vs fp64: hip {e_hip:.3e}  cpu-oracle-fp32 {e_cpu:.3e}")
    assert e_hip < 3 * e_cpu + 2e-5


def test_cpu_input_is_rejected():
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd)
    with pytest.raises(RuntimeError):
        model(inp["x"], x0=inp["x0"], timesteps=inp["t"].float(), frame_indices=inp["frame_indices"],
              obs_mask=inp["obs_mask"], latent_mask=inp["latent_mask"])


def test_full_size_pixel_space_forward_vs_reference():
    """BASELINE.json configs[4] at FULL size: pixel space 128x128x3, 20 frames (3 of them padding), batch 1,
    num_channels=128, num_res_blocks=2, channel_mult (1,1,2,3,4), attention at 16x16 and 8x8 (reference
    scripts/video_train.py:148, unet.py:428-464).  The fixture holds a 4x4-strided subsample of the reference's output
    plus per-(frame, channel) sums and norms of the whole output (oracle/make_golden.py::gen_forward_cfgE_T20)."""
    g = np.load(os.path.join(GOLDEN, "forward_cfgE_T20.npz"))
    kw = CONFIGS["cfgE_T2"][0]
    cfg = uo.make_cfg(**kw)
    sd = {k: torch.from_numpy(v) for k, v in recipe.fill_state_dict(uo.param_shapes(cfg)).items()}
    assert int(g["n_params"]) == sum(v.numel() for v in sd.values())
    inp = {k: torch.from_numpy(v) for k, v in recipe.make_inputs("cfgE_T20", 1, 20, cfg["in_channels"], 128, 128, n_pad=3).items()}
    assert np.array_equal(inp["frame_indices"].numpy(), g["frame_indices"])
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    with torch.no_grad():
        out, _ = model(d["x"], x0=d["x0"], timesteps=d["t"].float(), frame_indices=d["frame_indices"],
                       obs_mask=d["obs_mask"], latent_mask=d["latent_mask"])
    out = out.cpu()
    assert out.shape == (1, 20, 3, 128, 128)
    ref = torch.from_numpy(g["sub"])
    err = float((out[..., ::4, ::4] - ref).abs().max())
    print(f"[cfgE T=20] max|hip - reference| on the subsample = {err:.3e} (max|ref| {float(g['absmax']):.3f})")
    assert torch.allclose(out[..., ::4, ::4], ref, atol=2e-4, rtol=1e-3), err
    # whole-output checks: per-(frame, channel) L2 norms and sums over the 128x128 map
    o64 = out.double()
    np.testing.assert_allclose(o64.pow(2).sum(dim=(-1, -2)).sqrt().numpy(), g["frame_norm"], rtol=2e-5)
    np.testing.assert_allclose(o64.sum(dim=(-1, -2)).numpy(), g["frame_sum"], atol=2e-4 * 128 * 128 ** 0.5 + 1e-3 * np.abs(g["frame_sum"]).max())
