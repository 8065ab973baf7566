"""Haar wavelet diffusion space without a GPU: the plain torch path of improved_diffusion/wavelet.py against an independent
float64 evaluation written here straight from the definition (``yardstick``: per-block arithmetic on strided views, the
two-level layout built from two one-level calls plus explicit space-to-depth), its range / isometry / inverse properties, the
standardisation round trip, the refusals, ``space_args``, the encode / decode / can_decode boundary of GaussianDiffusion, the
new exports in the header and the binding, and TrainLoop's device batch preparation gate.

The GPU tests (test_wavelet_gpu.py) import ``yardstick``, ``make_pixels`` and ``make_stats`` from here."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

S = {"range": 0.25, "orthonormal": 0.5}
SHAPES = [(1, 1, 2, 2, 1), (3, 3, 6, 10, 1), (2, 3, 8, 16, 1), (2, 3, 8, 12, 2), (2, 4, 16, 32, 2)]      # (N, C, H, W, L)


def _one_level(x, s):
    """(N, C, H, W) float64 -> [ll, lh, hl, hh], each (N, C, H/2, W/2): the four sums of the definition, term by term."""
    a, b = x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2]
    c, d = x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]
    return [s * (a + b + c + d), s * (a - b + c - d), s * (a + b - c - d), s * (a - b - c + d)]


def _space_to_depth(x):
    return [x[:, :, i::2, j::2] for (i, j) in ((0, 0), (0, 1), (1, 0), (1, 1))]


def yardstick(x, levels, norm, stats=None):
    """float64 pixels in [-1, 1] -> (coefficients after the optional standardisation, coefficients before it)."""
    assert x.dtype == torch.float64
    ll, lh, hl, hh = _one_level(x, S[norm])
    if levels == 1:
        raw = torch.cat([ll, lh, hl, hh], dim=1)
    else:
        raw = torch.cat(_one_level(ll, S[norm]) + _space_to_depth(lh) + _space_to_depth(hl) + _space_to_depth(hh), dim=1)
    if stats is None:
        return raw, raw
    return (raw - stats["mean"].double().view(1, -1, 1, 1)) / stats["std"].double().view(1, -1, 1, 1), raw


def make_pixels(shape, dtype, seed=0):
    """Seeded pixels of (N, C, H, W): float32 uniform in [-1, 1] with the extremes planted, or uint8 over all of 0..255."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(1000 + seed + N * 7 + C * 11 + H * 13 + W * 17)
    if dtype == torch.uint8:
        x = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
        x.view(-1)[0], x.view(-1)[-1] = 255, 0
        return x
    x = torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1
    x.view(-1)[0], x.view(-1)[-1] = 1.0, -1.0
    return x


def make_stats(channels):
    """Per-channel mean in [-0.5, 0.5] and std in [0.25, 2].  The affine multiplies the transform's own error by 1 / std <= 4.
    Before it that error is at most 2 L 2^-24 max|x| (per level: two half-ulps of sums of two values and one of the sum of
    four, times s), so the bound's 8 L 2^-24 M, M >= max|x| / 4 by Parseval, still holds after it for data whose largest
    coefficient is of the order of its largest pixel, as the seeded cases here are."""
    k = torch.arange(channels, dtype=torch.float64)
    return {"mean": 0.5 * torch.sin(1.0 + 2.0 * k), "std": 0.25 + 1.75 * (0.5 + 0.5 * torch.cos(0.7 * k))}


def to_unit64(x):
    """The float64 value of a pixel as the kernels read it: float32 as it is, uint8 through the float32 scale 1 / 127.5."""
    if x.dtype == torch.uint8:
        return x.double() * float(np.float32(1.0 / 127.5)) - 1.0
    return x.double()


# ---------------------------------------------------------------------------------------------------- the torch path
@pytest.mark.parametrize("norm", ["range", "orthonormal"])
@pytest.mark.parametrize("with_stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.uint8], ids=["f32", "f64", "u8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_torch_path_matches_the_float64_definition(shape, dtype, with_stats, norm):
    from improved_diffusion.wavelet import wavelet_encode
    N, C, H, W, L = shape
    x = make_pixels((N, C, H, W), torch.float32 if dtype == torch.float64 else dtype)
    if dtype == torch.float64:
        x = x.double()
    stats = make_stats(C * 4 ** L) if with_stats else None
    want, raw = yardstick(to_unit64(x), L, norm, stats)
    got = wavelet_encode(x, L, norm, stats)
    assert got.shape == (N, C * 4 ** L, H >> L, W >> L)
    assert got.dtype == (torch.float64 if dtype == torch.float64 else torch.float32)
    M = float(raw.abs().max())
    eps = 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24
    bound = 8 * L * eps * M + (2 * eps * want.abs() if with_stats else 0.0)
    err = (got.double() - want).abs()
    print(f"[wavelet torch {shape} {dtype} {norm} stats={with_stats}] max err {float(err.max()):.2e}, "
          f"worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    # (B, T, C, H, W) is the same transform frame by frame
    if N % 2 == 0:
        assert torch.equal(wavelet_encode(x.view(N // 2, 2, C, H, W), L, norm, stats), got.view((N // 2, 2) + got.shape[1:]))


def test_two_level_layout_block_by_block():
    """The channel order of L = 2, spelled out on a frame whose value names its position."""
    from improved_diffusion.wavelet import wavelet_encode
    C, H, W = 2, 8, 8
    x = torch.arange(C * H * W, dtype=torch.float64).view(1, C, H, W) / (C * H * W)
    y = wavelet_encode(x, 2, "range")
    one = wavelet_encode(x, 1, "range")
    ll1, lh1, hl1, hh1 = one.split(C, dim=1)
    assert torch.equal(y[:, :4 * C], wavelet_encode(ll1, 1, "range"))
    for band, d in enumerate((lh1, hl1, hh1)):
        for ph, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            k = 4 + 4 * band + ph
            assert torch.equal(y[:, k * C:(k + 1) * C], d[:, :, i::2, j::2]), (band, ph)


@pytest.mark.parametrize("levels", [1, 2])
def test_range_norm_keeps_the_unit_interval(levels):
    from improved_diffusion.wavelet import wavelet_encode
    g = torch.Generator().manual_seed(3)
    x = torch.where(torch.rand(4, 3, 8, 8, generator=g) < 0.5, -1.0, 1.0)      # the corners of the cube: the extremes
    x[0] = 1.0
    x[1, :, ::2] = -1.0      # rows alternate: |hl| = 1
    y = wavelet_encode(x, levels, "range")
    assert float(y.abs().max()) == 1.0
    y = wavelet_encode(make_pixels((4, 3, 8, 8), torch.float32), levels, "range")
    assert float(y.abs().max()) <= 1.0


@pytest.mark.parametrize("levels", [1, 2])
def test_orthonormal_norm_preserves_the_squared_norm(levels):
    from improved_diffusion.wavelet import wavelet_encode
    x = make_pixels((3, 3, 8, 12), torch.float32).double()
    y = wavelet_encode(x, levels, "orthonormal")
    a, b = x.pow(2).sum(dim=(1, 2, 3)), y.pow(2).sum(dim=(1, 2, 3))
    assert torch.allclose(a, b, rtol=1e-13, atol=0)
    assert not torch.allclose(a, wavelet_encode(x, levels, "range").pow(2).sum(dim=(1, 2, 3)), rtol=1e-2)


@pytest.mark.parametrize("norm", ["range", "orthonormal"])
@pytest.mark.parametrize("with_stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_decode_inverts_encode(shape, with_stats, norm):
    from improved_diffusion.wavelet import wavelet_decode, wavelet_encode
    N, C, H, W, L = shape
    stats = make_stats(C * 4 ** L) if with_stats else None
    x = make_pixels((N, C, H, W), torch.float32)
    back = wavelet_decode(wavelet_encode(x.double(), L, norm, stats), L, norm, stats)
    assert back.dtype == torch.float64 and back.shape == x.shape
    assert float((back - x.double()).abs().max()) <= 64 * 2.0 ** -53 * (4 if with_stats else 1)
    back32 = wavelet_decode(wavelet_encode(x, L, norm, stats), L, norm, stats)
    assert back32.dtype == torch.float32
    assert float((back32 - x).abs().max()) <= 64 * 2.0 ** -24 * (4 if with_stats else 1)
    # uint8 frames come back exactly: the uint8 output rounds to nearest
    u = make_pixels((N, C, H, W), torch.uint8)
    assert torch.equal(wavelet_decode(wavelet_encode(u, L, norm, stats), L, norm, stats, out_dtype=torch.uint8), u)
    assert wavelet_decode(wavelet_encode(u.view(1, N, C, H, W), L, norm), L, norm).shape == (1, N, C, H, W)


def test_uint8_output_rounds_where_a_cast_truncates():
    from improved_diffusion.wavelet import wavelet_decode, wavelet_encode
    x = torch.full((1, 1, 2, 2), 200.6 / 127.5 - 1.0, dtype=torch.float64)
    out = wavelet_decode(wavelet_encode(x, 1, "range"), 1, "range", out_dtype=torch.uint8)
    assert out.dtype == torch.uint8 and int(out[0, 0, 0, 0]) == 201
    assert int(((x + 1) * 127.5).clamp(0, 255).to(torch.uint8)[0, 0, 0, 0]) == 200
    big = wavelet_decode(torch.tensor([3.0, 0, 0, 0, -3.0, 0, 0, 0]).view(2, 4, 1, 1), 1, "range", out_dtype=torch.uint8)
    assert int(big[0].max()) == 255 and int(big[1].min()) == 0


def test_channel_stats_standardise_the_data():
    from improved_diffusion.wavelet import channel_stats, wavelet_decode, wavelet_encode
    g = torch.Generator().manual_seed(5)
    vids = (torch.rand(2, 5, 3, 8, 8, generator=g) * 1.2 - 0.4).clamp(-1, 1)
    for L in (1, 2):
        st = channel_stats(vids, L, "range")
        assert st["mean"].dtype == torch.float64 and st["mean"].shape == st["std"].shape == (3 * 4 ** L,)
        y = wavelet_encode(vids.double(), L, "range", st)
        assert float(y.mean(dim=(0, 1, 3, 4)).abs().max()) < 1e-12
        assert float((y.var(dim=(0, 1, 3, 4), unbiased=False) - 1).abs().max()) < 1e-12
        assert float((wavelet_decode(y, L, "range", st) - vids.double()).abs().max()) < 1e-13
        # the same numbers from uint8 frames of the same content
        u8 = ((vids + 1) * 127.5).round().to(torch.uint8)
        st8 = channel_stats(u8, L, "range")
        assert float((st8["mean"] - st["mean"]).abs().max()) < 1e-2
    flat = channel_stats(torch.zeros(1, 3, 4, 4), 1, "range")
    assert bool((flat["std"] == 1).all())


def test_refusals_name_the_shape():
    from improved_diffusion.wavelet import space_args, wavelet_decode, wavelet_encode
    with pytest.raises(ValueError, match=r"\(1, 3, 6, 7\)"):
        wavelet_encode(torch.zeros(1, 3, 6, 7), 1)
    with pytest.raises(ValueError, match=r"\(2, 2, 3, 6, 8\)"):
        wavelet_encode(torch.zeros(2, 2, 3, 6, 8), 2)      # 6 is even but no multiple of 4
    with pytest.raises(ValueError, match=r"\(1, 6, 4, 4\)"):
        wavelet_decode(torch.zeros(1, 6, 4, 4), 1)
    with pytest.raises(ValueError):
        wavelet_encode(torch.zeros(1, 3, 8, 8), 3)
    with pytest.raises(ValueError):
        wavelet_encode(torch.zeros(1, 3, 8, 8), 1, "sqrt")
    with pytest.raises(ValueError):
        wavelet_encode(torch.zeros(1, 3, 8, 8), 1, "range", {"mean": torch.zeros(3), "std": torch.ones(3)})
    with pytest.raises(ValueError):
        wavelet_decode(torch.zeros(1, 4, 4, 4), 1, out_dtype=torch.float16)
    with pytest.raises(ValueError):
        space_args(130, levels=2)


def test_space_args():
    from improved_diffusion.wavelet import space_args
    a = space_args(128)
    assert a["image_size"] == 64 and a["in_channels"] == 12
    kw = a["diffusion_space_kwargs"]
    assert kw["diffusion_space"] == "wavelet" and kw["wavelet_levels"] == 1 and kw["wavelet_norm"] == "range"
    assert kw["pre_encoded"] is False and kw["wavelet_stats"] is None
    b = space_args((64, 96), channels=1, levels=2)
    assert b["image_size"] == (16, 24) and b["in_channels"] == 16 and b["diffusion_space_kwargs"]["wavelet_levels"] == 2


# ---------------------------------------------------------------------------------------------------- the diffusion boundary
def _diffusion(**kw):
    from improved_diffusion import script_util as su
    from improved_diffusion.wavelet import space_args
    return su.create_gaussian_diffusion(steps=50, rescale_timesteps=True, rescale_learned_sigmas=True,
                                        diffusion_space_kwargs=space_args(16, **kw)["diffusion_space_kwargs"])


def test_setup_enc_dec_accepts_the_wavelet_space():
    """Fails on the parent commit, where setup_enc_dec raises NotImplementedError for "wavelet"."""
    d = _diffusion()
    assert d.diffusion_space == "wavelet" and d.wavelet_levels == 1 and d.wavelet_norm == "range" and d.wavelet_stats is None
    assert d.vae is None
    from improved_diffusion import script_util as su
    d2 = su.create_gaussian_diffusion(steps=50, diffusion_space_kwargs={"diffusion_space": "wavelet"})
    assert d2.wavelet_levels == 1 and d2.wavelet_norm == "range"
    with pytest.raises(ValueError):
        su.create_gaussian_diffusion(steps=50, diffusion_space_kwargs={"diffusion_space": "wavelet", "wavelet_levels": 3})


@pytest.mark.parametrize("levels", [1, 2])
def test_diffusion_encode_decode_can_decode(levels):
    from improved_diffusion.wavelet import channel_stats, wavelet_decode, wavelet_encode
    vid = make_pixels((4, 3, 16, 16), torch.float32).view(2, 2, 3, 16, 16)
    d = _diffusion(levels=levels)
    assert d.can_decode() is True
    z = d.encode(vid, chunk_size=1)
    assert z.shape == (2, 2, 3 * 4 ** levels, 16 >> levels, 16 >> levels)
    assert torch.equal(z, wavelet_encode(vid, levels, "range"))
    back = d.decode(z, chunk_size=1)
    assert back.shape == vid.shape and torch.equal(back, wavelet_decode(z, levels, "range"))
    assert float((back - vid).abs().max()) <= 16 * 2.0 ** -24
    d._refuse_undecodable("p_sample_loop", True)      # nothing to refuse: the space decodes
    st = channel_stats(vid, levels, "orthonormal")
    ds = _diffusion(levels=levels, norm="orthonormal", stats=st)
    zs = ds.encode(vid)
    assert torch.equal(zs, wavelet_encode(vid, levels, "orthonormal", st))
    assert float((ds.decode(zs) - vid).abs().max()) <= 64 * 2.0 ** -24


def test_other_spaces_are_untouched():
    from improved_diffusion import script_util as su
    vid = torch.zeros(1, 2, 3, 8, 8)
    for space in (None, "pixel"):
        d = su.create_gaussian_diffusion(steps=50, diffusion_space_kwargs={"diffusion_space": space})
        assert d.encode(vid) is vid and d.decode(vid) is vid and d.can_decode()
    d = su.create_gaussian_diffusion(steps=50, diffusion_space_kwargs={"diffusion_space": "latent"})
    assert not d.can_decode()
    with pytest.raises(NotImplementedError):
        d.encode(vid)
    with pytest.raises(ValueError):
        su.create_gaussian_diffusion(steps=50, diffusion_space_kwargs={"diffusion_space": "fourier"})


# ---------------------------------------------------------------------------------------------------- exports and the gate
def test_exports_in_header_and_binding():
    from improved_diffusion import _native as nat
    with open(os.path.join(ROOT, "include", "lfvdm_hip.h")) as f:
        header = f.read()
    for name in ("lfvdm_wavelet_encode", "lfvdm_wavelet_decode", "lfvdm_prepare_batch_wavelet"):
        assert name in nat._SIGS and name in nat.EXPORTS
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(nat._SIGS[name][0]), name      # one ctypes entry per C parameter
    assert "#define LFVDM_WAVELET_RANGE 0" in header and "#define LFVDM_WAVELET_ORTHONORMAL 1" in header
    assert nat.WAVELET_NORMS == {"range": 0, "orthonormal": 1}
    assert os.path.exists(os.path.join(ROOT, "latent-flexible-video-diffusion-modeling_amd", "csrc", "wavelet.hip"))


def test_device_prep_gate_accepts_the_wavelet_space(monkeypatch):
    from improved_diffusion import dist_util
    from improved_diffusion.train_util import TrainLoop
    monkeypatch.setattr(dist_util, "dev", lambda: torch.device("cuda:0"))
    monkeypatch.delenv("LFVDM_DEVICE_BATCH_PREP", raising=False)
    loop = object.__new__(TrainLoop)
    loop.pad_with_random_frames = True
    loop.diffusion = _diffusion()
    f32, u8 = torch.zeros(2, 4, 3, 16, 16), torch.zeros(2, 4, 3, 16, 16, dtype=torch.uint8)
    assert loop._device_prep_ok(f32) and loop._device_prep_ok(u8)
    assert not loop._device_prep_ok(torch.zeros(2, 4, 3, 16, 18, dtype=torch.float64))
    assert not loop._device_prep_ok(torch.zeros(2, 4, 3, 15, 16))      # the host path raises the ValueError with the shape
    loop.diffusion = _diffusion(levels=2)
    assert loop._device_prep_ok(f32) and not loop._device_prep_ok(torch.zeros(2, 4, 3, 16, 18))
    monkeypatch.setenv("LFVDM_DEVICE_BATCH_PREP", "0")
    assert not loop._device_prep_ok(f32)
    monkeypatch.delenv("LFVDM_DEVICE_BATCH_PREP")
    # the other spaces as before: float32 only
    from improved_diffusion import script_util as su
    loop.diffusion = su.create_gaussian_diffusion(steps=50, diffusion_space_kwargs={"diffusion_space": "pixel"})
    assert loop._device_prep_ok(f32) and not loop._device_prep_ok(u8)
    loop.diffusion = su.create_gaussian_diffusion(steps=50, diffusion_space_kwargs={"diffusion_space": "latent"})
    assert not loop._device_prep_ok(f32)
