"""Haar wavelet diffusion space (``diffusion_space="wavelet"``): a compressed space that needs no weights and inverts exactly.

    wavelet_encode(video, levels=1, norm="range", stats=None)                     pixels -> coefficients
    wavelet_decode(coef, levels=1, norm="range", stats=None, out_dtype=float32)   coefficients -> pixels
    channel_stats(videos, levels=1, norm="range")                                 {"mean", "std"} per coefficient channel
    space_args(image_size, channels=3, levels=1)                                  what a training / sampling script needs

``L = levels`` is 1 or 2; H and W must be multiples of ``2^L``.  One level maps the 2 x 2 block ``[[a, b], [c, d]]`` (rows,
then columns) of every channel to four bands, in this order:

    ll = s (a + b + c + d)      lh = s (a - b + c - d)   difference along the width
    hl = s (a + b - c - d)      difference along the height      hh = s (a - b - c + d)

``norm="range"``: s = 1/4, pixels in [-1, 1] give coefficients in [-1, 1] in every band, so ``clip_denoised=True`` stays a
valid bound in this space.  ``norm="orthonormal"``: s = 1/2, an isometry (white noise stays white).  The inverse is the same
butterfly times 1 / (4 s).

Layout.  L = 1: (N, 4C, H/2, W/2), channel blocks [ll | lh | hl | hh] of C channels.  L = 2: (N, 16C, H/4, W/4): the level
is applied again to ll, and the three level-1 detail bands come to quarter resolution by space-to-depth with phases (0,0),
(0,1), (1,0), (1,1): [ll2 | lh2 | hl2 | hh2 | lh1 x 4 phases | hl1 x 4 phases | hh1 x 4 phases].

``stats = {"mean", "std"}`` (4^L C entries each, from ``channel_stats``) standardises every coefficient channel: encode ends
with ``(y - mean) / std``, decode undoes it first.  With stats attached the coefficients are no longer confined to [-1, 1]:
``clip_denoised=True`` is then NOT a valid bound and must be switched off.

Device tensors (float32 in [-1, 1] or uint8 0..255) go through csrc/wavelet.hip: one read of the pixels, one write of the
coefficients.  CPU tensors take ``_encode_torch`` / ``_decode_torch``, the same definition in plain torch (float32, or
float64 when given float64).  ``out_dtype=torch.uint8`` gives ``clamp(round((x + 1) * 127.5), 0, 255)``: it ROUNDS to nearest,
where ``TrainLoop``'s ``.to(uint8)`` truncates; rounding is what makes uint8 -> encode -> decode the identity.
"""
import torch

NORMS = {"range": 0.25, "orthonormal": 0.5}


def _check(levels, norm):
    if levels not in (1, 2):
        raise ValueError(f"wavelet_levels must be 1 or 2, got {levels!r}")
    if norm not in NORMS:
        raise ValueError(f"wavelet_norm must be one of {sorted(NORMS)}, got {norm!r}")


def _frames(x, levels, coef):
    """(B, T, C, H, W) or (N, C, H, W) -> (N, C, H, W) contiguous, the lead shape, the PIXEL (C, H, W)."""
    if not torch.is_tensor(x) or x.dim() not in (4, 5):
        raise ValueError("expected a tensor of (B, T, C, H, W) or (N, C, H, W)")
    lead = tuple(x.shape[:-3])
    C, H, W = x.shape[-3:]
    m = 1 << levels
    if coef:
        if C % (m * m):
            raise ValueError(f"coefficients of shape {tuple(x.shape)}: {C} channels are not a multiple of {m * m} "
                             f"(wavelet_levels={levels})")
        C, H, W = C // (m * m), H * m, W * m
    elif H % m or W % m:
        raise ValueError(f"frames of shape {tuple(x.shape)}: H = {H} and W = {W} must be divisible by {m} "
                         f"(wavelet_levels={levels})")
    if x.numel() == 0:
        raise ValueError(f"empty input {tuple(x.shape)}")
    return x.reshape((-1,) + tuple(x.shape[-3:])).contiguous(), lead, (C, H, W)


def _stats(stats, channels, device, dtype):
    """-> (mean, std) as (channels,) tensors, or (None, None)."""
    if stats is None:
        return None, None
    out = []
    for k in ("mean", "std"):
        v = torch.as_tensor(stats[k]).detach().reshape(-1).to(device=device, dtype=dtype)
        if v.numel() != channels:
            raise ValueError(f"wavelet_stats[{k!r}] has {v.numel()} entries, the coefficients have {channels} channels")
        out.append(v)
    if not bool((out[1] > 0).all()):
        raise ValueError("wavelet_stats['std'] must be positive")
    return out


def _level(x, s):
    """(N, C, H, W) -> ll, lh, hl, hh (N, C, H/2, W/2)"""
    a, b, c, d = x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]
    p, q, r, t = a + b, c + d, a - b, c - d
    return s * (p + q), s * (r + t), s * (p - q), s * (r - t)


def _unlevel(ll, lh, hl, hh, k):
    p, q, r, t = ll + lh, ll - lh, hl + hh, hl - hh
    out = ll.new_empty(ll.shape[:-2] + (2 * ll.shape[-2], 2 * ll.shape[-1]))
    out[..., 0::2, 0::2] = k * (p + r)
    out[..., 0::2, 1::2] = k * (q + t)
    out[..., 1::2, 0::2] = k * (p - r)
    out[..., 1::2, 1::2] = k * (q - t)
    return out


def _phases(x):
    return [x[..., i::2, j::2] for i in (0, 1) for j in (0, 1)]


def _encode_torch(x, levels, norm):
    """The definition in plain torch ops on any device, without the standardisation: (N, C, H, W) -> (N, 4^L C, ...)."""
    s = NORMS[norm]
    ll, lh, hl, hh = _level(x, s)
    if levels == 1:
        return torch.cat([ll, lh, hl, hh], dim=1)
    return torch.cat(list(_level(ll, s)) + _phases(lh) + _phases(hl) + _phases(hh), dim=1)


def _decode_torch(y, levels, norm):
    k = 0.25 / NORMS[norm]
    C = y.shape[1] >> (2 * levels)
    blk = list(y.split(C, dim=1))
    if levels == 1:
        return _unlevel(*blk, k)
    detail = []
    for band in range(3):
        d = y.new_empty(y.shape[0], C, 2 * y.shape[2], 2 * y.shape[3])
        for ph, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            d[..., i::2, j::2] = blk[4 + 4 * band + ph]
        detail.append(d)
    return _unlevel(_unlevel(*blk[:4], k), *detail, k)


def _to_unit(x):
    """CPU pixels -> float in [-1, 1]: floats as they are; uint8 0..255 with the kernel's bits, fma(float32(1 / 127.5), v, -1):
    the product and the sum are exact in float64, so the cast back is the one rounding of the fused operation."""
    if x.dtype == torch.uint8:
        scale = torch.tensor(1.0 / 127.5, dtype=torch.float32).double()
        return (x.double() * scale - 1.0).to(torch.float32)
    return x if x.dtype == torch.float64 else x.to(torch.float32)


def _rstd(std):
    """1 / std as the kernel receives it: rounded once to float32 from the float64 quotient."""
    return (1.0 / std.double()).to(torch.float32)


def wavelet_encode(video, levels=1, norm="range", stats=None):
    """Pixels (B, T, C, H, W) or (N, C, H, W) - float in [-1, 1], or uint8 0..255 (read as ``v / 127.5 - 1``) - ->
    coefficients with ``4^levels C`` channels at ``H / 2^levels x W / 2^levels``, float32 (float64 for float64 CPU input).
    ``ValueError`` naming the shape when H or W is not divisible by ``2^levels``."""
    _check(levels, norm)
    x, lead, (C, H, W) = _frames(video, levels, coef=False)
    m = 1 << levels
    K = m * m * C
    if x.is_cuda:
        from . import _native as nat
        if x.dtype != torch.uint8:
            x = x.to(torch.float32)
        mean, std = _stats(stats, K, x.device, torch.float32)
        with torch.cuda.device(x.device):
            y = torch.empty(x.shape[0], K, H // m, W // m, device=x.device, dtype=torch.float32)
            nat.wavelet_encode(x, y, levels, norm, mean, None if std is None else _rstd(std))
    else:
        x = _to_unit(x)
        y = _encode_torch(x, levels, norm)
        mean, std = _stats(stats, K, x.device, x.dtype)
        if mean is not None and x.dtype == torch.float64:
            y = (y - mean.view(1, -1, 1, 1)) / std.view(1, -1, 1, 1)
        elif mean is not None:      # float32: the kernel's operations, so host and device batch preparation agree bitwise
            y = (y - mean.view(1, -1, 1, 1)) * _rstd(std).view(1, -1, 1, 1)
    return y.reshape(lead + tuple(y.shape[1:]))


def wavelet_decode(coef, levels=1, norm="range", stats=None, out_dtype=torch.float32):
    """The inverse of ``wavelet_encode`` (same ``levels``, ``norm``, ``stats``): coefficients -> pixels (.., C, H, W) in
    [-1, 1] as float32 (float64 CPU input stays float64), or with ``out_dtype=torch.uint8`` as
    ``clamp(round((x + 1) * 127.5), 0, 255)`` - rounded to nearest, not truncated."""
    _check(levels, norm)
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"out_dtype must be torch.float32 or torch.uint8, got {out_dtype}")
    y, lead, (C, H, W) = _frames(coef, levels, coef=True)
    if y.is_cuda:
        from . import _native as nat
        y = y.to(torch.float32)
        mean, std = _stats(stats, y.shape[1], y.device, torch.float32)
        with torch.cuda.device(y.device):
            x = torch.empty(y.shape[0], C, H, W, device=y.device, dtype=out_dtype)
            nat.wavelet_decode(y, x, levels, norm, mean, std)
    else:
        if y.dtype != torch.float64:
            y = y.to(torch.float32)
        mean, std = _stats(stats, y.shape[1], y.device, y.dtype)
        if mean is not None:
            y = y * std.view(1, -1, 1, 1) + mean.view(1, -1, 1, 1)
        x = _decode_torch(y, levels, norm)
        if out_dtype == torch.uint8:
            x = ((x + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8)
    return x.reshape(lead + (C, H, W))


def channel_stats(videos, levels=1, norm="range"):
    """Mean and standard deviation of every coefficient channel over ``videos`` (pixels, any leading shape), in float64
    plain torch: the ``wavelet_stats`` of ``diffusion_space_kwargs``.  A channel that is constant over the data gets std 1."""
    _check(levels, norm)
    x, _, _ = _frames(videos, levels, coef=False)
    y = _encode_torch(_to_unit(x.cpu()).double(), levels, norm)
    mean = y.mean(dim=(0, 2, 3))
    std = y.var(dim=(0, 2, 3), unbiased=False).sqrt()
    return {"mean": mean, "std": torch.where(std > 0, std, torch.ones_like(std))}


def space_args(image_size, channels=3, levels=1, norm="range", stats=None):
    """The settings of a wavelet-space run for PIXEL frames of ``image_size`` (an int, or (H, W)) with ``channels`` channels:
    ``{"image_size", "in_channels", "diffusion_space_kwargs"}`` - the model sees ``4^levels channels`` channels at
    ``image_size / 2^levels`` (the reference scripts' per-space dictionaries have no "wavelet" key)."""
    _check(levels, norm)
    m = 1 << levels
    sizes = (image_size,) if isinstance(image_size, int) else tuple(image_size)
    if any(int(v) <= 0 or int(v) % m for v in sizes):
        raise ValueError(f"image_size {image_size!r} must be divisible by {m} (wavelet_levels={levels})")
    small = tuple(int(v) // m for v in sizes)
    kw = {"diffusion_space": "wavelet", "pre_encoded": False, "pre_encoded_stats_dict": None, "wavelet_levels": levels,
          "wavelet_norm": norm, "wavelet_stats": stats}
    return {"image_size": small[0] if isinstance(image_size, int) else small, "in_channels": m * m * int(channels),
            "diffusion_space_kwargs": kw}
