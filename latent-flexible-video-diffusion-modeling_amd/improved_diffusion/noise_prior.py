"""Temporally correlated noise prior for video training and sampling (not in the reference).

"Preserve Your Own Correlation" (PYoCo; Ge et al., ICCV 2023) trains and samples a video diffusion model with noise that
is correlated along time.  Its priors are defined per CONSECUTIVE frame; a window here holds frames at arbitrary, unsorted
and widely spaced video indices, so the prior is defined on the frame indices: for one sample with indices f_0 .. f_{T-1}
(any order, repeats allowed, T <= 64) the noise over frames at a fixed (channel, y, x) is Gaussian with covariance

    K_ij = a + c * rho^|f_i - f_j| + (1 - a - c) * [i == j],      a, c >= 0,  a + c <= 1,  0 <= rho < 1,

independent across (channel, y, x) and across samples.  The diagonal is 1: every frame is marginally N(0, 1), so q_sample's
marginals, every schedule table and every update rule stay valid.  Any subset of the frames has the matching sub-matrix
as its covariance, so two windows that share frames see the same law for them, observed or not.

    spec                meaning
    "mixed:ALPHA"       a = ALPHA^2 / (1 + ALPHA^2), c = 0: one component shared by all frames plus an independent one
    "progressive:ALPHA" a = 0, c = 1, rho = ALPHA / sqrt(1 + ALPHA^2): AR(1) along the frame index - on consecutive indices
                        exactly PYoCo's recursion eps_i = rho eps_{i-1} + sqrt(1 - rho^2) xi_i
    "cov:A:C:RHO"       the general form
    "none", ""          off (a = c = 0 is normalised to it)

The noise is L xi, L the lower Cholesky factor of K and xi i.i.d. N(0, 1).  Repeated indices (``pad_with_random_frames``)
make K singular when a + c = 1: a pivot d_j = K_jj - sum_k L_jk^2 below 1e-12 makes column j of L zero, so a repeated frame
receives the noise of its twin and nothing becomes NaN.

Native: lfvdm_noise_prior_factor (K and the factorisation in fp64, one workgroup per sample) and lfvdm_noise_prior_fill
(L xi over a given xi, or over a Philox draw of its own stream inside the replayed sampler step) - csrc/noise_prior.hip.
The float64 numpy functions here are their definition and the yardstick of the tests.  The effect of a prior on the sample
quality of a trained model has not been measured.
"""
import math

import numpy as np
import torch as th

MAX_FRAMES = 64
PIVOT_MIN = 1e-12
_SUM_SLACK = 1e-12      # a + c may exceed 1 by rounding ("cov:0.7:0.3:..."); the independent part is max(0, 1 - a - c)


def _validated(a, c, rho, what):
    try:
        a, c, rho = float(a), float(c), float(rho)
    except (TypeError, ValueError):
        raise ValueError(f"noise prior {what!r}: a, c and rho must be numbers") from None
    if not (math.isfinite(a) and math.isfinite(c) and math.isfinite(rho)):
        raise ValueError(f"noise prior {what!r}: a, c and rho must be finite")
    if a < 0 or c < 0:
        raise ValueError(f"noise prior {what!r}: a >= 0 and c >= 0, got a = {a!r}, c = {c!r}")
    if a + c > 1.0 + _SUM_SLACK:
        raise ValueError(f"noise prior {what!r}: a + c <= 1, got {a + c!r}")
    if not 0.0 <= rho < 1.0:
        raise ValueError(f"noise prior {what!r}: 0 <= rho < 1, got {rho!r}")
    if a == 0.0 and c == 0.0:
        return None
    return (a, c, rho)


def parse_noise_prior(spec):
    """A spec string (module docstring), an (a, c, rho) triple or None -> (a, c, rho) as floats, or None for "no prior"
    ("none", "", None, a = c = 0).  What LFVDM_NOISE_PRIOR and ``args.noise_prior`` hold.  ValueError otherwise: an unknown
    name, a wrong number of fields, a negative value, a + c > 1, rho outside [0, 1), anything that is not a finite number."""
    if spec is None:
        return None
    if isinstance(spec, (tuple, list)):
        if len(spec) != 3:
            raise ValueError(f"noise prior {spec!r}: a triple (a, c, rho)")
        return _validated(*spec, what=spec)
    if not isinstance(spec, str):
        raise ValueError(f"noise prior must be a string such as 'mixed:1', 'progressive:2' or 'cov:0.2:0.5:0.9', got {spec!r}")
    parts = [s.strip() for s in spec.strip().split(":")]
    kind, vals = parts[0].lower(), parts[1:]
    if kind in ("", "none"):
        if vals:
            raise ValueError(f"noise prior {spec!r}: 'none' takes no value")
        return None
    try:
        vals = [float(v) for v in vals]
    except ValueError:
        raise ValueError(f"noise prior {spec!r}: the values must be numbers") from None
    if kind in ("mixed", "progressive"):
        if len(vals) != 1:
            raise ValueError(f"noise prior {spec!r}: '{kind}:ALPHA'")
        alpha = vals[0]
        if not math.isfinite(alpha) or alpha < 0:
            raise ValueError(f"noise prior {spec!r}: ALPHA is finite and >= 0")
        if kind == "mixed":
            return _validated(alpha * alpha / (1.0 + alpha * alpha), 0.0, 0.0, what=spec)
        return _validated(0.0, 1.0, alpha / math.sqrt(1.0 + alpha * alpha), what=spec)
    if kind == "cov":
        if len(vals) != 3:
            raise ValueError(f"noise prior {spec!r}: 'cov:A:C:RHO'")
        return _validated(*vals, what=spec)
    raise ValueError(f"unknown noise prior {spec!r}: 'none', 'mixed:ALPHA', 'progressive:ALPHA' or 'cov:A:C:RHO'")


def format_noise_prior(prior):
    """(a, c, rho) or None -> the spec string that parses back to exactly it ("cov:..." with round-trip float text, or
    "none"): what is saved with a checkpoint's arguments."""
    prior = parse_noise_prior(prior)
    if prior is None:
        return "none"
    return "cov:" + ":".join(repr(float(v)) for v in prior)


def _indices(frame_indices):
    f = frame_indices.detach().cpu().numpy() if isinstance(frame_indices, th.Tensor) else np.asarray(frame_indices)
    if f.dtype.kind == "f":
        if not np.all(f == np.round(f)):
            raise ValueError("frame indices are whole numbers")
    elif f.dtype.kind not in "iu":
        raise ValueError(f"frame indices are integers, got {f.dtype}")
    f = f.astype(np.int64)
    if f.ndim not in (1, 2) or f.shape[-1] < 1 or f.shape[-1] > MAX_FRAMES:
        raise ValueError(f"frame indices are (T,) or (B, T) with 1 <= T <= {MAX_FRAMES}, got {f.shape}")
    return f


def noise_prior_cov(frame_indices, a, c, rho):
    """K of the module docstring in float64 numpy: (T,) indices -> (T, T), (B, T) -> (B, T, T).  The diagonal is exactly 1."""
    f = _indices(frame_indices)
    gap = np.abs(f[..., :, None] - f[..., None, :]).astype(np.float64)
    with np.errstate(under="ignore"):
        K = float(a) + float(c) * np.power(float(rho), gap)
    T = f.shape[-1]
    K[..., np.arange(T), np.arange(T)] = 1.0
    return K


def _factor(K):
    T = K.shape[0]
    L = np.zeros((T, T), dtype=np.float64)
    for j in range(T):
        s = K[j:, j] - L[j:, :j] @ L[j, :j]
        if s[0] < PIVOT_MIN:      # a frame that is a linear combination of earlier ones: a repeated index under a + c = 1
            continue
        L[j:, j] = s / math.sqrt(s[0])      # the diagonal too is d / sqrt(d): a twin's row then equals its twin's bit for bit
    return L


def noise_prior_factor_ref(frame_indices, a, c, rho):
    """The lower Cholesky factor L of ``noise_prior_cov`` in float64 numpy, column by column with the kernel's pivot rule:
    d_j = K_jj - sum_k L_jk^2 < 1e-12 -> column j is zero.  Same batch shape as ``noise_prior_cov``."""
    K = noise_prior_cov(frame_indices, a, c, rho)
    if K.ndim == 2:
        return _factor(K)
    return np.stack([_factor(k) for k in K])


def apply_noise_prior(xi, frame_indices, prior):
    """i.i.d. N(0, 1) noise ``xi`` (B, T, ...) -> L xi along the frame axis, L the factor of each sample's ``frame_indices``
    (B, T) under ``prior`` (a triple or a spec; None / "none": ``xi`` itself is returned).  A device tensor takes the two
    native launches (fp32, a tensor of its own); a CPU tensor a plain float64 torch product, rounded to ``xi``'s dtype."""
    prior = parse_noise_prior(prior)
    if prior is None:
        return xi
    if frame_indices is None:
        raise ValueError("a noise prior needs the window's frame_indices (B, T)")
    if xi.dim() < 2:
        raise ValueError(f"noise is (B, T, ...), got {tuple(xi.shape)}")
    B, T = xi.shape[0], xi.shape[1]
    if not isinstance(frame_indices, th.Tensor):
        frame_indices = th.as_tensor(np.asarray(frame_indices))
    if frame_indices.numel() != B * T:
        raise ValueError(f"frame_indices holds one index per frame (B, T) = {(B, T)}, got {tuple(frame_indices.shape)}")
    if T > MAX_FRAMES:
        raise ValueError(f"a noise prior covers windows of at most {MAX_FRAMES} frames, got {T}")
    if xi.is_cuda:
        from . import _native as nat
        if xi.dtype != th.float32:
            raise ValueError(f"device noise is float32, got {xi.dtype}")
        fi = frame_indices.to(device=xi.device, dtype=th.int64).reshape(B, T).contiguous()
        L = nat.noise_prior_factor(fi, *prior)
        out = th.empty_like(xi, memory_format=th.contiguous_format)
        nat.noise_prior_fill(L, out, xi=xi.contiguous())
        return out
    L = th.from_numpy(noise_prior_factor_ref(frame_indices.reshape(B, T), *prior))
    flat = xi.reshape(B, T, -1).to(th.float64)
    return th.einsum("bij,bje->bie", L, flat).reshape(xi.shape).to(xi.dtype)
