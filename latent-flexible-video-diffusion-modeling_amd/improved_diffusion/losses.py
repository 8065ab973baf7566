"""Likelihood helpers of the variational bound: the module surface of the reference's ``losses.py`` (same three public
names and signatures), written here in the formulation of the HIP kernel (csrc/vb_terms.hip) as plain elementwise torch.

The hot path does not pass through here: ``GaussianDiffusion._vb_terms_bpd`` evaluates the KL and the decoder term in one
launch.  These functions serve ``_prior_bpd`` (one call per bits-per-dim loop) and are what the tests evaluate in float64
next to the kernel.

Formulation.  The normal CDF is the tanh approximation Phi(z) ~ 0.5 (1 + tanh w(z)), w = sqrt(2/pi) (z + 0.044715 z^3),
which equals sigmoid(2 w).  Logarithms of bin probabilities are therefore sums of log-sigmoids, with no 1 + tanh
cancellation in the tails; every probability is floored at 1e-12 before its logarithm, i.e. every log at log(1e-12).
"""
import math

import torch as th
import torch.nn.functional as F

_LOG_FLOOR = math.log(1e-12)
_HALF_BIN = 1.0 / 255.0


def _logit_of_cdf(z):
    """a(z) with Phi(z) ~ sigmoid(a(z))"""
    return 2.0 * math.sqrt(2.0 / math.pi) * (z + 0.044715 * z * z * z)


def normal_kl(mean1, logvar1, mean2, logvar2):
    """KL(N(mean1, exp(logvar1)) || N(mean2, exp(logvar2))) elementwise, with broadcasting.  Any argument may be a Python
    number as long as one of the four is a tensor, which fixes dtype and device."""
    like = None
    for arg in (mean1, logvar1, mean2, logvar2):
        if th.is_tensor(arg):
            like = arg
            break
    if like is None:
        raise TypeError("normal_kl needs a tensor among its arguments")
    m1, lv1, m2, lv2 = (a if th.is_tensor(a) else th.as_tensor(a, dtype=like.dtype, device=like.device)
                        for a in (mean1, logvar1, mean2, logvar2))
    gap = lv2 - lv1
    # 0.5 (gap - 1 + exp(-gap)) is second order in the gap: expm1 keeps it exact when the two variances are close
    return 0.5 * (gap + th.expm1(-gap) + th.exp(-lv2) * th.square(m1 - m2))


def approx_standard_normal_cdf(x):
    """The tanh approximation of the standard normal CDF, in its sigmoid form."""
    return th.sigmoid(_logit_of_cdf(x))


def discretized_gaussian_log_likelihood(x, *, means, log_scales):
    """Log-probability that N(means, exp(log_scales)^2) puts on the bin of half-width 1/255 around ``x`` (data scaled to
    [-1, 1]).  The lowest bin (x < -0.999) reaches down to -inf and the highest (x > 0.999) up to +inf."""
    if not (x.shape == means.shape == log_scales.shape):
        raise ValueError(f"shapes differ: {tuple(x.shape)}, {tuple(means.shape)}, {tuple(log_scales.shape)}")
    z = (x - means) * th.exp(-log_scales)
    half = _HALF_BIN * th.exp(-log_scales)
    hi, lo = _logit_of_cdf(z + half), _logit_of_cdf(z - half)      # hi > lo: the map is increasing
    log_below_hi = F.logsigmoid(hi)        # log Phi(upper edge)
    log_above_lo = F.logsigmoid(-lo)       # log (1 - Phi(lower edge))
    # Phi(hi) - Phi(lo) = sigmoid(hi) sigmoid(-lo) (1 - exp(lo - hi))
    log_inside = log_below_hi + log_above_lo + th.log(-th.expm1(lo - hi))
    picked = th.where(x < -0.999, log_below_hi, th.where(x > 0.999, log_above_lo, log_inside))
    return picked.clamp(min=_LOG_FLOOR)
