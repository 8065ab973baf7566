"""Op-level parity at ill-conditioned inputs: GroupNorm statistics of activations far off centre (|mean| / std of 64 and
1280) and softmax cores with logits past the float32 exp range.  GPU only; the input builders, the fp64 references and the
two CPU float32 models that set each bound live here as well and are exercised without a GPU by test_conditioning_cpu.

GroupNorm.  Reference: torch group_norm in fp64 (fp64 autograd for the backward) on the float32 input values.  Per case two
float32 models of the statistics are evaluated on the CPU: ``model_two_pass`` (mean by strictly sequential addition, then
the squared deviations, sequentially: the most pessimistic order a correct kernel could use) and ``model_one_pass``
(E[x^2] - mean^2 with numpy's pairwise sums: the most favourable order a one-pass kernel could use).  A kernel may miss
fp64 by at most 4 x the two-pass model's error + the absolute tolerance of the entry's existing test; the factor 4 covers
another legitimate summation order and v_rcp / v_sqrt rounding.  Regime "b" (mean 64, std 0.05) separates the two models
by more than 10 x the bound at every shape here (asserted on the CPU); regime "a" (mean 64, std 1) is held to the same
kind of bound, which its one-pass error (2e-3 to 4e-3) misses by 1.7 x to 55 x only.

Softmax.  q and k are scaled by s = 3 (logit std about 9) and s = 6 (std about 36, largest logits past 88 where expf
overflows without the max subtraction).  Reference: the fp64 core; model: the same core in torch float32 on the CPU; bound
4 x the model's error + the existing test's tolerance.  Every comparison prints kernel error, model error and bound."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import rnd, cl, from_cl, packed, _temporal_core_f64
from test_norm_backward_gpu import _gnt_target, GNT_SHAPES, _gnt_columns, _gnt_rows, _gn_reference, SMALL_SLICE_CASES, _p_of, _pl

pytestmark = pytest.mark.gpu

EPS = 1e-5
REGIMES = {"a": (64.0, 1.0), "b": (64.0, 0.05)}


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from improved_diffusion import _native
    _native.lib()
    return _native


# ------------------------------------------------------------------------------------------------------------------------
# 1. shared inputs, models and bounds (CPU only)
# ------------------------------------------------------------------------------------------------------------------------
def offcentre(tag, shape, mean, std, gw=0):
    """rnd(tag, *shape) * std + mean in float32.  gw > 0: the mean alternates sign per group of gw channels (last axis), so
    that a kernel sharing one shift across groups shows as well."""
    x = rnd(tag, *shape) * std
    if gw:
        sign = 1.0 - 2.0 * ((torch.arange(shape[-1]) // gw) % 2).float()
        return x + mean * sign
    return x + mean


def _seq_sum(a):
    """Strictly sequential float32 addition along axis 1 (numpy's accumulate does not reassociate)."""
    return np.cumsum(a, axis=1, dtype=np.float32)[:, -1]


def model_two_pass(xg):
    """float32 (mean, variance) of every row of xg: sequential sum, then sequential sum of squared deviations."""
    a = xg.numpy()
    n = np.float32(a.shape[1])
    mean = _seq_sum(a) / n
    d = a - mean[:, None]
    return torch.from_numpy(mean), torch.from_numpy(_seq_sum(d * d) / n)


def model_one_pass(xg):
    """float32 (mean, variance) as E[x^2] - mean^2, both sums pairwise (numpy)."""
    a = xg.numpy()
    n = np.float32(a.shape[1])
    mean = a.sum(1, dtype=np.float32) / n
    ex2 = (a * a).sum(1, dtype=np.float32) / n
    return torch.from_numpy(mean), torch.from_numpy(np.maximum(ex2 - mean * mean, np.float32(0)))


def model_no_between(xg, P, chunk=64):
    """float32 (mean, variance) of rows laid out [P][gw] whose chunks of ``chunk`` positions are merged WITHOUT the
    between-chunk term of Chan's formula (variance = weighted mean of the chunk variances): what a broken merge gives."""
    a = xg.double().view(xg.shape[0], P, -1)
    parts = [a[:, i:i + chunk].reshape(a.shape[0], -1) for i in range(0, P, chunk)]
    w = torch.tensor([p.shape[1] for p in parts], dtype=torch.float64)
    var = sum(wi * p.var(1, unbiased=False) for wi, p in zip(w, parts)) / w.sum()
    return a.reshape(a.shape[0], -1).mean(1).float(), var.float()


def _rstd32(var):
    return (1.0 / torch.sqrt(var + torch.tensor(EPS, dtype=torch.float32))).float()


def gn_budget(xg, finish, ref, floor, extra=(), x64=None):
    """xg: float32 [groups][elements], one row per GroupNorm group; finish(xhat fp64, same shape) -> the entry's output in
    fp64; ref: that output from torch's fp64 group_norm.  x64: the fp64 rows where the kernel computes the statistics input
    itself (a GEMM's accumulators): the models then see that value rounded to float32 (xg), the reference the fp64 value, and
    the difference (half an ulp of 64) is part of the two-pass error.  Returns the model errors, the bound and the stats."""
    x64 = xg.double() if x64 is None else x64
    m64 = x64.mean(1)
    r64 = (x64.var(1, unbiased=False) + EPS).rsqrt()
    self_check = float((finish((x64 - m64[:, None]) * r64[:, None]) - ref).abs().max())
    assert self_check < 1e-9, f"the model's restatement disagrees with torch's fp64 group_norm: {self_check:.3e}"
    out = {"mean64": m64, "rstd64": r64, "floor": floor}
    for name, model in (("two", model_two_pass), ("one", model_one_pass)) + tuple(extra):
        m, v = model(xg)
        r = _rstd32(v)
        xh = (xg - m[:, None]) * r[:, None]
        out[name] = float((finish(xh.double()) - ref).abs().max())
        out["mean_" + name] = float((m.double() - m64).abs().max())
        out["rstd_" + name] = float((r.double() / r64 - 1).abs().max())
    out["bound"] = 4 * out["two"] + floor
    return out


def held(tag, got, want, bound, model=None):
    err = float((got.detach().double().cpu() - want.double()).abs().max())
    print(f"[cond] {tag}: kernel {err:.3e}" + (f", two-pass model {model:.3e}" if model is not None else "") + f", bound {bound:.3e}")
    assert bool(torch.isfinite(got).all()), f"{tag}: not finite"
    assert err <= bound, f"{tag}: max|d| = {err:.3e} > {bound:.3e}"
    return err


def to_groups(x, N, P, Cc, gw=None):
    """[N*P][C] rows -> [N * C/gw][P * gw]: one row per (sample, group)."""
    gw = gw or Cc // 32
    return x.reshape(N, P, Cc // gw, gw).permute(0, 2, 1, 3).reshape(N * (Cc // gw), P * gw).contiguous()


def from_groups(xh, N, P, Cc, gw=None):
    gw = gw or Cc // 32
    return xh.reshape(N, Cc // gw, P, gw).permute(0, 2, 1, 3).reshape(N * P, Cc)


def t_to_groups(x, B, T, P, Cc):
    """temporal rows (b, t, pixel) x C -> one row per (b, pixel, group) over (T, C/32)."""
    gw = Cc // 32
    return x.reshape(B, T, P, 32, gw).permute(0, 2, 3, 1, 4).reshape(B * P * 32, T * gw).contiguous()


def t_from_groups(xh, B, T, P, Cc):
    gw = Cc // 32
    return xh.reshape(B, P, 32, T, gw).permute(0, 3, 1, 2, 4).reshape(B * T * P, Cc)


def _affine_post(y, N, P, Cc, fm, T, act):
    """rows [N*P][C] after the GroupNorm affine -> act(y * (1 + scale) + shift) in fp64."""
    if fm is not None:
        f = fm.double().repeat_interleave(T, dim=0)[:, None, :]
        y = (y.view(N, P, Cc) * (1 + f[..., :Cc]) + f[..., Cc:]).reshape(N * P, Cc)
    return F.silu(y) if act else y


def _affine(xhat_rows, N, P, Cc, gamma, beta, fm, T, act):
    """rows [N*P][C] of normalised values -> act((xhat * gamma + beta) * (1 + scale) + shift) in fp64."""
    return _affine_post(xhat_rows * gamma.double() + beta.double(), N, P, Cc, fm, T, act)


def _gn_rows_f64(x, N, P, Cc, gamma, beta, fm, T, act, groups=32):
    """torch fp64 group_norm of [N*P][C] rows (+ FiLM, + SiLU), as test_gn_apply states it."""
    ref = F.group_norm(x.double().view(N, P, Cc).permute(0, 2, 1), groups, gamma.double(), beta.double(), eps=EPS)
    ref = ref.permute(0, 2, 1).reshape(N * P, Cc)
    return _affine_post(ref, N, P, Cc, fm, T, act)


# ------------------------------------------------------------------------------------------------------------------------
# 2. GroupNorm sites: case lists and CPU builders (every builder is cached: one reference per case)
# ------------------------------------------------------------------------------------------------------------------------
def _with_regimes(shapes):
    return [s + (r,) for s in shapes for r in ("a", "b")]


# (N, P, C0, C1, film, act, regime)
GN_APPLY_CASES = _with_regimes([(4, 16, 128, 0, False, 1), (3, 4, 256, 128, False, 1), (2, 37, 512, 0, True, 0)])
# (N, P, C0, C1, film, act, drift, regime): drift = the mean runs linearly from 32 to 96 over the pixels
GN_WS_CASES = [s[:6] + (False, s[6]) for s in _with_regimes([(4, 1061, 64, 0, False, 1), (2, 2500, 96, 32, True, 1)])] + \
              [(4, 1061, 64, 0, False, 1, True, "b")]
GN_COEF_CASES = _with_regimes([(3, 4, 256, 128, True, 0)])


@functools.lru_cache(maxsize=None)
def build_gn_rows(site, N, P, C0, C1, film, act, drift, regime, floor):
    """Inputs, fp64 reference and budget of a spatial GroupNorm over the virtual concat [N*P][C0 + C1]."""
    mean, std = REGIMES[regime]
    Cc, T = C0 + C1, (2 if N % 2 == 0 else 1)
    gw = Cc // 32
    tag = f"cond/{site}/{N}/{P}/{C0}/{C1}/{regime}"
    if drift:
        ramp = torch.linspace(32.0, 96.0, P).repeat(N)[:, None]
        a = rnd(tag + "/a", N * P, C0) * std + ramp
    else:
        a = offcentre(tag + "/a", (N * P, C0), mean, std, gw=gw)
    # the second source sits at another mean than the first (C0 is a multiple of the group width: no group straddles)
    b = offcentre(tag + "/b", (N * P, C1), -0.5 * mean, std) if C1 else None
    gamma, beta = 1 + 0.1 * rnd(tag + "/g", Cc), 0.1 * rnd(tag + "/be", Cc)
    fm = 0.3 * rnd(tag + "/film", N // T, 2 * Cc) if film else None
    x = torch.cat([a] + ([b] if C1 else []), dim=1)
    ref = _gn_rows_f64(x, N, P, Cc, gamma, beta, fm, T, act)
    finish = lambda xh: _affine(from_groups(xh, N, P, Cc), N, P, Cc, gamma, beta, fm, T, act)      # noqa: E731
    extra = (("no_between", lambda g_: model_no_between(g_, P)),) if drift else ()
    bud = gn_budget(to_groups(x, N, P, Cc), finish, ref, floor, extra)
    return dict(a=a, b=b, x=x, gamma=gamma, beta=beta, fm=fm, T=T, ref=ref, bud=bud, Cc=Cc)


def gn_apply_case(N, P, C0, C1, film, act, regime):
    return build_gn_rows("apply", N, P, C0, C1, film, act, False, regime, 3e-5)        # test_gn_apply: atol 3e-5


def gn_ws_case(N, P, C0, C1, film, act, drift, regime):
    return build_gn_rows("ws", N, P, C0, C1, film, act, drift, regime, 3e-5)           # test_gn_apply_large_maps: 3e-5


def gn_coef_case(N, P, C0, C1, film, act, regime):
    return build_gn_rows("coef", N, P, C0, C1, film, act, False, regime, 5e-5)         # test_gn_apply's coefficient map: 5e-5


def large_maps_inputs_one_pass_error(N, P, C0, C1, film, act):
    """The one-pass model on the inputs of test_gn_apply_large_maps (same tags, same * 1.3 + 0.7)."""
    Cc, T = C0 + C1, 2
    a = rnd("gl/a", N * P, C0) * 1.3 + 0.7
    b = rnd("gl/b", N * P, C1) if C1 else None
    gamma, beta = 1 + 0.1 * rnd("gl/g", Cc), 0.1 * rnd("gl/be", Cc)
    fm = 0.3 * rnd("gl/film", N // T, 2 * Cc) if film else None
    x = torch.cat([a] + ([b] if C1 else []), dim=1)
    ref = _gn_rows_f64(x, N, P, Cc, gamma, beta, fm, T, act)
    finish = lambda xh: _affine(from_groups(xh, N, P, Cc), N, P, Cc, gamma, beta, fm, T, act)      # noqa: E731
    return gn_budget(to_groups(x, N, P, Cc), finish, ref, 3e-5)


LARGE_MAPS_CASES = [(2, 2500, 96, 32, True, 1), (4, 1061, 64, 0, False, 1), (2, 4096, 128, 64, True, 1), (3, 16384, 128, 0, False, 1),
                    (2, 300, 512, 256, False, 0), (4, 256, 64, 0, False, 1)]


def _one_per_kernel():
    seen, out = set(), []
    for s in GNT_SHAPES:
        k = _gnt_target(s[1], s[3])
        if k not in seen:
            seen.add(k)
            out.append(s)
    return out


GNT_CASES = _with_regimes(_one_per_kernel())                       # (B, T, P, C, regime): one shape per kernel
GNT_QKV_CASES = _with_regimes([(2, 7, 6, 64), (3, 5, 1, 128)])
PROJ_GN_CASES = _with_regimes([(5, 64, 64), (3, 64, 256)])       # (N, C, P, regime): frames of 64 and of 256 positions


@functools.lru_cache(maxsize=None)
def gnt_case(B, T, P, Cc, regime, floor=1e-5):
    """Temporal GroupNorm over (C/32, T) per (b, pixel): test_gn_temporal_forward's reference and tolerance (1e-5)."""
    mean, std = REGIMES[regime]
    tag = f"cond/gnt/{B}/{T}/{P}/{Cc}/{regime}"
    x = offcentre(tag + "/x", (B * T * P, Cc), mean, std, gw=Cc // 32)
    gamma, beta = 1 + 0.1 * rnd(tag + "/g", Cc), 0.1 * rnd(tag + "/b", Cc)
    ref = _gnt_rows(F.group_norm(_gnt_columns(x, B, T, P, Cc), 32, gamma.double(), beta.double(), EPS), B, T, P, Cc)
    finish = lambda xh: t_from_groups(xh, B, T, P, Cc) * gamma.double() + beta.double()      # noqa: E731
    bud = gn_budget(t_to_groups(x, B, T, P, Cc), finish, ref, floor)
    return dict(x=x, gamma=gamma, beta=beta, ref=ref, bud=bud)


@functools.lru_cache(maxsize=None)
def gnt_qkv_case(B, T, P, Cc, regime):
    """lfvdm_gn_temporal_qkv: the normalised rows (1e-5) and qkv = fp64 GEMM of the fp64 normalisation (2e-5)."""
    c = dict(gnt_case(B, T, P, Cc, regime))
    tag = f"cond/gntq/{B}/{T}/{P}/{Cc}"
    W, bias = rnd(tag + "/w", 3 * Cc, Cc) * (Cc ** -0.5), rnd(tag + "/bias", 3 * Cc) * 0.1
    proj = lambda y: y @ W.double().t() + bias.double()      # noqa: E731
    c["W"], c["bias"], c["ref_q"] = W, bias, proj(c["ref"])
    finish = lambda xh: proj(t_from_groups(xh, B, T, P, Cc) * c["gamma"].double() + c["beta"].double())      # noqa: E731
    c["bud_q"] = gn_budget(t_to_groups(c["x"], B, T, P, Cc), finish, c["ref_q"], 2e-5)
    return c


@functools.lru_cache(maxsize=None)
def proj_gn_case(N, Cc, P, regime):
    """lfvdm_proj_gn: GroupNorm32 of (o W^T + bias + res); the offset sits on the residual, so the statistics see it after
    bias + residual.  test_projection_with_the_next_groupnorm_inside's reference and tolerance (2e-5)."""
    mean, std = REGIMES[regime]
    M = N * P
    tag = f"cond/pg/{N}/{Cc}/{P}/{regime}"
    # the projection's own spread (o W^T: about 0.8 std) would drown regime b: scale it with the regime
    o = rnd(tag + "/o", M, Cc) * 0.8 * std
    res = offcentre(tag + "/res", (M, Cc), mean, 0.6 * std, gw=Cc // 32)
    W, bias = rnd(tag + "/w", Cc, Cc) * (Cc ** -0.5), rnd(tag + "/bias", Cc) * 0.1 * std
    gamma, beta = rnd(tag + "/g", Cc) * 0.3 + 1.0, rnd(tag + "/b", Cc) * 0.2
    y64 = o.double() @ W.double().t() + bias.double() + res.double()
    ref = F.group_norm(y64.view(N, P, Cc).permute(0, 2, 1), 32, gamma.double(), beta.double(), EPS).permute(0, 2, 1).reshape(M, Cc)
    return dict(o=o, res=res, W=W, bias=bias, gamma=gamma, beta=beta, y64=y64, ref=ref,
                bud=computed_budget(y64, N, P, Cc, Cc // 32, lambda r: r * gamma.double() + beta.double(), ref, 2e-5))


def computed_budget(y64, N, P, Cc, gw, post, ref, floor):
    """gn_budget of a GroupNorm over rows [N*P][C] that the kernel computes itself (fp64 value y64, groups of gw channels)."""
    return gn_budget(to_groups(y64.float(), N, P, Cc, gw), lambda xh: post(from_groups(xh, N, P, Cc, gw)), ref, floor,
                     x64=to_groups(y64, N, P, Cc, gw))


# Fused output GroupNorm of lfvdm_conv_igemm: (N, Cin, Cout, H, regime), FiLM + skip_raw.  The offset is the conv bias (64),
# the weights are scaled so that the conv output has a std of about 1 (a) / 0.05 (b).
CONV_GN_CASES = _with_regimes([(6, 64, 128, 8), (8, 128, 128, 4)])
CONCAT_GN_CASES = _with_regimes([(6, 64, 64, 64, 4)])              # (N, Cin, C0, C1, H, regime)


@functools.lru_cache(maxsize=None)
def conv_gn_case(N, Cin, Cout, H, regime):
    mean, std = REGIMES[regime]
    T, P = 2, H * H
    tag = f"cond/cgn/{N}/{Cin}/{Cout}/{H}/{regime}"
    x = rnd(tag + "/x", N, Cin, H, H)
    w = rnd(tag + "/w", Cout, Cin, 3, 3, scale=std / (9 * Cin) ** 0.5)
    sign = 1.0 - 2.0 * ((torch.arange(Cout) // (Cout // 32)) % 2).float()
    b = mean * sign + std * rnd(tag + "/b", Cout)
    gamma, beta = 1 + 0.1 * rnd(tag + "/g", Cout), 0.1 * rnd(tag + "/be", Cout)
    fm = 0.3 * rnd(tag + "/film", N // T, 2 * Cout)
    raw = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ref = F.group_norm(raw, 32, gamma.double(), beta.double(), eps=EPS)
    f = fm.double().repeat_interleave(T, dim=0)
    ref = F.silu(ref * (1 + f[:, :Cout, None, None]) + f[:, Cout:, None, None])
    ref_rows = ref.permute(0, 2, 3, 1).reshape(N * P, Cout)
    rows = raw.permute(0, 2, 3, 1).reshape(N * P, Cout)
    post = lambda r: _affine(r, N, P, Cout, gamma, beta, fm, T, 1)      # noqa: E731
    bud = computed_budget(rows, N, P, Cout, Cout // 32, post, ref_rows, 1e-4)      # the existing test: err < 1e-4
    return dict(x=x, w=w, b=b, gamma=gamma, beta=beta, fm=fm, T=T, ref=ref.float(), bud=bud, raw_std=float(raw.std()))


@functools.lru_cache(maxsize=None)
def concat_gn_case(N, Cin, C0, C1, H, regime):
    """GroupNorm32 + SiLU over concat(conv3x3(x), skip) half by half; the halves sit at different means."""
    mean, std = REGIMES[regime]
    P, Cc = H * H, C0 + C1
    gw = Cc // 32
    tag = f"cond/cat/{N}/{Cin}/{C0}/{C1}/{H}/{regime}"
    x = rnd(tag + "/x", N, Cin, H, H)
    w = rnd(tag + "/w", C0, Cin, 3, 3, scale=std / (9 * Cin) ** 0.5)
    b = mean + std * rnd(tag + "/b", C0)
    skip = offcentre(tag + "/skip", (N, H, H, C1), -0.5 * mean, std).permute(0, 3, 1, 2).contiguous()
    gamma, beta = 1 + 0.1 * rnd(tag + "/g", Cc), 0.1 * rnd(tag + "/be", Cc)
    h = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    cat = torch.cat([h, skip.double()], 1)
    ref = F.silu(F.group_norm(cat, 32, gamma.double(), beta.double(), eps=EPS))
    rows = cat.permute(0, 2, 3, 1).reshape(N * P, Cc)
    post = lambda r: F.silu(r * gamma.double() + beta.double())      # noqa: E731
    bud = computed_budget(rows, N, P, Cc, gw, post, ref.permute(0, 2, 3, 1).reshape(N * P, Cc), 1e-4)
    return dict(x=x, w=w, b=b, skip=skip, gamma=gamma, beta=beta, ref=ref.float(), h=h, bud=bud)


# ---- backward ----------------------------------------------------------------------------------------------------------
def _pick_small_slices():
    """One case of SMALL_SLICE_CASES per channel split: the one with the most elements per group among the classes below the
    chunked boundary (t, t + 1 and 256 are left to the workspace shape: the CPU models walk every group sequentially)."""
    best = {}
    for c in SMALL_SLICE_CASES:
        C0, C1, cls, N, T, act, film, adds = c.values
        if cls in ("t+1", "t", "256"):
            continue
        P = _p_of(cls, C0 + C1, 16 * _pl(C0 + C1))
        if (C0, C1) not in best or P > best[(C0, C1)][0]:
            best[(C0, C1)] = (P, (C0, C1, cls, N, T, act, film))
    return [v[1] for v in best.values()]


GN_BWD_SMALL_CASES = _with_regimes(_pick_small_slices())
GN_BWD_WS_CASES = [(4, 1061, 64, 0, False, 1, "a"), (4, 1061, 64, 0, False, 1, "b")]
GNT_BWD_CASES = _with_regimes([(2, 20, 16, 128), (2, 64, 3, 96)])


def _bwd_model(xg, stats, head, dy_rows, to_rows, to_g):
    """fp64 GroupNorm backward formula on given (mean, rstd) per group: head(xhat_rows, gamma, beta) -> output rows."""
    m, r = stats
    xh = ((xg.double() - m.double()[:, None]) * r.double()[:, None])
    xr = to_rows(xh).detach().requires_grad_(True)
    gamma, beta = head.gamma.double().detach().requires_grad_(True), head.beta.double().detach().requires_grad_(True)
    (head(xr, gamma, beta) * dy_rows.double()).sum().backward()
    g = to_g(xr.grad)
    dx = r.double()[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return to_rows(dx), gamma.grad, beta.grad


class _Head:
    def __init__(self, N, P, Cc, gamma, beta, fm, T, act):
        self.N, self.P, self.Cc, self.gamma, self.beta, self.fm, self.T, self.act = N, P, Cc, gamma, beta, fm, T, act

    def __call__(self, xr, gamma, beta):
        return _affine_post(xr * gamma + beta, self.N, self.P, self.Cc, self.fm, self.T, self.act)


def bwd_budget(xg, head, dy_rows, to_rows, to_g, refs, floors):
    """Budgets for (dx, dgamma, dbeta): the float32 two-pass / one-pass forward statistics, then the fp64 backward formula."""
    x64 = xg.double()
    exact = (x64.mean(1), (x64.var(1, unbiased=False) + EPS).rsqrt())
    chk = _bwd_model(xg, exact, head, dy_rows, to_rows, to_g)
    for got, want in zip(chk, refs):
        assert float((got - want).abs().max()) <= 1e-9 * (1 + float(want.abs().max())), "backward restatement != fp64 autograd"
    out = {}
    for name, model in (("two", model_two_pass), ("one", model_one_pass)):
        m, v = model(xg)
        got = _bwd_model(xg, (m, _rstd32(v)), head, dy_rows, to_rows, to_g)
        out[name] = [float((g_ - w_).abs().max()) for g_, w_ in zip(got, refs)]
    out["bound"] = [4 * t + f_ for t, f_ in zip(out["two"], floors)]
    out["floor"] = floors
    return out


@functools.lru_cache(maxsize=None)
def gn_bwd_case(C0, C1, N, P, T, act, film, regime):
    mean, std = REGIMES[regime]
    Cc = C0 + C1
    tag = f"cond/gb/{C0}/{C1}/{N}/{P}/{regime}"
    a = offcentre(tag + "/a", (N * P, C0), mean, std, gw=Cc // 32)
    b = offcentre(tag + "/b", (N * P, C1), -0.5 * mean, std) if C1 else None
    gamma, beta = 1 + 0.1 * rnd(tag + "/g", Cc), 0.1 * rnd(tag + "/be", Cc)
    fm = 0.3 * rnd(tag + "/film", N // T, 2 * Cc) if film else None
    da = rnd(tag + "/da", N * P, Cc)
    dx, dg, db, _ = _gn_reference(a, b, C0, C1, N, P, gamma, beta, fm, T, act, da)
    # the existing tests' tolerances: 3e-5 max(|dx|, 1); 2e-4 |dgamma|max; 2e-4 |dbeta|max
    floors = [3e-5 * max(float(dx.abs().max()), 1.0), 2e-4 * float(dg.abs().max()), 2e-4 * float(db.abs().max())]
    x = torch.cat([a] + ([b] if C1 else []), dim=1)
    head = _Head(N, P, Cc, gamma, beta, fm, T, act)
    bud = bwd_budget(to_groups(x, N, P, Cc), head, da, lambda xh: from_groups(xh, N, P, Cc), lambda r: to_groups(r, N, P, Cc),
                     (dx, dg, db), floors)
    return dict(a=a, b=b, gamma=gamma, beta=beta, fm=fm, da=da, refs=(dx, dg, db), bud=bud)


@functools.lru_cache(maxsize=None)
def gnt_bwd_case(B, T, P, Cc, regime):
    mean, std = REGIMES[regime]
    tag = f"cond/gtb/{B}/{T}/{P}/{Cc}/{regime}"
    x = offcentre(tag + "/x", (B * T * P, Cc), mean, std, gw=Cc // 32)
    dy = rnd(tag + "/dy", B * T * P, Cc)
    gamma = 1 + 0.1 * rnd(tag + "/g", Cc)
    xr = _gnt_columns(x, B, T, P, Cc).requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), torch.zeros(Cc, dtype=torch.float64, requires_grad=True)
    F.group_norm(xr, 32, gr, br, eps=EPS).backward(_gnt_columns(dy, B, T, P, Cc))
    refs = (_gnt_rows(xr.grad, B, T, P, Cc), gr.grad, br.grad)
    # test_gn_temporal_backward_every_kernel: dx 5e-5; dgamma / dbeta 1e-4 max(1, |.|max)
    floors = [5e-5, 1e-4 * max(1.0, float(gr.grad.abs().max())), 1e-4 * max(1.0, float(br.grad.abs().max()))]
    head = _Head(B * T, P, Cc, gamma, torch.zeros(Cc), None, 1, 0)
    bud = bwd_budget(t_to_groups(x, B, T, P, Cc), head, dy, lambda xh: t_from_groups(xh, B, T, P, Cc),
                     lambda r: t_to_groups(r, B, T, P, Cc), refs, floors)
    return dict(x=x, dy=dy, gamma=gamma, refs=refs, bud=bud)


# ------------------------------------------------------------------------------------------------------------------------
# 3. softmax cores: case lists and CPU builders
# ------------------------------------------------------------------------------------------------------------------------
SCALES = (3.0, 6.0)
# (N, P, C, heads, constructed): constructed = every query's largest logit lies in the last key block of 64, the first
# block's maximum at least 40 below it
ATTN_SPATIAL_CASES = [(1, 70, 96, 4, False), (2, 100, 64, 2, False), (1, 33, 448, 4, False), (1, 70, 96, 4, True)]
ATTN_FUSED_CASES = [(2, 36, 64, 4), (1, 9, 128, 2)]
# (B, T, P, C, heads): one shape per kernel the dispatch can pick (temporal_kernels below restates the dispatch)
ATTN_TEMPORAL_CASES = [(2, 5, 4, 128, 4),          # second generation, head dim 32
                       (1, 20, 33, 64, 4),         # second generation, head dim 16
                       (1, 40, 5, 64, 4),          # long window (33..64 frames), forward and backward
                       (1, 20, 7, 384, 4),         # head dim 96: first generation <16> forward, first-generation backward rows
                       (2, 4, 16, 32, 4),          # head dim 8: first generation <8> forward and backward
                       (2, 5, 256, 128, 4)]        # B P F = 16384 at head dim 32: first generation <32> (whole head in a chunk)
MASK_SHAPES = [(2, 7, 5, 64, 4), (2, 7, 5, 32, 4)]      # second generation (head dim 16) and first generation (head dim 8)


def temporal_kernels(B, T, P, Cc, heads):
    """(forward kernel, backward rows kernel) that lfvdm_attn_temporal / _bwd pick for a shape: attention.hip
    lfvdm_attn_temporal_ring, attention_temporal2.hip lfvdm_attn_temporal2_try / _bwd_rows_try, attention_bwd.hip."""
    Fh = Cc // heads
    if T > 32:
        return "long", "long"
    bwd = "gen2" if Fh in (16, 32, 64) else ("gen1<16>" if Fh % 16 == 0 and T <= 24 else "gen1<8>")
    if B * P * Fh < 16384 and Fh in (16, 32, 64):
        return "gen2", bwd
    if Fh == 32 and T <= 24:
        return "gen1<32>", bwd
    if Fh % 16 == 0 and T <= 24:
        return "gen1<16>", bwd
    assert Fh % 8 == 0
    return "gen1<8>", bwd
KEY_BLOCK = 64          # keys staged per block by attention.hip (32 at padded head dim 128: 64 is a multiple)


def _spatial_core(qkv, N, P, Cc, heads):
    """Softmax attention of [N*P][3C] rows ([3][heads][F] channels), as test_attn_spatial_backward states it; any dtype."""
    Fh = Cc // heads
    q, k, v = (qkv.view(N, P, 3, heads, Fh)[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    logits = (q * Fh ** -0.5) @ k.transpose(-1, -2)
    attn = torch.softmax(logits, -1)
    o = (attn @ v).permute(0, 2, 1, 3).reshape(N * P, Cc)
    return o, attn, torch.logsumexp(logits, -1).reshape(N * heads, P), logits


def _spatial_all(qkv, d_o, N, P, Cc, heads, dtype):
    x = qkv.to(dtype).clone().requires_grad_(True)
    o, attn, lse, logits = _spatial_core(x, N, P, Cc, heads)
    (o * d_o.to(dtype)).sum().backward()
    return dict(o=o.detach(), attn=attn.detach(), lse=lse.detach(), dqkv=x.grad, logits=logits.detach())


@functools.lru_cache(maxsize=None)
def attn_spatial_case(N, P, Cc, heads, constructed, s):
    tag = f"cond/as/{N}/{P}/{Cc}/{heads}/{int(constructed)}"
    qkv = rnd(tag + "/qkv", N * P, 3 * Cc)
    Fh = Cc // heads
    v5 = qkv.view(N, P, 3, heads, Fh)
    if constructed:
        # keys of the last block share a direction u per head with the queries; keys of the first block oppose it
        u = rnd(tag + "/u", heads, Fh)
        u = u / u.norm(dim=-1, keepdim=True) * Fh ** 0.5
        v5[:, :, 0] = 0.3 * v5[:, :, 0] + u
        last = (P - 1) // KEY_BLOCK * KEY_BLOCK
        v5[:, :, 1] = 0.3 * v5[:, :, 1]
        v5[:, last:, 1] += u
        v5[:, :KEY_BLOCK, 1] -= u
    v5[:, :, 0] *= s
    v5[:, :, 1] *= s
    d_o = rnd(tag + "/do", N * P, Cc)
    ref = _spatial_all(qkv, d_o, N, P, Cc, heads, torch.float64)
    mod = _spatial_all(qkv, d_o, N, P, Cc, heads, torch.float32)
    g = ref["dqkv"]
    # the existing tests' absolute tolerances: o 2e-5, attn 1e-5, lse 2e-5; dqkv 2e-5 (1 + |g|max) + 3e-5
    floors = dict(o=2e-5, attn=1e-5, lse=2e-5, dqkv=2e-5 * (1.0 + float(g.abs().max())) + 3e-5)
    model = {k: float((mod[k].double() - ref[k]).abs().max()) for k in floors}
    bound = {k: 4 * model[k] + floors[k] for k in floors}
    return dict(qkv=qkv, d_o=d_o, ref=ref, model=model, bound=bound)


@functools.lru_cache(maxsize=None)
def attn_fused_case(N, P, Cc, heads, s):
    """lfvdm_attn_spatial_fused: the scale is produced through Wqkv (its q and k rows times s)."""
    tag = f"cond/af/{N}/{P}/{Cc}/{heads}"
    xn = rnd(tag + "/xn", N * P, Cc)
    W, bias = rnd(tag + "/w", 3 * Cc, Cc) * (Cc ** -0.5), rnd(tag + "/bias", 3 * Cc) * 0.1
    W[:2 * Cc] *= s
    bias[:2 * Cc] *= s
    outs = {}
    for dt in (torch.float64, torch.float32):
        qkv = xn.to(dt) @ W.to(dt).t() + bias.to(dt)
        outs[dt] = _spatial_core(qkv, N, P, Cc, heads)
    ref, logits = outs[torch.float64][0], outs[torch.float64][3]
    model = float((outs[torch.float32][0].double() - ref).abs().max())
    floor = 2e-5          # close(o, o2, 2e-5) of the existing test
    return dict(xn=xn, W=W, bias=bias, ref=ref, logits=logits, attn=outs[torch.float64][1], model=model, bound=4 * model + floor)


def _temporal_all(qkv, Rs, d_o, mask, B, T, P, Cc, heads, dtype):
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in [qkv] + list(Rs)]
    o = _temporal_core_f64(leaves[0], leaves[1], leaves[2], leaves[3], mask.to(dtype), B, T, P, Cc, heads)
    (o * d_o.to(dtype)).sum().backward()
    return [o.detach()] + [t.grad for t in leaves]


def _temporal_logits(qkv, Rq, Rk, mask, B, T, P, Cc, heads, dtype=torch.float64):
    """Logits and probabilities of the temporal core (the statements of _temporal_core_f64) in ``dtype``."""
    Fh = Cc // heads
    scale = Fh ** -0.5
    x = qkv.to(dtype).view(B, T, P, 3, heads, Fh).permute(3, 0, 2, 4, 1, 5)
    q, k = x[0] * scale, x[1]
    logits = q @ k.transpose(-1, -2)
    logits = logits + torch.einsum("bdhtf,btshf->bdhts", q, Rk.to(dtype).view(B, T, T, heads, Fh))
    logits = logits + torch.einsum("bdhtf,btshf->bdhts", k * scale, Rq.to(dtype).view(B, T, T, heads, Fh)).transpose(-1, -2)
    m = mask.to(dtype).view(B, T)
    same = m[:, None, :] * m[:, :, None] + (1 - m[:, None, :]) * (1 - m[:, :, None])
    logits = logits.masked_fill((same == 0).view(B, 1, 1, T, T), float("-inf"))
    return logits, torch.softmax(logits, -1)


MASK_PATTERNS = ["zeros", "one_obs_first", "one_obs_middle", "one_obs_last", "one_latent", "alternating"]


def mask_pattern(name, B, T):
    m = torch.zeros(B, T)
    if name == "one_obs_first":
        m[:, 0] = 1
    elif name == "one_obs_middle":
        m[:, T // 2] = 1
    elif name == "one_obs_last":
        m[:, T - 1] = 1
    elif name == "one_latent":
        m[:] = 1
        m[:, T // 3] = 0
    elif name == "alternating":
        m[:, ::2] = 1
    elif name == "random":
        from oracle import recipe
        m = (torch.from_numpy(recipe.uniform_pm1("cond/mask", B * T)).view(B, T) > 0).float()
    return m


def lone_frame(name, T):
    """Index of the frame that is alone in its class, or None."""
    return {"one_obs_first": 0, "one_obs_middle": T // 2, "one_obs_last": T - 1, "one_latent": T // 3}.get(name)


@functools.lru_cache(maxsize=None)
def attn_temporal_case(B, T, P, Cc, heads, s, pattern="random"):
    tag = f"cond/at/{B}/{T}/{P}/{Cc}/{heads}"
    M = B * T * P
    qkv = rnd(tag + "/qkv", M, 3 * Cc)
    qkv[:, :2 * Cc] *= s
    Rs = tuple(0.3 * rnd(f"{tag}/R{i}", B, T, T, Cc) for i in range(3))
    d_o = rnd(tag + "/do", M, Cc)
    mask = mask_pattern(pattern, B, T)
    ref = _temporal_all(qkv, Rs, d_o, mask, B, T, P, Cc, heads, torch.float64)
    mod = _temporal_all(qkv, Rs, d_o, mask, B, T, P, Cc, heads, torch.float32)
    names = ("o", "dqkv", "dRq", "dRk", "dRv")
    # the existing tests: o 5e-5, probabilities 2e-5; gradients 3e-5 (1 + |g|max) + 3e-5
    floors = [5e-5] + [3e-5 * (1.0 + float(w.abs().max())) + 3e-5 for w in ref[1:]]
    model = {n: float((m_.double() - r_).abs().max()) for n, m_, r_ in zip(names, mod, ref)}
    bound = {n: 4 * model[n] + f_ for n, f_ in zip(names, floors)}
    logits, attn = _temporal_logits(qkv, Rs[0], Rs[1], mask, B, T, P, Cc, heads)
    model["attn"] = float((_temporal_logits(qkv, Rs[0], Rs[1], mask, B, T, P, Cc, heads, torch.float32)[1].double() - attn).abs().max())
    bound["attn"] = 4 * model["attn"] + 2e-5
    return dict(qkv=qkv, Rs=Rs, d_o=d_o, mask=mask, ref=dict(zip(names, ref)), model=model, bound=bound, logits=logits, attn=attn)


# ------------------------------------------------------------------------------------------------------------------------
# 4. GPU tests: GroupNorm sites
# ------------------------------------------------------------------------------------------------------------------------
def _dev(*ts):
    return [t.cuda().contiguous() if t is not None else None for t in ts]


def _check_stats(tag, st, bud):
    """(mean, rstd) side output [N][32][2]: mean absolutely, rstd relatively, 4 x the two-pass model + 1e-5."""
    st = st.double().cpu().reshape(-1, 2)
    e_m = float((st[:, 0] - bud["mean64"]).abs().max())
    e_r = float((st[:, 1] / bud["rstd64"] - 1).abs().max())
    b_m, b_r = 4 * bud["mean_two"] + 1e-5, 4 * bud["rstd_two"] + 1e-5
    print(f"[cond] {tag} stats: mean {e_m:.3e} (model {bud['mean_two']:.3e}, bound {b_m:.3e}), "
          f"rstd rel {e_r:.3e} (model {bud['rstd_two']:.3e}, bound {b_r:.3e})")
    assert e_m <= b_m and e_r <= b_r, (tag, e_m, b_m, e_r, b_r)


def _check_coef(tag, c, cA, cB, N, P, act):
    """x * coefA + coefB reproduces the reference map (test_gn_apply's coefficient check, floor 5e-5 there)."""
    Cc = c["Cc"]
    pre = (c["x"].double().view(N, P, Cc) * cA.cpu().double()[:, None, :] + cB.cpu().double()[:, None, :]).reshape(N * P, Cc)
    held(tag + " coefA/coefB", F.silu(pre) if act else pre, c["ref"], c["bud"]["bound"] + 2e-5, c["bud"]["two"])


@pytest.mark.parametrize("N,P,C0,C1,film,act,regime", GN_APPLY_CASES)
def test_gn_apply_off_centre(nat, N, P, C0, C1, film, act, regime):
    """lfvdm_gn_apply (gn_wave_body.h / groupnorm.hip): output, statistics and coefficients."""
    c = gn_apply_case(N, P, C0, C1, film, act, regime)
    Cc, T = c["Cc"], c["T"]
    out = torch.full((N * P, Cc), float("nan"), device="cuda")
    cA, cB, st = torch.empty(N, Cc, device="cuda"), torch.empty(N, Cc, device="cuda"), torch.empty(N, 32, 2, device="cuda")
    g = _dev(c["a"], c["b"], c["gamma"], c["beta"], c["fm"])
    nat.check(nat.lib().lfvdm_gn_apply(nat.ptr(g[0]), nat.ptr(g[1]), C0, C1, N, P, nat.ptr(g[2]), nat.ptr(g[3]), nat.ptr(g[4]),
                                       T if film else 1, 2 * Cc if film else 0, EPS, act, nat.ptr(out), nat.ptr(cA), nat.ptr(cB),
                                       nat.ptr(st), nat.stream()), "lfvdm_gn_apply")
    held(f"gn_apply {N}x{P}x{C0}+{C1} {regime}", out, c["ref"], c["bud"]["bound"], c["bud"]["two"])
    _check_stats("gn_apply", st, c["bud"])
    _check_coef("gn_apply", c, cA, cB, N, P, act)


@pytest.mark.parametrize("N,P,C0,C1,film,act,drift,regime", GN_WS_CASES)
def test_gn_apply_large_maps_off_centre(nat, N, P, C0, C1, film, act, drift, regime):
    """lfvdm_gn_apply_ws (chunk statistics + Chan merge) and lfvdm_gn_coef_stats on the same inputs; with ``drift`` the chunk
    means differ and the between-chunk term of the merge carries the variance."""
    c = gn_ws_case(N, P, C0, C1, film, act, drift, regime)
    Cc, T = c["Cc"], c["T"]
    L = nat.lib()
    need = int(L.lfvdm_gn_apply_ws_floats(Cc, N, P))
    assert need > 0
    ws = torch.full((need,), float("nan"), device="cuda")
    out = torch.full((N * P, Cc), float("nan"), device="cuda")
    cA, cB, st = torch.empty(N, Cc, device="cuda"), torch.empty(N, Cc, device="cuda"), torch.empty(N, 32, 2, device="cuda")
    g = _dev(c["a"], c["b"], c["gamma"], c["beta"], c["fm"])
    args = (nat.ptr(g[0]), nat.ptr(g[1]), C0, C1, N, P, nat.ptr(g[2]), nat.ptr(g[3]), nat.ptr(g[4]), T if film else 1,
            2 * Cc if film else 0, EPS)
    nat.check(L.lfvdm_gn_apply_ws(*args, act, nat.ptr(out), nat.ptr(cA), nat.ptr(cB), nat.ptr(st), nat.ptr(ws), need, nat.stream()),
              "lfvdm_gn_apply_ws")
    tag = f"gn_apply_ws {N}x{P}x{C0}+{C1} {regime}{' drift' if drift else ''}"
    held(tag, out, c["ref"], c["bud"]["bound"], c["bud"]["two"])
    _check_stats(tag, st, c["bud"])
    _check_coef(tag, c, cA, cB, N, P, act)
    cA2, cB2, st2 = torch.full_like(cA, float("nan")), torch.full_like(cB, float("nan")), torch.full_like(st, float("nan"))
    nat.check(L.lfvdm_gn_coef_stats(*args, nat.ptr(cA2), nat.ptr(cB2), nat.ptr(st2), nat.stream()), "lfvdm_gn_coef_stats")
    _check_stats(tag + " (gn_coef_stats)", st2, c["bud"])
    _check_coef(tag + " (gn_coef_stats)", c, cA2, cB2, N, P, act)


@pytest.mark.parametrize("N,P,C0,C1,film,act,regime", GN_COEF_CASES)
def test_gn_coef_off_centre(nat, N, P, C0, C1, film, act, regime):
    """lfvdm_gn_coef on a concatenated shape: x * coefA + coefB against the fp64 map."""
    c = gn_coef_case(N, P, C0, C1, film, act, regime)
    Cc, T = c["Cc"], c["T"]
    cA, cB = torch.full((N, Cc), float("nan"), device="cuda"), torch.full((N, Cc), float("nan"), device="cuda")
    g = _dev(c["a"], c["b"], c["gamma"], c["beta"], c["fm"])
    nat.gn_coef(g[0], g[1], C0, C1, N, P, g[2], g[3], g[4], T if film else 1, 2 * Cc if film else 0, EPS, cA, cB)
    pre = (c["x"].double().view(N, P, Cc) * cA.cpu().double()[:, None, :] + cB.cpu().double()[:, None, :]).reshape(N * P, Cc)
    held(f"gn_coef {N}x{P}x{C0}+{C1} {regime}", F.silu(pre) if act else pre, c["ref"], c["bud"]["bound"], c["bud"]["two"])


# One shape per branch of gn_fwd_launch (csrc/groupnorm.hip): the one-wave kernel; its four-wave form (P >= 128, P % 64 == 0);
# gn_coef_kernel<8> and <16> where gn_wave_launch refuses (P > 256; 32 channels per group, with P <= 8 resp. 16 float4
# per thread: 4 pixel lanes at C = 1024); a concat with FiLM.
GN_ENTRY_CASES = [(2, 16, 64, 0, False), (2, 128, 64, 0, False), (2, 260, 64, 0, False), (2, 520, 64, 0, False),
                  (2, 16, 1024, 0, False), (2, 40, 1024, 0, False), (4, 16, 32, 32, True)]


@pytest.mark.parametrize("N,P,C0,C1,film", GN_ENTRY_CASES)
def test_gn_forward_entries_write_the_same_bits(nat, N, P, C0, C1, film):
    """lfvdm_gn_coef, lfvdm_gn_coef_stats and lfvdm_gn_apply share one launch path and run the same kernel on the same input:
    coefA / coefB of all three, and the statistics of the latter two, are bitwise equal (no tolerance)."""
    Cc, T, L = C0 + C1, 2, nat.lib()
    x = (rnd("gn_entries/x", N * P, Cc) + 0.5).cuda()
    a, b = (x[:, :C0].contiguous(), x[:, C0:].contiguous()) if C1 else (x, None)
    gamma, beta = (1.0 + rnd("gn_entries/gamma", Cc, scale=0.3)).cuda(), rnd("gn_entries/beta", Cc, scale=0.2).cuda()
    fm = rnd("gn_entries/film", N // T, 2 * Cc, scale=0.3).cuda() if film else None
    args = (nat.ptr(a), nat.ptr(b), C0, C1, N, P, nat.ptr(gamma), nat.ptr(beta), nat.ptr(fm), T if film else 1, 2 * Cc if film else 0, EPS)
    got = [[torch.full(s, float("nan"), device="cuda") for s in ((N, Cc), (N, Cc), (N, 32, 2))] for _ in range(3)]
    out = torch.full((N * P, Cc), float("nan"), device="cuda")
    nat.check(L.lfvdm_gn_coef(*args, *map(nat.ptr, got[0][:2]), nat.stream()), "lfvdm_gn_coef")
    nat.check(L.lfvdm_gn_coef_stats(*args, *map(nat.ptr, got[1]), nat.stream()), "lfvdm_gn_coef_stats")
    nat.check(L.lfvdm_gn_apply(*args, nat.ACT_SILU, nat.ptr(out), *map(nat.ptr, got[2]), nat.stream()), "lfvdm_gn_apply")
    bits = [[t.cpu().view(torch.int32) for t in g] for g in got]
    assert all(bool(torch.isfinite(t).all()) for g in (got[0][:2], got[1], got[2], [out]) for t in g)
    for k, name in enumerate(("coefA", "coefB")):
        assert torch.equal(bits[0][k], bits[1][k]) and torch.equal(bits[1][k], bits[2][k]), name
    assert torch.equal(bits[1][2], bits[2][2]), "stats"


@pytest.mark.parametrize("B,T,P,Cc,regime", GNT_CASES, ids=[f"{b}-{t}-{p}-{c}-{_gnt_target(t, c)}-{r}" for b, t, p, c, r in GNT_CASES])
def test_gn_temporal_off_centre(nat, B, T, P, Cc, regime):
    c = gnt_case(B, T, P, Cc, regime)
    x, gamma, beta = _dev(c["x"], c["gamma"], c["beta"])
    y = torch.full((B * T * P, Cc), float("nan"), device="cuda")
    nat.gn_temporal(x, gamma, beta, EPS, y, B, T, P, Cc)
    held(f"gn_temporal {B}x{T}x{P}x{Cc} {regime}", y, c["ref"], c["bud"]["bound"], c["bud"]["two"])


@pytest.mark.parametrize("B,T,P,Cc,regime", GNT_QKV_CASES)
def test_gn_temporal_qkv_off_centre(nat, B, T, P, Cc, regime):
    c = gnt_qkv_case(B, T, P, Cc, regime)
    L = nat.lib()
    assert L.lfvdm_gn_temporal_qkv_ok(B, T, P, Cc) == 0
    x, gamma, beta, W, bias = _dev(c["x"], c["gamma"], c["beta"], c["W"], c["bias"])
    M = B * T * P
    xn = torch.full((M, Cc), float("nan"), device="cuda")
    qkv = torch.full((M, 3 * Cc), float("nan"), device="cuda")
    nat.check(L.lfvdm_gn_temporal_qkv(nat.ptr(x), nat.ptr(gamma), nat.ptr(beta), EPS, nat.ptr(xn), nat.ptr(W), nat.ptr(bias),
                                      nat.ptr(qkv), B, T, P, Cc, nat.stream()), "lfvdm_gn_temporal_qkv")
    held(f"gn_temporal_qkv xn {B}x{T}x{P}x{Cc} {regime}", xn, c["ref"], c["bud"]["bound"], c["bud"]["two"])
    held(f"gn_temporal_qkv qkv {B}x{T}x{P}x{Cc} {regime}", qkv, c["ref_q"], c["bud_q"]["bound"], c["bud_q"]["two"])


@pytest.mark.parametrize("N,Cc,P,regime", PROJ_GN_CASES)
def test_proj_gn_off_centre(nat, N, Cc, P, regime):
    c = proj_gn_case(N, Cc, P, regime)
    L = nat.lib()
    assert L.lfvdm_proj_gn_ok(N, P, Cc) == 0
    o, res, W, bias, gamma, beta = _dev(c["o"], c["res"], c["W"], c["bias"], c["gamma"], c["beta"])
    out = torch.full((N * P, Cc), float("nan"), device="cuda")
    raw = torch.full((N * P, Cc), float("nan"), device="cuda")
    nat.check(L.lfvdm_proj_gn(nat.ptr(o), nat.ptr(W), nat.ptr(bias), nat.ptr(res), nat.ptr(gamma), nat.ptr(beta), EPS, nat.ACT_NONE,
                              nat.ptr(out), nat.ptr(raw), N, P, Cc, nat.stream()), "lfvdm_proj_gn")
    held(f"proj_gn {N}x{Cc}x{P} {regime}", out, c["ref"], c["bud"]["bound"], c["bud"]["two"])


def _codes(nat, a):
    ws = torch.empty(1 << 22, device="cuda")
    cnt = torch.zeros(4096, dtype=torch.int32, device="cuda")
    a.splitk_ws, a.splitk_cnt, a.splitk_ws_floats, a.splitk_cnt_ints = ws.data_ptr(), cnt.data_ptr(), ws.numel(), cnt.numel()
    codes = (C.c_int * 256)()
    n = nat.lib().lfvdm_conv_igemm_candidates(C.byref(a), codes, 256)
    assert n > 0
    return [0] + [codes[i] for i in range(n)], (ws, cnt)


@pytest.mark.parametrize("N,Cin,Cout,H,regime", CONV_GN_CASES)
def test_conv_fused_output_groupnorm_off_centre(nat, N, Cin, Cout, H, regime):
    """The fused output-GroupNorm epilogue of lfvdm_conv_igemm (conv_igemm_body.h), every tune code, both epilogue forms."""
    c = conv_gn_case(N, Cin, Cout, H, regime)
    out = torch.empty(N * H * H, Cout, device="cuda")
    gn_out = torch.empty(N * H * H, Cout, device="cuda")
    keep = dict(src0=cl(c["x"]), W=packed(nat, c["w"]), bias=c["b"].cuda(), gn_gamma=c["gamma"].cuda(), gn_beta=c["beta"].cuda(),
                gn_film=c["fm"].cuda())
    a = nat.fill_conv_args(C0=Cin, N=N, Hs=H, Ws=H, Ho=H, Wo=H, Cout=Cout, out=out, ldo=Cout, ksize=3, gn_out=gn_out,
                           gn_film_div=c["T"], gn_act=nat.ACT_SILU, gn_skip_raw=True, **keep)
    codes, hold = _codes(nat, a)
    worst = 0.0
    for code, general in [(cd, g) for cd in codes for g in (0, 1)]:
        a.tune, a.gn_general = code, general
        gn_out.fill_(float("nan"))
        nat.conv_igemm_struct(a)
        got = from_cl(gn_out, N, H, H, Cout)
        err = float((got.double() - c["ref"].double()).abs().max())
        worst = max(worst, err)
        assert bool(torch.isfinite(got).all()) and err <= c["bud"]["bound"], \
            f"tune code {code}, general form {general}: {err:.3e} > {c['bud']['bound']:.3e}"
    print(f"[cond] conv fused GroupNorm {N}x{Cin}x{Cout}x{H} {regime}: kernel {worst:.3e} over {2 * len(codes)} variants, "
          f"two-pass model {c['bud']['two']:.3e}, bound {c['bud']['bound']:.3e}")


@pytest.mark.parametrize("N,Cin,C0,C1,H,regime", CONCAT_GN_CASES)
def test_concat_groupnorm_half_by_half_off_centre(nat, N, Cin, C0, C1, H, regime):
    """GroupNorm32 + SiLU over concat(conv3x3(x), skip): the conv half in the GEMM's epilogue (gn_gw / gn_ld), the skip half
    by lfvdm_gn_apply_part; the halves sit at +64 and -32."""
    c = concat_gn_case(N, Cin, C0, C1, H, regime)
    Cc, P, M = C0 + C1, H * H, N * H * H
    gw = Cc // 32
    act = torch.full((M, Cc), float("nan"), device="cuda")
    raw = torch.empty(M, C0, device="cuda")
    g_dev, b_dev = c["gamma"].cuda(), c["beta"].cuda()
    sk = cl(c["skip"])
    nat.check(nat.lib().lfvdm_gn_apply_part(sk.data_ptr(), C1, N, P, gw, g_dev.data_ptr() + 4 * C0, b_dev.data_ptr() + 4 * C0, EPS,
                                            nat.ACT_SILU, act.data_ptr() + 4 * C0, Cc, nat.stream()), "lfvdm_gn_apply_part")
    keep = dict(src0=cl(c["x"]), W=packed(nat, c["w"]), bias=c["b"].cuda())
    a = nat.fill_conv_args(C0=Cin, N=N, Hs=H, Ws=H, Ho=H, Wo=H, Cout=C0, out=raw, ldo=C0, gn_out=act, gn_gamma=g_dev, gn_beta=b_dev,
                           gn_film_div=1, gn_act=nat.ACT_SILU, gn_skip_raw=0, **keep)
    a.gn_gw, a.gn_ld = gw, Cc
    codes, hold = _codes(nat, a)
    worst = 0.0
    for code, general in [(cd, g) for cd in codes for g in (0, 1)]:
        a.tune, a.gn_general = code, general
        act[:, :C0].fill_(float("nan"))
        nat.conv_igemm_struct(a)
        got = from_cl(act, N, H, H, Cc)
        err = float((got.double() - c["ref"].double()).abs().max())
        worst = max(worst, err)
        assert bool(torch.isfinite(got).all()) and err <= c["bud"]["bound"], \
            f"tune code {code}, general form {general}: {err:.3e} > {c['bud']['bound']:.3e}"
    print(f"[cond] concat GroupNorm {N}x{Cin}x{C0}+{C1}x{H} {regime}: kernel {worst:.3e} over {2 * len(codes)} variants, "
          f"two-pass model {c['bud']['two']:.3e}, bound {c['bud']['bound']:.3e}")


# ---- backward ----------------------------------------------------------------------------------------------------------
def _run_gn_backward(nat, monkeypatch, c, C0, C1, N, P, T, act, film, tag):
    """_backward._gn_backward in its three delivery modes (atomics: lfvdm_gn_bwd_fused or lfvdm_gn_bwd_ws; deterministic:
    the _sums forms; autograd: lfvdm_gn_bwd_stats + lfvdm_gn_bwd_apply), each against fp64 autograd."""
    from improved_diffusion import _backward as bw
    ac, bc, dac, fc = _dev(c["a"], c["b"], c["da"], c["fm"])
    gpar, bpar = torch.nn.Parameter(c["gamma"].cuda()), torch.nn.Parameter(c["beta"].cuda())
    _, cA, cB, st = bw._gn_apply(ac, bc, C0, C1, N, P, gpar.detach(), bpar.detach(), fc, T, act)
    bound, two = c["bud"]["bound"], c["bud"]["two"]
    for mode in ("atomics", "deterministic", "autograd"):
        monkeypatch.setenv("LFVDM_DETERMINISTIC", "1" if mode == "deterministic" else "0")
        inplace = mode != "autograd"
        gpar.grad = bpar.grad = None
        dxa, dxb, dg, db, _ = bw._gn_backward(dac, ac, bc, C0, C1, N, P, cA, cB, st, act, gpar, bpar, fc, T, inplace=inplace)
        if inplace:
            dg, db = gpar.grad, bpar.grad
        dx = torch.cat([dxa] + ([dxb] if C1 else []), dim=1)
        for name, got, want, bnd, mod in zip(("dx", "dgamma", "dbeta"), (dx, dg, db), c["refs"], bound, two):
            held(f"{tag} {mode} {name}", got, want, bnd, mod)


@pytest.mark.parametrize("C0,C1,pcls,N,T,act,film,regime", GN_BWD_SMALL_CASES)
def test_gn_backward_small_slices_off_centre(nat, monkeypatch, C0, C1, pcls, N, T, act, film, regime):
    """lfvdm_gn_bwd_fused / _fused_sums / _stats + _apply: one slice per channel split, both regimes."""
    P = _p_of(pcls, C0 + C1, 16 * _pl(C0 + C1))
    assert nat.lib().lfvdm_gn_bwd_ws_floats(C0 + C1, N, P) == 0
    c = gn_bwd_case(C0, C1, N, P, T, act, film, regime)
    _run_gn_backward(nat, monkeypatch, c, C0, C1, N, P, T, act, film, f"gn_bwd {C0}+{C1} P{P} N{N} {regime}")


@pytest.mark.parametrize("N,P,C0,C1,film,act,regime", GN_BWD_WS_CASES)
def test_gn_backward_large_maps_off_centre(nat, monkeypatch, N, P, C0, C1, film, act, regime):
    """lfvdm_gn_bwd_ws (the chunked backward) at the workspace shape."""
    assert nat.lib().lfvdm_gn_bwd_ws_floats(C0 + C1, N, P) > 0
    c = gn_bwd_case(C0, C1, N, P, 2, act, film, regime)
    _run_gn_backward(nat, monkeypatch, c, C0, C1, N, P, 2, act, film, f"gn_bwd_ws {N}x{P}x{C0} {regime}")


@pytest.mark.parametrize("B,T,P,Cc,regime", GNT_BWD_CASES)
def test_gn_temporal_backward_off_centre(nat, B, T, P, Cc, regime):
    """lfvdm_gn_temporal_bwd and lfvdm_gn_temporal_bwd_det: a register kernel and the general one."""
    c = gnt_bwd_case(B, T, P, Cc, regime)
    L = nat.lib()
    xc, dyc, gc = _dev(c["x"], c["dy"], c["gamma"])
    need = 2 * (-(-(B * P) // 4)) * Cc
    ws = torch.empty(need, device="cuda")
    for det in (0, 1):
        dx = torch.full((B * T * P, Cc), float("nan"), device="cuda")
        dg, db = torch.zeros(Cc, device="cuda"), torch.zeros(Cc, device="cuda")
        args = (nat.ptr(xc), nat.ptr(dyc), nat.ptr(gc), EPS, nat.ptr(dx), nat.ptr(dg), nat.ptr(db), B, T, P, Cc, 0)
        rc = (L.lfvdm_gn_temporal_bwd_det(*args, ws.data_ptr(), need, nat.stream()) if det else L.lfvdm_gn_temporal_bwd(*args, nat.stream()))
        nat.check(rc, "lfvdm_gn_temporal_bwd" + ("_det" if det else ""))
        for name, got, want, bnd, mod in zip(("dx", "dgamma", "dbeta"), (dx, dg, db), c["refs"], c["bud"]["bound"], c["bud"]["two"]):
            held(f"gn_temporal_bwd{'_det' if det else ''} {B}x{T}x{P}x{Cc} {regime} {name}", got, want, bnd, mod)


# ------------------------------------------------------------------------------------------------------------------------
# 5. GPU tests: softmax cores
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("N,P,Cc,heads,constructed", ATTN_SPATIAL_CASES)
def test_attn_spatial_saturated(nat, N, P, Cc, heads, constructed, s):
    """lfvdm_attn_spatial (output, probabilities, lse) and lfvdm_attn_spatial_bwd at logits of std 9 / 36."""
    c = attn_spatial_case(N, P, Cc, heads, constructed, s)
    qc, doc = _dev(c["qkv"], c["d_o"])
    nanf = lambda *shape: torch.full(shape, float("nan"), device="cuda")      # noqa: E731
    o, a, lse = nanf(N * P, Cc), nanf(N, heads, P, P), nanf(N * heads, P)
    nat.attn_spatial(qc, o, a, N, P, Cc, heads)                      # probabilities, as test_attn_spatial asks for them
    held(f"attn_spatial {N}x{P}x{Cc}x{heads} s={s:g} o (with probabilities)", o, c["ref"]["o"], c["bound"]["o"], c["model"]["o"])
    o = nanf(N * P, Cc)
    nat.attn_spatial(qc, o, None, N, P, Cc, heads, lse=lse)          # lse, as the backward's forward asks for it
    dqkv = nanf(N * P, 3 * Cc)
    nat.attn_spatial_bwd(qc, o, doc, lse, torch.empty(N * heads, P, device="cuda"), dqkv, N, P, Cc, heads)
    tag = f"attn_spatial {N}x{P}x{Cc}x{heads}{' constructed' if constructed else ''} s={s:g}"
    for name, got in (("o", o), ("attn", a), ("lse", lse), ("dqkv", dqkv)):
        held(f"{tag} {name}", got, c["ref"][name], c["bound"][name], c["model"][name])


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("N,P,Cc,heads", ATTN_FUSED_CASES)
def test_attn_spatial_fused_saturated(nat, N, P, Cc, heads, s):
    """lfvdm_attn_spatial_fused (base-2 exponent path); the scale comes through Wqkv."""
    c = attn_fused_case(N, P, Cc, heads, s)
    L = nat.lib()
    assert L.lfvdm_attn_spatial_fused_ok(N, P, Cc, heads) == 0
    xn, W, bias = _dev(c["xn"], c["W"], c["bias"])
    o = torch.full((N * P, Cc), float("nan"), device="cuda")
    nat.check(L.lfvdm_attn_spatial_fused(nat.ptr(xn), nat.ptr(W), nat.ptr(bias), nat.ptr(o), N, P, Cc, heads, nat.stream()),
              "lfvdm_attn_spatial_fused")
    held(f"attn_spatial_fused {N}x{P}x{Cc}x{heads} s={s:g}", o, c["ref"], c["bound"], c["model"])


def _run_temporal(nat, c, B, T, P, Cc, heads, tag):
    M = B * T * P
    g = _dev(c["qkv"], c["d_o"], *c["Rs"], c["mask"])
    nanf = lambda *shape: torch.full(shape, float("nan"), device="cuda")      # noqa: E731
    o, attn = nanf(M, Cc), nanf(B * P, heads, T, T)
    nat.attn_temporal(g[0], g[2], g[3], g[4], g[5], o, attn, B, T, P, Cc, heads)
    dqkv, dRq, dRk, dRv = nanf(M, 3 * Cc), nanf(B, T, T, Cc), nanf(B, T, T, Cc), nanf(B, T, T, Cc)
    ws = torch.empty(2, B * P * heads * T * T, device="cuda")
    nat.attn_temporal_bwd(g[0], g[1], g[2], g[3], g[4], g[5], ws[0], ws[1], dqkv, dRq, dRk, dRv, B, T, P, Cc, heads)
    for name, got in (("o", o), ("dqkv", dqkv), ("dRq", dRq), ("dRk", dRk), ("dRv", dRv)):
        held(f"{tag} {name}", got, c["ref"][name], c["bound"][name], c["model"][name])
    held(f"{tag} attn", attn.view(B, P, heads, T, T), c["attn"], c["bound"]["attn"], c["model"]["attn"])
    return attn, dqkv


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("B,T,P,Cc,heads", ATTN_TEMPORAL_CASES)
def test_attn_temporal_saturated(nat, B, T, P, Cc, heads, s):
    """lfvdm_attn_temporal and lfvdm_attn_temporal_bwd: the second-generation kernels (head dims 32 and 16), the long-window
    kernels and the first-generation kernels <16>, <8> and <32> with the first-generation backward rows kernel (head dims 96
    and 8); test_conditioning_cpu asserts that the shapes reach them by the dispatch's own conditions."""
    c = attn_temporal_case(B, T, P, Cc, heads, s)
    _run_temporal(nat, c, B, T, P, Cc, heads, f"attn_temporal {B}x{T}x{P}x{Cc}x{heads} s={s:g}")


@pytest.mark.parametrize("s", (1.0, 3.0))
@pytest.mark.parametrize("pattern", MASK_PATTERNS)
@pytest.mark.parametrize("B,T,P,Cc,heads", MASK_SHAPES)
def test_attn_temporal_mask_patterns(nat, B, T, P, Cc, heads, pattern, s):
    """Degenerate masks: all latent, one frame in a class of its own (first / middle / last; observed or latent), alternating.
    The lone frame's probability row is exactly one-hot and q and k of that frame get exactly no gradient through the
    logits; everything else is held to the bound.  Once on the second-generation kernels, once on the first generation."""
    c = attn_temporal_case(B, T, P, Cc, heads, s, pattern)
    attn, dqkv = _run_temporal(nat, c, B, T, P, Cc, heads, f"attn_temporal mask {pattern} {Cc}/{heads} s={s:g}")
    t = lone_frame(pattern, T)
    if t is not None:
        row = attn.view(B, P, heads, T, T)[:, :, :, t, :].cpu()
        onehot = torch.zeros(T)
        onehot[t] = 1.0
        assert torch.equal(row, onehot.expand_as(row)), "a softmax over a single entry is exactly one-hot"
        # dS = 0 on that row: dq of the lone frame is exactly 0; its dk only comes from other rows, all masked: exactly 0
        d = dqkv.view(B, T, P, 3, Cc)[:, t].cpu()
        assert float(d[:, :, 0].abs().max()) == 0.0 and float(d[:, :, 1].abs().max()) == 0.0, "dS of a single-entry softmax must be 0"
