"""The yardstick of test_backward_nodes_gpu: input builders, fp64 restatements and float32 models of the autograd nodes of
``improved_diffusion/_backward.py`` (ConvFn, LinearFn, ResBlockFn, HeadFn, SpatialAttnFn, TemporalAttnFn), checked here
without a GPU.

Every restatement takes and returns tensors in the node's own layouts (channels-last rows [N*H*W][C], FiLM rows per batch
element with T frames sharing a row, the head's (N, Cout, H, W) output) and states the block in plain NCHW torch:
``F.conv2d``, ``F.group_norm`` with 32 groups, ``F.silu``, ``F.interpolate(mode="nearest")``, FiLM ``(1 + scale) * h +
shift``, and the fp64 attention cores the op tests already state.  Evaluated in fp64 it is the reference, evaluated in
float32 on the CPU it is the model: a node's tensor may miss fp64 by at most

    4 x (max error of the float32 model of that tensor) + atol x (1 + |ref|max of that tensor)

with atol the absolute tolerance of the existing op test of the kernel that produces the tensor (``ATOL``).  The factor 4
covers another legitimate summation order and v_exp / v_rcp rounding, as in test_conditioning_gpu.

Checked here: the ResBlock, head and attention-block restatements agree with ``oracle.unet_oracle`` in fp64 to 1e-10
relative; every bound is finite and non-zero; and at every non-square case the fp64 reference with H and W swapped differs
from the reference by more than 10 x the bound, so a swapped H / W inside a node cannot hide in the tolerance."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import recipe, unet_oracle as uo
from test_ops_gpu import rnd, _temporal_core_f64
from test_conditioning_gpu import _spatial_core

# absolute tolerances of the existing op tests, by the kernel that produces a tensor
ATOL = {
    "igemm": 2e-5,       # test_conv3x3_plain / test_conv_stride2_and_upsample: close(..., 2e-5)
    "wgrad": 2e-5,       # test_conv_wgrad_matches_autograd: 2e-5 * max(1, |ref|max)
    "gn_dx": 3e-5,       # test_norm_backward_gpu: tol_dx = 3e-5 * max(|ref|max, 1)
    "gn_par": 2e-4,      # test_norm_backward_gpu: tol_g, tol_b, tol_f = 2e-4 * |ref|max
    "gnt_dx": 5e-5,      # test_gn_temporal_backward: close(dx, ..., 5e-5)
    "gnt_par": 1e-4,     # test_gn_temporal_backward: 1e-4 * max(1, |ref|max)
    "tcore": 3e-5,       # test_attn_temporal_backward: 3e-5 * (1 + |ref|max) + 3e-5
}


# ------------------------------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------------------------------
def nchw(rows, N, H, W):
    return rows.view(N, H, W, rows.shape[-1]).permute(0, 3, 1, 2)


def to_rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _gn(x, g, b):
    return F.group_norm(x, 32, g, b, 1e-5)


def _w(tag, *shape):
    """A weight at the scale of its fan-in."""
    fan = 1
    for d in shape[1:]:
        fan *= d
    return rnd(tag, *shape) * fan ** -0.5


def _affine(tag, C):
    return 1 + 0.1 * rnd(tag + "/g", C), 0.1 * rnd(tag + "/b", C)


# ------------------------------------------------------------------------------------------------------------------------
# restatements: t is a dict of tensors of one dtype in the node's layouts
# ------------------------------------------------------------------------------------------------------------------------
def conv_node(t, N, H, W, stride, up):
    """ConvFn: 3x3 conv, optional stride 2 / nearest-2x upsample in front.  Rows wider than the weight (the input conv's
    zero-padded rows) count with their first Cin channels only."""
    x = nchw(t["x"][:, :t["w"].shape[1]], N, H, W)
    if up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return to_rows(F.conv2d(x, t["w"], t["b"], stride=stride, padding=1))


def linear_node(t):
    y = t["x"] @ t["w"].t()
    if "b" in t:
        y = y + t["b"]
    return y + t["res"] if "res" in t else y


def resblock_node(t, N, H, W, T, keep=None):
    """ResBlockFn on the virtual concat (a | b); film rows [N / T][2 Cout] = (scale | shift), frame n reads row n // T."""
    x = nchw(t["a"], N, H, W)
    if "b" in t:
        x = torch.cat([x, nchw(t["b"], N, H, W)], dim=1)
    Cout = t["w1"].shape[0]
    h = F.conv2d(F.silu(_gn(x, t["g1"], t["be1"])), t["w1"], t["b1"], padding=1)
    film = t["film"].repeat_interleave(T, dim=0)[:, :, None, None]
    h = F.silu(_gn(h, t["g2"], t["be2"]) * (1 + film[:, :Cout]) + film[:, Cout:])
    if keep is not None:
        h = h * nchw(keep.to(h.dtype), N, H, W)
    h = F.conv2d(h, t["w2"], t["b2"], padding=1)
    if "ws" in t:
        x = F.conv2d(x, t["ws"], t["bs"])
    return to_rows(x + h)


def head_node(t, N, H, W):
    """HeadFn: conv3x3(SiLU(GN(h))) in the frame layout (N, Cout, H, W)."""
    return F.conv2d(F.silu(_gn(nchw(t["h"], N, H, W), t["g"], t["be"])), t["w"], t["b"], padding=1)


def spatial_node(t, N, P, heads):
    """SpatialAttnFn: xn + proj(attention(qkv(xn))), xn = GroupNorm over (C / 32, P) of each frame."""
    C = t["x"].shape[1]
    xn = _gn(t["x"].view(N, P, C).permute(0, 2, 1), t["gn_w"], t["gn_b"]).permute(0, 2, 1).reshape(N * P, C)
    o = _spatial_core(xn @ t["wqkv"].t() + t["bqkv"], N, P, C, heads)[0]
    return xn + o @ t["wproj"].t() + t["bproj"]


def temporal_node(t, B, T, P, heads, mask):
    """TemporalAttnFn on rows (b, t, p): GroupNorm over (C / 32, T) of each (b, p), then the RPE core with R given."""
    C = t["x"].shape[1]
    xc = t["x"].view(B, T, P, C).permute(0, 2, 3, 1).reshape(B * P, C, T)
    xn = _gn(xc, t["gn_w"], t["gn_b"]).view(B, P, C, T).permute(0, 3, 1, 2).reshape(B * T * P, C)
    qkv = xn @ t["wqkv"].t() + t["bqkv"]
    o = _temporal_core_f64(qkv, t["Rq"], t["Rk"], t["Rv"], mask.to(qkv.dtype), B, T, P, C, heads)
    return xn + o @ t["wproj"].t() + t["bproj"]


# ------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------
class Case:
    """inputs: name -> float32 tensor (every one a leaf of the comparison); fn(t, H, W) -> output; kinds: tensor name ->
    ATOL key ("out" and "d<input>"); geometry: (H, W) or None; geo_free: tensors that cannot depend on H / W."""

    def __init__(self, tag, inputs, fn, kinds, probe_shape, geometry=None, geo_free=()):
        self.tag, self.inputs, self.fn, self.kinds, self.geometry, self.geo_free = tag, inputs, fn, kinds, geometry, set(geo_free)
        self.probe = rnd(tag + "/probe", *probe_shape)
        self._memo = {}

    def evaluate(self, dtype, transposed=False):
        key = (dtype, transposed)
        if key not in self._memo:
            t = {k: v.to(dtype).clone().requires_grad_(True) for k, v in self.inputs.items()}
            H, W = self.geometry if self.geometry else (None, None)
            out = self.fn(t, W, H) if transposed else self.fn(t, H, W)
            (out.reshape(-1) * self.probe.to(dtype).reshape(-1)).sum().backward()
            res = {"out": out.detach()}
            res.update({"d" + k: v.grad for k, v in t.items()})
            self._memo[key] = res
        return self._memo[key]

    @property
    def ref(self):
        return self.evaluate(torch.float64)

    def model_error(self, name):
        return float((self.evaluate(torch.float32)[name].double() - self.ref[name]).abs().max())

    def bound(self, name, want=None):
        """4 x float32-model error + atol (1 + |want|max); want defaults to the fp64 reference of the tensor."""
        want = self.ref[name] if want is None else want
        return 4 * self.model_error(name) + ATOL[self.kinds[name]] * (1.0 + float(want.abs().max()))


CONV_SHAPES = [(3, 64, 64, 8, 8), (5, 64, 96, 4, 8), (3, 128, 64, 6, 10), (2, 32, 32, 8, 4), (13, 64, 64, 1, 3)]
CONV_CASES = ([s + (1, False) for s in CONV_SHAPES] + [s + (2, False) for s in CONV_SHAPES if s[3] % 2 == 0 and s[4] % 2 == 0]
              + [(5, 64, 96, 4, 8, 1, True), (3, 64, 64, 3, 5, 1, True), (2, 32, 32, 8, 4, 1, True)])
CONV_SLOT_CASES = [s + (2, False) for s in CONV_SHAPES[:4]]
CONV_IN_CASE = (3, 5, 64, 4, 8, 1, False, 32)             # the input conv: 5 real channels on 32-channel rows


@functools.lru_cache(maxsize=None)
def conv_case(N, Cin, Cout, H, W, stride, up, cin_pad=0):
    tag = f"bn/conv/{N}/{Cin}/{Cout}/{H}x{W}/{stride}/{int(up)}/{cin_pad}"
    inputs = dict(x=rnd(tag + "/x", N * H * W, cin_pad or Cin), w=_w(tag + "/w", Cout, Cin, 3, 3), b=0.1 * rnd(tag + "/b", Cout))
    Hi, Wi = (2 * H, 2 * W) if up else (H, W)
    Mo = N * ((Hi - 1) // stride + 1) * ((Wi - 1) // stride + 1)
    kinds = dict(out="igemm", dx="igemm", dw="wgrad", db="wgrad")
    return Case(tag, inputs, lambda t, h, w: conv_node(t, N, h, w, stride, up), kinds, (Mo, Cout), (H, W), geo_free=["db"])


LINEAR_CASES = [(M, K, O, res, True) for M in (70, 257) for K, O in ((64, 192), (128, 128), (96, 32)) for res in (False, True)] \
    + [(70, K, O, False, False) for K, O in ((64, 192), (128, 128), (96, 32))]


@functools.lru_cache(maxsize=None)
def linear_case(M, K, O, res, bias):
    tag = f"bn/lin/{M}/{K}/{O}/{int(res)}/{int(bias)}"
    inputs = dict(x=rnd(tag + "/x", M, K), w=_w(tag + "/w", O, K))
    if bias:
        inputs["b"] = 0.1 * rnd(tag + "/b", O)
    if res:
        inputs["res"] = rnd(tag + "/res", M, O)
    kinds = dict(out="igemm", dx="igemm", dw="wgrad", db="wgrad", dres="igemm")
    return Case(tag, inputs, lambda t, h, w: linear_node(t), kinds, (M, O))


RES_CHANNELS = [(64, 0, 64), (64, 32, 128), (128, 0, 64), (64, 64, 64)]
RES_MAPS = [(4, 4), (4, 8), (6, 10)]
RES_CASES = [c + m for c in RES_CHANNELS for m in RES_MAPS]
RES_N, RES_T, RES_DROP = 4, 2, 0.25
RES_KINDS = dict(out="igemm", da="gn_dx", db="gn_dx", dfilm="gn_par", dg1="gn_par", dbe1="gn_par", dg2="gn_par", dbe2="gn_par",
                 dw1="wgrad", db1="wgrad", dw2="wgrad", db2="wgrad", dws="wgrad", dbs="wgrad")


def dropout_keep(C0, C1, Cout, H, W):
    """The pinned draw of the dropout case: 0 or 1 / (1 - p) per element of the [N*H*W][Cout] activation."""
    u = torch.from_numpy(recipe.uniform_pm1(f"bn/res/keep/{C0}/{C1}/{Cout}/{H}x{W}", RES_N * H * W * Cout)).view(RES_N * H * W, Cout)
    return ((u + 1) * 0.5 >= RES_DROP).float() / (1.0 - RES_DROP)


@functools.lru_cache(maxsize=None)
def res_case(C0, C1, Cout, H, W, drop=False):
    N, T, Cin = RES_N, RES_T, C0 + C1
    tag = f"bn/res/{C0}/{C1}/{Cout}/{H}x{W}"
    g1, be1 = _affine(tag + "/n1", Cin)
    g2, be2 = _affine(tag + "/n2", Cout)
    inputs = dict(a=rnd(tag + "/a", N * H * W, C0), film=0.3 * rnd(tag + "/film", N // T, 2 * Cout), g1=g1, be1=be1,
                  w1=_w(tag + "/w1", Cout, Cin, 3, 3), b1=0.1 * rnd(tag + "/b1", Cout), g2=g2, be2=be2,
                  w2=_w(tag + "/w2", Cout, Cout, 3, 3), b2=0.1 * rnd(tag + "/b2", Cout))
    if C1:
        inputs["b"] = 1.5 * rnd(tag + "/bskip", N * H * W, C1)
    if Cin != Cout:
        inputs.update(ws=_w(tag + "/ws", Cout, Cin, 1, 1), bs=0.1 * rnd(tag + "/bs", Cout))
    keep = dropout_keep(C0, C1, Cout, H, W) if drop else None
    # b2 and bs see the sum of dout over every row only, and the 1x1 skip's weight gradient is a sum of per-row products
    return Case(tag + ("/drop" if drop else ""), inputs, lambda t, h, w: resblock_node(t, N, h, w, T, keep), RES_KINDS,
                (N * H * W, Cout), (H, W), geo_free=["db2", "dbs", "dws"])


HEAD_CASES = [(C, Cout) + s for C in (64, 128) for Cout in (4, 3) for s in ((4, 8, 8), (6, 4, 8), (2, 6, 10))]


@functools.lru_cache(maxsize=None)
def head_case(C, Cout, N, H, W):
    tag = f"bn/head/{C}/{Cout}/{N}/{H}x{W}"
    g, be = _affine(tag + "/n", C)
    inputs = dict(h=rnd(tag + "/h", N * H * W, C), g=g, be=be, w=_w(tag + "/w", Cout, C, 3, 3), b=0.1 * rnd(tag + "/b", Cout))
    kinds = dict(out="igemm", dh="gn_dx", dg="gn_par", dbe="gn_par", dw="wgrad", db="wgrad")
    return Case(tag, inputs, lambda t, h, w: head_node(t, N, h, w), kinds, (N, Cout, H, W), (H, W), geo_free=["db"])


ATTN_KINDS = dict(out="igemm", dwqkv="wgrad", dbqkv="wgrad", dwproj="wgrad", dbproj="wgrad")


def _attn_inputs(tag, M, C):
    g, be = _affine(tag + "/n", C)
    return dict(x=1.2 * rnd(tag + "/x", M, C) + 0.3, gn_w=g, gn_b=be, wqkv=_w(tag + "/wqkv", 3 * C, C),
                bqkv=0.1 * rnd(tag + "/bqkv", 3 * C), wproj=_w(tag + "/wproj", C, C), bproj=0.1 * rnd(tag + "/bproj", C))


SPATIAL_CASES = [(3, 16, 64, 4), (2, 24, 128, 4), (1, 70, 96, 4), (2, 64, 32, 2)]


@functools.lru_cache(maxsize=None)
def spatial_case(N, P, C, heads):
    tag = f"bn/sa/{N}/{P}/{C}/{heads}"
    kinds = dict(ATTN_KINDS, dx="gn_dx", dgn_w="gn_par", dgn_b="gn_par")
    return Case(tag, _attn_inputs(tag, N * P, C), lambda t, h, w: spatial_node(t, N, P, heads), kinds, (N * P, C))


TEMPORAL_CASES = [(2, 5, 4, 64, 4), (1, 14, 6, 128, 4), (2, 20, 2, 32, 2), (1, 40, 2, 64, 4)]     # the last: long-window kernels


def temporal_mask(B, T):
    """Observed / latent classes per frame, both present in every batch element."""
    m = (torch.from_numpy(recipe.uniform_pm1(f"bn/ta/mask/{B}/{T}", B * T)).view(B, T) > 0).float()
    m[:, 0], m[:, -1] = 1.0, 0.0
    return m


@functools.lru_cache(maxsize=None)
def temporal_case(B, T, P, C, heads):
    tag = f"bn/ta/{B}/{T}/{P}/{C}/{heads}"
    inputs = _attn_inputs(tag, B * T * P, C)
    inputs.update({r: 0.3 * rnd(f"{tag}/{r}", B, T, T, C) for r in ("Rq", "Rk", "Rv")})
    mask = temporal_mask(B, T)
    kinds = dict(ATTN_KINDS, dx="gnt_dx", dgn_w="gnt_par", dgn_b="gnt_par", dRq="tcore", dRk="tcore", dRv="tcore")
    c = Case(tag, inputs, lambda t, h, w: temporal_node(t, B, T, P, heads, mask), kinds, (B * T * P, C))
    c.mask = mask
    return c


def all_cases():
    out = [conv_case(*c) for c in CONV_CASES] + [conv_case(*CONV_IN_CASE)] + [linear_case(*c) for c in LINEAR_CASES]
    out += [res_case(*c) for c in RES_CASES] + [res_case(*RES_CASES[4], drop=True)] + [head_case(*c) for c in HEAD_CASES]
    return out + [spatial_case(*c) for c in SPATIAL_CASES] + [temporal_case(*c) for c in TEMPORAL_CASES]


# ------------------------------------------------------------------------------------------------------------------------
# the restatements against the oracle (fp64)
# ------------------------------------------------------------------------------------------------------------------------
def _agree(tag, got, want):
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f"[nodes] {tag}: restatement vs oracle {err:.3e} (scale {scale:.3e})")
    assert err <= 1e-10 * scale, f"{tag}: {err:.3e} vs scale {scale:.3e}"


def _f64(inputs):
    return {k: v.double() for k, v in inputs.items()}


@pytest.mark.parametrize("C0,C1,Cout,H,W", RES_CASES)
def test_resblock_restatement_is_the_oracles(C0, C1, Cout, H, W):
    N, T, ted = RES_N, RES_T, 128
    keep = dropout_keep(C0, C1, Cout, H, W).double()
    t = _f64(res_case(C0, C1, Cout, H, W).inputs)
    emb = rnd("bn/res/emb", N // T, ted).double()
    we, bemb = _w("bn/res/we", 2 * Cout, ted).double(), 0.1 * rnd("bn/res/bemb", 2 * Cout).double()
    t["film"] = F.linear(uo.silu(emb), we, bemb)
    sd = {"p.in_layers.0.weight": t["g1"], "p.in_layers.0.bias": t["be1"], "p.in_layers.2.weight": t["w1"],
          "p.in_layers.2.bias": t["b1"], "p.emb_layers.1.weight": we, "p.emb_layers.1.bias": bemb,
          "p.out_layers.0.weight": t["g2"], "p.out_layers.0.bias": t["be2"], "p.out_layers.3.weight": t["w2"],
          "p.out_layers.3.bias": t["b2"]}
    if "ws" in t:
        sd.update({"p.skip_connection.weight": t["ws"], "p.skip_connection.bias": t["bs"]})
    x = nchw(t["a"], N, H, W)
    if "b" in t:
        x = torch.cat([x, nchw(t["b"], N, H, W)], dim=1)
    for k in (None, keep):
        want = uo.res_block(sd, "p", x, emb.repeat_interleave(T, 0), keep=nchw(k, N, H, W) if k is not None else None)
        _agree(f"resblock {C0}+{C1}->{Cout} {H}x{W} keep={k is not None}", resblock_node(t, N, H, W, T, k), to_rows(want))


@pytest.mark.parametrize("C,Cout,N,H,W", HEAD_CASES)
def test_head_restatement_is_the_oracles(C, Cout, N, H, W):
    """The head of uo.unet_forward: silu(group_norm32(h, out.0)) -> conv2d(out.2)."""
    t = _f64(head_case(C, Cout, N, H, W).inputs)
    want = F.conv2d(uo.silu(uo.group_norm32(nchw(t["h"], N, H, W), t["g"], t["be"])), t["w"], t["b"], padding=1)
    _agree(f"head {C}->{Cout} {N}x{H}x{W}", head_node(t, N, H, W), want)


def _attn_sd(t):
    return {"p.norm.weight": t["gn_w"], "p.norm.bias": t["gn_b"], "p.qkv.weight": t["wqkv"], "p.qkv.bias": t["bqkv"],
            "p.proj_out.weight": t["wproj"], "p.proj_out.bias": t["bproj"]}


@pytest.mark.parametrize("N,P,C,heads", SPATIAL_CASES)
def test_spatial_block_restatement_is_the_oracles(N, P, C, heads):
    t = _f64(spatial_case(N, P, C, heads).inputs)
    x = t["x"].view(1, N, P, C).permute(0, 1, 3, 2)                      # oracle layout (B, D = frames, C, tokens)
    want, _ = uo.rpe_attention(_attn_sd(t), "p", x, None, None, None, heads, False)
    _agree(f"spatial {N}/{P}/{C}/{heads}", spatial_node(t, N, P, heads), want[0].permute(0, 2, 1).reshape(N * P, C))


@pytest.mark.parametrize("B,T,P,C,heads", TEMPORAL_CASES)
def test_temporal_block_restatement_is_the_oracles(B, T, P, C, heads):
    """R_q / R_k / R_v come from the oracle's RPE networks and are handed to the restatement, as the node receives them."""
    ted = 128
    c = temporal_case(B, T, P, C, heads)
    t = _f64(c.inputs)
    sd = _attn_sd(t)
    for r in ("rpe_q", "rpe_k", "rpe_v"):
        q = f"p.{r}.rpe_net."
        sd.update({q + "embed_distances.weight": _w(f"bn/ta/{r}/wd", C, 3).double(), q + "embed_distances.bias": 0.1 * rnd(f"bn/ta/{r}/bd", C).double(),
                   q + "embed_diffusion_time.weight": _w(f"bn/ta/{r}/wt", C, ted).double(),
                   q + "embed_diffusion_time.bias": 0.1 * rnd(f"bn/ta/{r}/bt", C).double(),
                   q + "out.weight": _w(f"bn/ta/{r}/wo", C, C).double(), q + "out.bias": 0.1 * rnd(f"bn/ta/{r}/bo", C).double()})
    temb = rnd("bn/ta/temb", B, ted).double().repeat_interleave(T, 0)
    fi = torch.stack([torch.arange(T), torch.arange(T) * 3 + 2])[:B]
    rel = fi.unsqueeze(-1) - fi.unsqueeze(-2)
    for r in ("q", "k", "v"):
        t["R" + r] = uo.rpe_net(sd, f"p.rpe_{r}.rpe_net", temb, rel, heads).reshape(B, T, T, C)
    x = t["x"].view(B, T, P, C).permute(0, 2, 3, 1)                    # oracle layout (B, D = pixels, C, T)
    want, _ = uo.rpe_attention(sd, "p", x, temb, fi, c.mask.double(), heads, True)
    _agree(f"temporal {B}/{T}/{P}/{C}/{heads}", temporal_node(t, B, T, P, heads, c.mask), want.permute(0, 3, 1, 2).reshape(B * T * P, C))


# ------------------------------------------------------------------------------------------------------------------------
# the bounds
# ------------------------------------------------------------------------------------------------------------------------
def test_every_bound_is_finite_and_non_zero():
    n = 0
    for c in all_cases():
        for name in c.ref:
            b, m = c.bound(name), c.model_error(name)
            assert 0.0 < b < float("inf") and b == b, (c.tag, name, b)
            assert m <= 1e-3 * (1.0 + float(c.ref[name].abs().max())), (c.tag, name, m)      # the float32 model is a float32 model
            n += 1
    print(f"[nodes] {n} bounds")


def _nonsquare():
    return [c for c in all_cases() if c.geometry and c.geometry[0] != c.geometry[1]]


def test_a_swapped_geometry_cannot_hide_inside_a_bound():
    """Non-square cases: the fp64 reference evaluated with H and W swapped (same rows, same weights) is more than 10 x the
    bound away from the reference, for the output, every input gradient and every weight gradient.  Exempt: tensors that
    cannot depend on the geometry (the gradient of a bias added after the last conv is the sum of the probe's rows, that of
    the 1x1 skip weight a sum of per-row products): those must not move at all."""
    cases = _nonsquare()
    assert len(cases) >= 20
    for c in cases:
        ref, swapped = c.ref, c.evaluate(torch.float64, transposed=True)
        for name in ref:
            if name in c.geo_free:
                assert float((swapped[name].reshape(-1) - ref[name].reshape(-1)).abs().max()) <= 1e-9 * (1 + float(ref[name].abs().max()))
                continue
            d = float((swapped[name].reshape(-1) - ref[name].reshape(-1)).abs().max())
            print(f"[nodes] {c.tag} {name}: swapped geometry {d:.3e}, bound {c.bound(name):.3e}")
            assert d > 10 * c.bound(name), (c.tag, name, d, c.bound(name))
