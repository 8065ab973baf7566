"""The autograd nodes of ``improved_diffusion/_backward.py`` one by one against fp64 autograd of a plain-torch restatement
(test_backward_nodes_cpu holds the builders, the restatements, the float32 models and the bound), and the weight-pack /
gradient-unpack primitives against their definitions.  GPU only.

Each node runs in both gradient delivery modes (``_mode.inplace``) and both reduction modes (LFVDM_DETERMINISTIC); its output,
every input gradient and every parameter gradient must sit within 4 x float32-model error + atol (1 + |ref|max) of fp64, per
tensor.  Deterministic mode runs twice and must repeat bitwise.  Every comparison prints kernel error, model error and bound;
the worst error / bound ratio of each node is printed when the module finishes."""
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_ops_gpu import rnd, cl, from_cl
from test_conditioning_gpu import _spatial_core
import test_backward_nodes_cpu as bn

pytestmark = pytest.mark.gpu

DELIVERY = pytest.mark.parametrize("inplace", [False, True], ids=["autograd", "inplace"])
REDUCTION = pytest.mark.parametrize("det", ["0", "1"], ids=["atomics", "deterministic"])
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    for node, (ratio, where) in sorted(WORST.items()):
        print(f"[nodes] worst error / bound of {node}: {ratio:.3f} ({where})")


@pytest.fixture
def bw(monkeypatch):
    """The module under test; whatever a case leaves in its module-level state is put back afterwards."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from improved_diffusion import _backward, _native
    _native.lib()
    saved = _backward._mode.inplace
    # the grouped embedding / RPE backward belongs to a whole network: gradient slots are filled here, their consumer is not queued
    monkeypatch.setattr(_backward._embed, "queued", True)
    yield _backward
    _backward._mode.inplace = saved
    _backward._SkipSlot.reset_stale()
    _backward._rpe_group.pending = False
    _backward._head_rows.clear()
    if _backward._packed.queued:            # a backward pass that raised never ran its end-of-backward fold
        _backward._packed.flush()
    torch.cuda.synchronize()


def held(node, tag, got, want, bound, model):
    err = float((got.detach().double().cpu().reshape(-1) - want.double().reshape(-1)).abs().max())
    print(f"[nodes] {tag}: kernel {err:.3e}, float32 model {model:.3e}, bound {bound:.3e}")
    assert bool(torch.isfinite(got).all()), f"{tag}: not finite"
    if err / bound > WORST.get(node, (0.0, ""))[0]:
        WORST[node] = (err / bound, tag)
    assert err <= bound, f"{tag}: max|d| = {err:.3e} > {bound:.3e}"


def fill(bw, slot, g):
    """What ``_SkipSlot.put`` does inside a backward pass, from outside of one (no end-of-backward callback to queue)."""
    slot.g = g
    bw._SkipSlot.pending.append(slot)


def leaves(case, params, no_grad=()):
    t = {}
    for k, v in case.inputs.items():
        d = v.cuda().contiguous()
        t[k] = nn.Parameter(d) if k in params else (d if k in no_grad else d.requires_grad_(True))
    return t


def run(bw, case, call, params, inplace, no_grad=()):
    """One forward + backward of a node on fresh leaves -> {"out", "d<input>"} (None where autograd saw no gradient)."""
    bw._mode.inplace = inplace
    t = leaves(case, params, no_grad)
    out = call(t)
    (out * case.probe.cuda().view_as(out)).sum().backward()
    torch.cuda.synchronize()
    res = {"out": out.detach()}
    res.update({"d" + k: v.grad for k, v in t.items()})
    return res


def run_checked(bw, case, call, params, inplace, det, no_grad=()):
    res = run(bw, case, call, params, inplace, no_grad)
    if det == "1":
        again = run(bw, case, call, params, inplace, no_grad)
        diff = [k for k in res if res[k] is not None and not torch.equal(res[k], again[k])]
        assert not diff, f"deterministic mode is not bitwise repeatable: {diff}"
    if inplace:
        bw._SkipSlot.check_drained()
    return res


def compare(node, case, res, mode, skip=(), want=None):
    want = want or {}
    for name in case.ref:
        if name in skip:
            continue
        assert res[name] is not None, f"{case.tag} {name}: no gradient"
        w = want.get(name, case.ref[name])
        held(node, f"{case.tag} {mode} {name}", res[name], w, case.bound(name, w), case.model_error(name))


def mode_id(inplace, det):
    return ("inplace" if inplace else "autograd") + "/" + ("deterministic" if det == "1" else "atomics")


# ------------------------------------------------------------------------------------------------------------------------
# ConvFn
# ------------------------------------------------------------------------------------------------------------------------
def conv_call(bw, N, H, W, stride, up, cin_pad=0, slot=None):
    return lambda t: bw.ConvFn.apply(t["x"], t["w"], t["b"], N, H, W, stride, up, cin_pad, slot)


@REDUCTION
@DELIVERY
@pytest.mark.parametrize("N,Cin,Cout,H,W,stride,up", bn.CONV_CASES)
def test_conv_node(bw, monkeypatch, N, Cin, Cout, H, W, stride, up, inplace, det):
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    case = bn.conv_case(N, Cin, Cout, H, W, stride, up)
    res = run_checked(bw, case, conv_call(bw, N, H, W, stride, up), ("w", "b"), inplace, det)
    compare("ConvFn", case, res, mode_id(inplace, det))


@REDUCTION
@pytest.mark.parametrize("N,Cin,Cout,H,W,stride,up", bn.CONV_SLOT_CASES)
def test_conv_node_adds_the_skip_slot_gradient(bw, monkeypatch, N, Cin, Cout, H, W, stride, up, det):
    """stride 2, in-place mode: the decoder's gradient of x waits in the slot and rides in the data-gradient GEMM's epilogue."""
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    case = bn.conv_case(N, Cin, Cout, H, W, stride, up)
    extra = rnd(case.tag + "/slot", N * H * W, Cin)
    slots = []

    def call(t):
        slots.append(bw._SkipSlot())
        fill(bw, slots[-1], extra.cuda())
        return conv_call(bw, N, H, W, stride, up, 0, slots[-1])(t)
    res = run_checked(bw, case, call, ("w", "b"), True, det)
    assert all(s.g is None for s in slots), "the slot must be drained"
    compare("ConvFn", case, res, mode_id(True, det) + "/slot", want={"dx": case.ref["dx"] + extra.double()})


@REDUCTION
def test_conv_node_of_the_padded_input_conv(bw, monkeypatch, det):
    """cin_pad: a 5-channel weight on 32-channel rows (in-place mode only).  The rows' 27 padding channels are non-zero here,
    so the packed accumulator collects gradients for them: none of it may reach ``w.grad``, and the fold leaves it zero."""
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    N, Cin, Cout, H, W, stride, up, pad = bn.CONV_IN_CASE
    case = bn.conv_case(*bn.CONV_IN_CASE)
    assert float(case.inputs["x"][:, Cin:].abs().min()) > 0
    seen = []

    def call(t):
        seen.append(t["w"])
        return conv_call(bw, N, H, W, stride, up, pad)(t)
    res = run_checked(bw, case, call, ("w", "b"), True, det, no_grad=("x",))
    assert tuple(res["dw"].shape) == (Cout, Cin, 3, 3)
    compare("ConvFn", case, res, mode_id(True, det) + "/cin_pad", skip=("dx",))
    acc = bw._packed.bufs[id(seen[-1])][1]
    assert tuple(acc.shape) == (Cout, 9, pad) and float(acc.abs().max()) == 0.0


def test_conv_node_refuses_a_slot_gradient_without_an_input_gradient(bw):
    N, Cin, Cout, H, W, stride, up = bn.CONV_SLOT_CASES[1]
    case = bn.conv_case(N, Cin, Cout, H, W, stride, up)
    bw._mode.inplace = True
    t = leaves(case, ("w", "b"), no_grad=("x",))
    slot = bw._SkipSlot()
    fill(bw, slot, rnd(case.tag + "/slot", N * H * W, Cin).cuda())
    out = conv_call(bw, N, H, W, stride, up, 0, slot)(t)
    with pytest.raises(RuntimeError, match="computes no input gradient"):
        out.sum().backward()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# LinearFn
# ------------------------------------------------------------------------------------------------------------------------
@REDUCTION
@DELIVERY
@pytest.mark.parametrize("M,K,O,res,bias", bn.LINEAR_CASES)
def test_linear_node(bw, monkeypatch, M, K, O, res, bias, inplace, det):
    """b=None: the node keeps the weight gradient on the autograd path in both modes, so ``w.grad`` must still arrive."""
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    case = bn.linear_case(M, K, O, res, bias)
    got = run_checked(bw, case, lambda t: bw.LinearFn.apply(t["x"], t["w"], t.get("b"), t.get("res")), ("w", "b"), inplace, det)
    compare("LinearFn", case, got, mode_id(inplace, det))


# ------------------------------------------------------------------------------------------------------------------------
# ResBlockFn
# ------------------------------------------------------------------------------------------------------------------------
RES_PARAMS = ("g1", "be1", "w1", "b1", "g2", "be2", "w2", "b2", "ws", "bs")


def res_call(bw, H, W, dfilm_slot=None, drop_p=0.0, a_slot=None, b_slot=None):
    return lambda t: bw.ResBlockFn.apply(t["a"], t.get("b"), t["film"], t["g1"], t["be1"], t["w1"], t["b1"], t["g2"], t["be2"],
                                         t["w2"], t["b2"], t.get("ws"), t.get("bs"), bn.RES_N, H, W, bn.RES_T, dfilm_slot, drop_p,
                                         a_slot, b_slot)


@REDUCTION
@DELIVERY
@pytest.mark.parametrize("C0,C1,Cout,H,W", bn.RES_CASES)
def test_resblock_node(bw, monkeypatch, C0, C1, Cout, H, W, inplace, det):
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    case = bn.res_case(C0, C1, Cout, H, W)
    res = run_checked(bw, case, res_call(bw, H, W), RES_PARAMS, inplace, det)
    compare("ResBlockFn", case, res, mode_id(inplace, det))


@REDUCTION
@DELIVERY
def test_resblock_node_with_dropout(bw, monkeypatch, inplace, det):
    """drop_p > 0 with the draw pinned: the same keep factors go to the restatement."""
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    C0, C1, Cout, H, W = bn.RES_CASES[4]
    case = bn.res_case(C0, C1, Cout, H, W, drop=True)
    keep = bn.dropout_keep(C0, C1, Cout, H, W).cuda()
    monkeypatch.setattr(bw, "_dropout_keep", lambda act, p: keep)
    res = run_checked(bw, case, res_call(bw, H, W, drop_p=bn.RES_DROP), RES_PARAMS, inplace, det)
    compare("ResBlockFn", case, res, mode_id(inplace, det) + "/dropout")


@REDUCTION
@pytest.mark.parametrize("C0,C1,Cout,H,W", [(64, 0, 64, 4, 8), (128, 0, 64, 4, 8)], ids=["identity-add2", "skip1x1-epilogue"])
def test_resblock_node_adds_the_a_slot_gradient(bw, monkeypatch, C0, C1, Cout, H, W, det):
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    case = bn.res_case(C0, C1, Cout, H, W)
    extra = rnd(case.tag + "/aslot", bn.RES_N * H * W, C0)
    slots = []

    def call(t):
        slots.append(bw._SkipSlot())
        fill(bw, slots[-1], extra.cuda())
        return res_call(bw, H, W, a_slot=slots[-1])(t)
    res = run_checked(bw, case, call, RES_PARAMS, True, det)
    assert all(s.g is None for s in slots), "the slot must be drained"
    compare("ResBlockFn", case, res, mode_id(True, det) + "/a_slot", want={"da": case.ref["da"] + extra.double()})


@REDUCTION
def test_resblock_node_hands_the_gradient_of_b_to_its_slot(bw, monkeypatch, det):
    """b_slot receives d b and autograd sees None.  The consumer of the slot is a hook on the gradient of ``a`` here (the
    node's backward has run by then), standing in for the encoder-side kernel that drains the slot in a whole network."""
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    C0, C1, Cout, H, W = 64, 32, 128, 4, 8
    case = bn.res_case(C0, C1, Cout, H, W)
    taken = []

    def call(t):
        slot = bw._SkipSlot()
        t["a"].register_hook(lambda g: taken.append(slot.take()))
        return res_call(bw, H, W, b_slot=slot)(t)
    res = run_checked(bw, case, call, RES_PARAMS, True, det)
    assert res["db"] is None, "autograd must not see the gradient that went to the slot"
    assert taken[-1] is not None
    if det == "1":
        assert torch.equal(taken[0], taken[1])
    res["db"] = taken[-1]
    compare("ResBlockFn", case, res, mode_id(True, det) + "/b_slot")


@REDUCTION
def test_resblock_node_writes_the_film_gradient_to_its_slot(bw, monkeypatch, det):
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    C0, C1, Cout, H, W = 64, 32, 128, 6, 10
    case = bn.res_case(C0, C1, Cout, H, W)
    dfilm = []

    def call(t):
        dfilm.append(torch.zeros(bn.RES_N // bn.RES_T, 2 * Cout, device="cuda"))
        return res_call(bw, H, W, dfilm_slot=dfilm[-1])(t)
    res = run_checked(bw, case, call, RES_PARAMS, True, det)
    assert res["dfilm"] is None, "autograd must not see the gradient that went to the slot"
    if det == "1":
        assert torch.equal(dfilm[0], dfilm[1])
    res["dfilm"] = dfilm[-1]
    compare("ResBlockFn", case, res, mode_id(True, det) + "/dfilm_slot")


# ------------------------------------------------------------------------------------------------------------------------
# HeadFn
# ------------------------------------------------------------------------------------------------------------------------
@REDUCTION
@DELIVERY
@pytest.mark.parametrize("C,Cout,N,H,W", bn.HEAD_CASES)
def test_head_node(bw, monkeypatch, C, Cout, N, H, W, inplace, det):
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    case = bn.head_case(C, Cout, N, H, W)
    res = run_checked(bw, case, lambda t: bw.HeadFn.apply(t["h"], t["g"], t["be"], t["w"], t["b"], N, H, W), ("g", "be", "w", "b"),
                      inplace, det)
    assert tuple(res["out"].shape) == (N, Cout, H, W)
    compare("HeadFn", case, res, mode_id(inplace, det))


# ------------------------------------------------------------------------------------------------------------------------
# attention blocks
# ------------------------------------------------------------------------------------------------------------------------
ATTN_PARAMS = ("gn_w", "gn_b", "wqkv", "bqkv", "wproj", "bproj")


def spatial_call(bw, N, P, heads, sink=None):
    return lambda t: bw.SpatialAttnFn.apply(t["x"], t["gn_w"], t["gn_b"], t["wqkv"], t["bqkv"], t["wproj"], t["bproj"], N, P, heads,
                                            sink)


@REDUCTION
@DELIVERY
@pytest.mark.parametrize("N,P,C,heads", bn.SPATIAL_CASES)
def test_spatial_attention_node(bw, monkeypatch, N, P, C, heads, inplace, det):
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    case = bn.spatial_case(N, P, C, heads)
    res = run_checked(bw, case, spatial_call(bw, N, P, heads), ATTN_PARAMS, inplace, det)
    compare("SpatialAttnFn", case, res, mode_id(inplace, det))


@DELIVERY
@pytest.mark.parametrize("N,P,C,heads", bn.SPATIAL_CASES)
def test_spatial_attention_node_with_an_attention_sink(bw, monkeypatch, N, P, C, heads, inplace):
    """The sink receives |mean over heads| of the probabilities (1e-5: test_attn_spatial); every gradient still holds its
    bound, and repeats bitwise what the run without a sink gave (fixed summation order)."""
    monkeypatch.setenv("LFVDM_DETERMINISTIC", "1")
    case = bn.spatial_case(N, P, C, heads)
    sink = []
    res = run_checked(bw, case, spatial_call(bw, N, P, heads, sink), ATTN_PARAMS, inplace, "0")
    compare("SpatialAttnFn", case, res, mode_id(inplace, "1") + "/sink")
    t = {k: v.double() for k, v in case.inputs.items()}
    xn = F.group_norm(t["x"].view(N, P, C).permute(0, 2, 1), 32, t["gn_w"], t["gn_b"], 1e-5).permute(0, 2, 1).reshape(N * P, C)
    attn = _spatial_core(xn @ t["wqkv"].t() + t["bqkv"], N, P, C, heads)[1]
    assert len(sink) == 1 and not sink[0].requires_grad
    model = float((_spatial_core((xn @ t["wqkv"].t() + t["bqkv"]).float(), N, P, C, heads)[1].double() - attn).abs().max())
    want = attn.mean(dim=1).abs()
    held("SpatialAttnFn", f"{case.tag} sink", sink[0], want, 4 * model + 1e-5 * (1.0 + float(want.max())), model)
    plain = run(bw, case, spatial_call(bw, N, P, heads), ATTN_PARAMS, inplace)
    diff = [k for k in res if k != "out" and not torch.equal(res[k], plain[k])]
    assert not diff, f"the sink changed gradients: {diff}"


@REDUCTION
@DELIVERY
@pytest.mark.parametrize("B,T,P,C,heads", bn.TEMPORAL_CASES)
def test_temporal_attention_node(bw, monkeypatch, B, T, P, C, heads, inplace, det):
    """Autograd delivery: R_q / R_k / R_v are leaves.  In-place delivery: their gradients go to ``dR_slots`` (NaN-filled before
    the call: the kernels overwrite) and autograd sees None."""
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    case = bn.temporal_case(B, T, P, C, heads)
    mask = case.mask.cuda()
    assert 0 < float(case.mask.sum(1).min()) and float(case.mask.sum(1).max()) < T
    slots = []

    def call(t):
        dR = None
        if inplace:
            dR = [torch.full((B, T, T, C), float("nan"), device="cuda") for _ in range(3)]
            slots.append(dR)
        return bw.TemporalAttnFn.apply(t["x"], t["gn_w"], t["gn_b"], t["wqkv"], t["bqkv"], t["wproj"], t["bproj"], t["Rq"], t["Rk"],
                                       t["Rv"], mask, B, T, P, heads, dR)
    res = run_checked(bw, case, call, ATTN_PARAMS, inplace, det)
    if inplace:
        assert res["dRq"] is None and res["dRk"] is None and res["dRv"] is None
        if det == "1":
            assert all(torch.equal(a, b) for a, b in zip(slots[0], slots[1]))
        res.update(dRq=slots[-1][0], dRk=slots[-1][1], dRv=slots[-1][2])
    compare("TemporalAttnFn", case, res, mode_id(inplace, det))


# ------------------------------------------------------------------------------------------------------------------------
# primitives against their definitions
# ------------------------------------------------------------------------------------------------------------------------
PACK_SHAPES = [(64, 64), (96, 160), (4, 64), (33, 7)]


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def pack_t_definition(w):
    Cout, Cin, k, _ = w.shape
    return w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, k * k, Cout)


def pack_definition(w):
    Cout, Cin, k, _ = w.shape
    return w.permute(0, 2, 3, 1).reshape(Cout, k * k, Cin)


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("Cout,Cin", PACK_SHAPES)
def test_weight_packs_are_their_definitions(bw, Cout, Cin, k):
    from improved_diffusion import _native as nat
    w = rnd(f"bn/pack/{Cout}/{Cin}/{k}", Cout, Cin, k, k).cuda()
    o = _nan(Cin, k * k, Cout)
    nat.pack_conv_weight_t(w, o)
    assert torch.equal(o, pack_t_definition(w)), "lfvdm_pack_conv_weight_t"
    o = _nan(Cout, k * k, Cin)
    nat.pack_conv_weight(w, o)
    assert torch.equal(o, pack_definition(w)), "lfvdm_pack_conv_weight"
    # the persistent packs of a leaf parameter, with a padded channel stride: the padding is exactly zero
    p = nn.Parameter(w.clone())
    ld_t, ld_f = (Cout + 31) // 32 * 32 + 32, (Cin + 31) // 32 * 32 + 32
    ot, of = bw._pack_t(p, ld_t), bw._pack(p, ld_f)
    assert tuple(ot.shape) == (Cin, k * k, ld_t) and tuple(of.shape) == (Cout, k * k, ld_f)
    assert torch.equal(ot[:, :, :Cout], pack_t_definition(w)) and float(ot[:, :, Cout:].abs().max()) == 0.0
    assert torch.equal(of[:, :, :Cin], pack_definition(w)) and float(of[:, :, Cin:].abs().max()) == 0.0
    assert torch.equal(bw._pack_t(p), pack_t_definition(w)) and torch.equal(bw._pack(p), pack_definition(w))


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("Cout,Cin", PACK_SHAPES)
def test_gradient_unpack_is_the_inverse_permutation(bw, Cout, Cin, k):
    """lfvdm_unpack_conv_grad: packed [Cout][tap][Cin] -> OIHW, written (over NaN) or added in float32."""
    from improved_diffusion import _native as nat
    gp = rnd(f"bn/unpack/gp/{Cout}/{Cin}/{k}", Cout, k * k, Cin).cuda()
    want = gp.view(Cout, k, k, Cin).permute(0, 3, 1, 2).contiguous()
    g = _nan(Cout, Cin, k, k)
    nat.unpack_conv_grad(gp, g, accumulate=False)
    assert torch.equal(g, want), "accumulate=0"
    g0 = rnd(f"bn/unpack/g0/{Cout}/{Cin}/{k}", Cout, Cin, k, k).cuda()
    g = g0.clone()
    nat.unpack_conv_grad(gp, g, accumulate=True)
    assert torch.equal(g, g0 + want), "accumulate=1"
    assert torch.equal(gp.view(Cout, k, k, Cin).permute(0, 3, 1, 2), want), "the packed source must stay as it was"


def test_data_gradient_is_what_the_transposed_pack_promises(bw):
    """conv_igemm(dout, W = _pack_t(w)) == d/dx conv2d(x, w, padding=1) in fp64, over every launch variant."""
    from improved_diffusion import _native as nat
    N, Cin, Cout, H, W = 3, 64, 96, 6, 10
    x, w, dout = rnd("bn/dg/x", N, Cin, H, W), bn._w("bn/dg/w", Cout, Cin, 3, 3), rnd("bn/dg/d", N, Cout, H, W)

    def dgrad(dt):
        xs = x.to(dt).requires_grad_(True)
        return torch.autograd.grad(F.conv2d(xs, w.to(dt), padding=1), xs, dout.to(dt))[0]
    ref = dgrad(torch.float64)
    model = float((dgrad(torch.float32).double() - ref).abs().max())
    bound = 4 * model + bn.ATOL["igemm"] * (1.0 + float(ref.abs().max()))
    out = torch.empty(N * H * W, Cin, device="cuda")
    ws = torch.empty(1 << 22, device="cuda")
    cnt = torch.zeros(4096, dtype=torch.int32, device="cuda")
    keep = dict(src0=cl(dout), W=bw._pack_t(nn.Parameter(w.cuda())))
    a = nat.fill_conv_args(C0=Cout, N=N, Hs=H, Ws=W, Ho=H, Wo=W, Cout=Cin, out=out, ldo=Cin, ksize=3, **keep)
    a.splitk_ws, a.splitk_cnt, a.splitk_ws_floats, a.splitk_cnt_ints = ws.data_ptr(), cnt.data_ptr(), ws.numel(), cnt.numel()
    codes = (C.c_int * 256)()
    n = nat.lib().lfvdm_conv_igemm_candidates(C.byref(a), codes, 256)
    assert n > 0
    for code in [0] + [codes[i] for i in range(n)]:
        a.tune = code
        out.fill_(float("nan"))
        nat.conv_igemm_struct(a)
        held("pack_t data gradient", f"bn/dg tune code {code}", from_cl(out, N, H, W, Cin), ref, bound, model)
    assert int(cnt.abs().sum()) == 0
