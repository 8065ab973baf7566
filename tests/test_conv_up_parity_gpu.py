"""Nearest-2x upsample + 3x3 conv as four 2x2 parity-class GEMMs on pre-summed weights (``lfvdm_conv_args::up = 3``,
``lfvdm_pack_conv_weight_up2x``) against an fp64 CPU reference, with the nine-tap ``up = 1`` launch alongside.  GPU only.

Tolerance against fp64: the one ``tests/test_ops_gpu.py::test_conv_stride2_and_upsample`` uses for ``up = 1``
(|d| <= 2e-5 + 1e-4 * |ref|).  In addition the new form's maximum error must not exceed twice that of the ``up = 1`` launch
on the same input: it does fewer additions, the factor 2 only absorbs the rounding of the summed weights.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import recipe

pytestmark = pytest.mark.gpu

ATOL, RTOL = 2e-5, 1e-4
UNSUPPORTED = 3


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from improved_diffusion import _native
    _native.lib()
    return _native


def rnd(tag, *shape, scale=1.0):
    return torch.from_numpy((scale * recipe.gaussianish(tag, int(np.prod(shape)))).reshape(shape).astype(np.float32))


def cl(x):  # NCHW -> channels-last rows, on device
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def from_cl(y, N, H, W, Cc):
    return y.view(N, H, W, Cc).permute(0, 3, 1, 2).cpu()


def pack_up2x_reference(w):
    """The documented sums in torch CPU fp32: class 2*py + px, tap 2*a + b; source row a collects filter rows {0} | {1, 2}
    (py = 0) or {0, 1} | {2} (py = 1), columns likewise; rows first (per filter column, ascending row), then columns."""
    Cout, Cin = w.shape[:2]
    out = torch.empty(4, Cout, 4, Cin, dtype=torch.float32)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    r0, r1 = (0, py) if a == 0 else (1 + py, 2)
                    c0, c1 = (0, px) if b == 0 else (1 + px, 2)
                    acc = None
                    for c in range(c0, c1 + 1):
                        colsum = w[:, :, r0, c].clone()
                        if r1 > r0:
                            colsum = colsum + w[:, :, r1, c]
                        acc = colsum if acc is None else acc + colsum
                    out[2 * py + px, :, 2 * a + b, :] = acc
    return out


def pack9(nat, w):
    o = torch.empty(w.shape[0], 9, w.shape[1], device="cuda")
    nat.pack_conv_weight(w.cuda().contiguous(), o)
    return o


def pack4(nat, w):
    o = torch.empty(4, w.shape[0], 4, w.shape[1], device="cuda")
    nat.pack_conv_weight_up2x(w.cuda().contiguous(), o)
    return o


def launch(nat, tune=0, **kw):
    """One lfvdm_conv_igemm launch with an explicit tune code (0: the built-in model) and the shared split-K workspace;
    -> the return code."""
    a = nat.fill_conv_args(**kw)
    ws, cnt = nat.splitk_workspace(kw["out"].device)
    a.splitk_ws, a.splitk_cnt, a.splitk_ws_floats, a.splitk_cnt_ints = ws.data_ptr(), cnt.data_ptr(), ws.numel(), cnt.numel()
    a.tune = tune
    rc = nat.lib().lfvdm_conv_igemm(C.byref(a), nat.stream())
    torch.cuda.synchronize()
    return rc


def candidates(nat, **kw):
    a = nat.fill_conv_args(**kw)
    ws, cnt = nat.splitk_workspace(kw["out"].device)
    a.splitk_ws, a.splitk_cnt, a.splitk_ws_floats, a.splitk_cnt_ints = ws.data_ptr(), cnt.data_ptr(), ws.numel(), cnt.numel()
    codes = (C.c_int * 256)()
    n = nat.lib().lfvdm_conv_igemm_candidates(C.byref(a), codes, 256)
    return [codes[i] for i in range(n)]


def case(tag, N, Hs, Ws, Cin, Cout, extras):
    x = rnd(tag + "/x", N, Cin, Hs, Ws)
    w = rnd(tag + "/w", Cout, Cin, 3, 3, scale=0.05)
    b = rnd(tag + "/b", Cout) if extras else None
    r = rnd(tag + "/r", N, Cout, 2 * Hs, 2 * Ws) if extras else None
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), b.double() if extras else None, padding=1)
    if extras:
        ref = ref + r.double()
    return x, w, b, r, ref


def within(out, ref):
    return bool(((out.double() - ref).abs() <= ATOL + RTOL * ref.abs()).all())


@pytest.mark.parametrize("Cout,Cin", [(32, 32), (96, 64)])
def test_pack_is_bitwise_the_documented_sums(nat, Cout, Cin):
    w = rnd(f"up3/pack{Cout}", Cout, Cin, 3, 3, scale=0.05)
    got = pack4(nat, w).cpu()
    assert torch.equal(got, pack_up2x_reference(w))


@pytest.mark.parametrize("N,Hs,Ws,Cin,Cout,extras", [
    (2, 2, 2, 32, 32, False),       # every pixel is a border pixel
    (3, 3, 5, 64, 96, True),        # odd, non-square; class M = 45 is no multiple of a tile; Cout tail; bias + residual
    (2, 8, 8, 128, 128, False),     # the channels of the flagship layer
    (1, 1, 1, 32, 32, False),       # a single source pixel
])
def test_up3_against_fp64_with_up1_alongside(nat, N, Hs, Ws, Cin, Cout, extras):
    x, w, b, r, ref = case(f"up3/op{N}x{Hs}x{Ws}", N, Hs, Ws, Cin, Cout, extras)
    Ho, Wo = 2 * Hs, 2 * Ws
    common = dict(src0=cl(x), C0=Cin, N=N, Hs=Hs, Ws=Ws, Ho=Ho, Wo=Wo, Cout=Cout, ldo=Cout)
    if extras:
        common.update(bias=b.cuda(), res=cl(r).view(N * Ho * Wo, Cout), ldr=Cout)
    out1 = torch.zeros(N * Ho * Wo, Cout, device="cuda")
    out3 = torch.zeros(N * Ho * Wo, Cout, device="cuda")
    assert launch(nat, up=1, W=pack9(nat, w), out=out1, **common) == 0
    assert launch(nat, up=3, W=pack4(nat, w), out=out3, **common) == 0
    o1, o3 = from_cl(out1, N, Ho, Wo, Cout), from_cl(out3, N, Ho, Wo, Cout)
    e1, e3 = float((o1.double() - ref).abs().max()), float((o3.double() - ref).abs().max())
    print(f"[up3 {N}x{Hs}x{Ws} {Cin}->{Cout}] max|d| vs fp64: up=3 {e3:.3e}  up=1 {e1:.3e}  (max|ref| {float(ref.abs().max()):.3f})")
    assert within(o1, ref), e1
    assert within(o3, ref), e3
    assert e3 <= 2 * e1, (e3, e1)


def test_every_legal_tune_code(nat):
    N, Hs, Ws, Cc = 2, 8, 8, 128
    x, w, _, _, ref = case("up3/codes", N, Hs, Ws, Cc, Cc, False)
    Ho, Wo = 2 * Hs, 2 * Ws
    out = torch.empty(N * Ho * Wo, Cc, device="cuda")
    kw = dict(src0=cl(x), C0=Cc, N=N, Hs=Hs, Ws=Ws, Ho=Ho, Wo=Wo, Cout=Cc, ldo=Cc, up=3, W=pack4(nat, w), out=out)
    codes = candidates(nat, **kw)
    split = [c for c in codes if ((c - 1) >> 5) & 7]
    assert codes and split, "the shape has plain and split-K codes"
    worst = 0.0
    for code in codes:
        out.fill_(float("nan"))
        assert launch(nat, tune=code, **kw) == 0, code
        o = from_cl(out, N, Ho, Wo, Cc)
        worst = max(worst, float((o.double() - ref).abs().max()))
        assert within(o, ref), (code, float((o.double() - ref).abs().max()))
    print(f"[up3 codes] {len(codes)} codes ({len(split)} split-K), worst max|d| vs fp64 {worst:.3e}")


def test_illegal_forms_are_refused(nat):
    N, Hs, Ws, Cc = 2, 4, 4, 32
    x, w, _, _, _ = case("up3/refuse", N, Hs, Ws, Cc, Cc, False)
    Ho, Wo = 2 * Hs, 2 * Ws
    src, wp = cl(x), pack4(nat, w)
    base = dict(src0=src, C0=Cc, N=N, Hs=Hs, Ws=Ws, Ho=Ho, Wo=Wo, Cout=Cc, ldo=Cc, up=3, W=wp)
    gamma, beta = torch.ones(Cc, device="cuda"), torch.zeros(Cc, device="cuda")
    gn_out = torch.full((N * Ho * Wo, Cc), 7.0, device="cuda")
    forms = {
        "concat source": dict(base, C1=Cc, src1=src),
        "gn_out": dict(base, gn_out=gn_out, gn_gamma=gamma, gn_beta=beta),
        "nchw": dict(base, out_mode=nat.OUT_NCHW),
    }
    for name, kw in forms.items():
        out = torch.full((N * Ho * Wo, Cc), 7.0, device="cuda")
        assert launch(nat, out=out, **kw) == UNSUPPORTED, name
        assert candidates(nat, out=out, **kw) == [], name
        assert bool((out == 7.0).all()) and bool((gn_out == 7.0).all()), f"{name}: refused, yet something was written"
    out = torch.empty(N * Ho * Wo, Cc, device="cuda")
    assert launch(nat, out=out, **base) == 0


def _cfgA_forward(switch_off, monkeypatch):
    from test_forward_gpu import build_native
    from test_oracle_golden import load_case
    from improved_diffusion import _engine, _native
    if switch_off:
        monkeypatch.setenv("LFVDM_CONV_NO_UP_PARITY", "1")
    else:
        monkeypatch.delenv("LFVDM_CONV_NO_UP_PARITY", raising=False)
    cfg, sd, inp = load_case("cfgA")
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    with torch.no_grad():
        out, _ = model(d["x"], x0=d["x0"], timesteps=d["t"].float(), frame_indices=d["frame_indices"],
                       obs_mask=d["obs_mask"], latent_mask=d["latent_mask"])
    (plan,) = model.native_engine().plans.values()
    L = _native.lib()
    ups = [(a.up, a.N * a.Ho * a.Wo) for fn, args in plan.steps if fn is L.lfvdm_conv_igemm
           for a in (args[0]._obj,) if a.Ho == 2 * a.Hs]
    kinds = [e[2] for e in plan.packs if len(e) == 3]
    return out.cpu(), ups, kinds, _engine.CHAIN_MAX_M


def test_plan_uses_the_form_on_stand_alone_upsamples_only(monkeypatch):
    """The cfg-A plan (1 x 5 frames, 32x32 latent, three upsample convs: 4->8 with 320 output rows - a candidate stage of a
    level chain -, 8->16 and 16->32 stand-alone) built with the form on and with it switched off by
    LFVDM_CONV_NO_UP_PARITY: the outputs agree within the forward tolerance of tests/test_forward_gpu.py, and the launch
    list shows up = 3 on the stand-alone upsample convs only.  (The plan of a no-grad forward is built by the same
    ``Plan._build`` a sampler's plan is; it runs here on the built-in tile choice, without autotuning.)"""
    on, ups_on, kinds_on, max_m = _cfgA_forward(False, monkeypatch)
    off, ups_off, kinds_off, _ = _cfgA_forward(True, monkeypatch)
    err = float((on - off).abs().max())
    print(f"[cfgA plan] max|on - off| = {err:.3e} (max|out| {float(off.abs().max()):.3f}); upsample launches (up, M): {ups_on}")
    assert len(ups_on) == 3 and len(ups_off) == 3
    assert all(up == 1 for up, _ in ups_off) and kinds_off == []
    assert [up for up, M in ups_on] == [1 if M <= max_m else 3 for _, M in ups_on]
    assert sorted(up for up, _ in ups_on) == [1, 3, 3]
    assert kinds_on == ["up2x", "up2x"], "the summed packs are refreshed through the plan's pack list"
    assert torch.allclose(on, off, atol=1e-4, rtol=1e-3), err
