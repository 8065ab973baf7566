"""The conv family at 384 to 1024 channels - the widths of the pixel-space model, BASELINE.json configs[4] - op by op
against fp64 (test_wide_channels_cpu holds the cases, the references and the bound): the implicit-GEMM forward, the data
gradient through the transposed pack, the weight and bias gradient, the conv with the next GroupNorm in its epilogue, and the
ConvFn / ResBlockFn nodes.  GPU only.

Every launch goes through the C ABI wrappers of ``_native`` with outputs pre-filled with NaN, over code 0 and every launch
code the tuners may pick (``lfvdm_conv_igemm_candidates``, ``_native._wgrad_codes``); every element must be finite and within
4 x float32-model error + 2e-5 (1 + |ref|max) of fp64, a second launch of the same forward code must repeat bitwise, the
split-K tickets must be left at zero, deterministic weight gradients must repeat bitwise.  Every variant loop prints its worst
max|d| / bound, the module prints the worst of each family when it finishes.

Observed on an MI355X (worst max|d| / bound over the family; comparisons made; launch codes per case, code 0 included):

    forward 3x3 (28 cases + up = 3)   0.085   3915 comparisons   134 codes per case, 114 of them split-K
    forward 1x1 (8 cases)             0.036    778 comparisons
    data gradient 3x3 (28 cases)      0.094   6111 comparisons
    data gradient 1x1 (8 cases)       0.089    910 comparisons
    weight / bias gradient            0.035   3134 comparisons   every code x (atomics, ample slab, one-slice slab);
                                                                 M slices 1 (3x3 cases) and 2 to 4 (257-row GEMMs)
    conv + GroupNorm epilogue         0.105   2412 comparisons   Cout = 512: 133 codes x 2 epilogue forms; Cout = 384 and the
                                                                 384 + 384 concat: no code offered, refused without a write
    ConvFn node                       0.031     96 comparisons
    ResBlockFn node                   0.022    112 comparisons

No kernel or legality check had to change.
"""
import ctypes as C

import pytest
import torch

import test_backward_nodes_cpu as bn
import test_wide_channels_cpu as wc
from test_backward_nodes_gpu import bw, run_checked, conv_call, res_call, mode_id, DELIVERY, REDUCTION, RES_PARAMS  # noqa: F401

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from improved_diffusion import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    for family, (ratio, where, n) in sorted(WORST.items()):
        print(f"[wide] {family}: worst max|d| / bound {ratio:.3f} ({where}), {n} comparisons")


def held(family, tag, got, want, bound):
    """-> max|d| / bound, asserted finite and at most 1."""
    assert bool(torch.isfinite(got).all()), f"{tag}: not finite"
    ratio = float((got.double() - want).abs().max()) / bound
    worst, where, n = WORST.get(family, (0.0, "", 0))
    WORST[family] = (ratio, tag, n + 1) if ratio >= worst else (worst, where, n + 1)
    assert ratio <= 1.0, f"{tag}: max|d| / bound = {ratio:.3f} (bound {bound:.3e})"
    return ratio


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def dev(case):
    return {k: v.cuda().contiguous() for k, v in case.inputs.items()}


def pack(nat, w):
    o = nan(w.shape[0], w.shape[2] * w.shape[3], w.shape[1])
    nat.pack_conv_weight(w.contiguous(), o)
    return o


def pack_t(nat, w):
    o = nan(w.shape[1], w.shape[2] * w.shape[3], w.shape[0])
    nat.pack_conv_weight_t(w.contiguous(), o)
    return o


def private_workspace(a):
    ws = torch.empty(1 << 22, device="cuda")
    cnt = torch.zeros(4096, dtype=torch.int32, device="cuda")
    a.splitk_ws, a.splitk_cnt, a.splitk_ws_floats, a.splitk_cnt_ints = ws.data_ptr(), cnt.data_ptr(), ws.numel(), cnt.numel()
    return ws, cnt


def candidates(nat, a):
    codes = (C.c_int * 256)()
    n = nat.lib().lfvdm_conv_igemm_candidates(C.byref(a), codes, 256)
    return [codes[i] for i in range(n)]


def split_k(code):
    return ((code - 1) >> 5) & 7


def sweep(nat, family, tag, kw, checks, want_split=False):
    """Every launch code of one implicit-GEMM launch.  kw: the keyword form of the launch; checks: [(tensor, columns or None,
    fp64 reference on the device, bound)], every tensor NaN-filled before each launch."""
    a = nat.fill_conv_args(**kw)
    keep = private_workspace(a)
    codes = candidates(nat, a)
    assert codes, f"{tag}: no launch code offered"
    assert not want_split or any(split_k(c) for c in codes), f"{tag}: no split-K code offered"
    worst, at = 0.0, 0
    for code in [0] + codes:
        a.tune = code
        runs = []
        for _ in range(2):
            for t, _, _, _ in checks:
                t.fill_(float("nan"))
            nat.conv_igemm_struct(a)
            runs.append([t.clone() for t, _, _, _ in checks])
        assert all(torch.equal(u, v) for u, v in zip(*runs)), f"{tag} code {code}: a second launch differs"
        for t, cols, want, bound in checks:
            r = held(family, f"{tag} code {code}", t if cols is None else t[:, cols[0]:cols[1]], want, bound)
            if r > worst:
                worst, at = r, code
    assert int(keep[1].abs().sum()) == 0, f"{tag}: split-K tickets must be left at zero"
    print(f"[wide] {family} {tag}: {len(codes) + 1} codes ({sum(1 for c in codes if split_k(c))} split-K), "
          f"worst max|d| / bound {worst:.3f} (code {at})")
    # once more the way the engine launches it: the tuned code on the shared eager workspace
    for t, _, _, _ in checks:
        t.fill_(float("nan"))
    nat.conv_igemm(**kw)
    for t, cols, want, bound in checks:
        held(family, f"{tag} eager", t if cols is None else t[:, cols[0]:cols[1]], want, bound)
    return codes


def ref_dev(t):
    return t.double().cuda()


# ------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------
def forward_kw(nat, args, d, out):
    N, C0, C1, Cout, H, W, stride, up, skip = args
    Ho, Wo = wc.out_map(H, W, stride, up)
    kw = dict(src0=d["x0"], C0=C0, C1=C1, N=N, Hs=H, Ws=W, Ho=Ho, Wo=Wo, stride=stride, up=up, ksize=3, W=pack(nat, d["w"]), bias=d["b"],
              Cout=Cout, out=out, ldo=Cout)
    if C1:
        kw["src1"] = d["x1"]
    if skip:
        kw.update(s2src0=d["x0"], s2C0=C0, s2C1=C1, W2=d["ws"].view(Cout, C0 + C1).contiguous(), bias2=d["bs"])
        if C1:
            kw["s2src1"] = d["x1"]
    if "res" in d:
        kw.update(res=d["res"], ldr=Cout)
    return kw


@pytest.mark.parametrize("args", wc.FORWARD_CASES, ids=lambda a: "-".join(map(str, a)))
def test_conv_forward_every_tune_code(nat, args):
    """3x3 conv over one source or a virtual concat, + residual, + the 1x1 skip segment over the same raw concat, stride 2 and
    the nearest-2x source: every launch code, a private split-K workspace, then the tuned code on the shared 8 MiB one."""
    case = wc.wide_case(*args)
    d = dev(case)
    out = nan(*case.probe.shape)
    kw = forward_kw(nat, args, d, out)
    sweep(nat, "forward", case.tag, kw, [(out, None, ref_dev(case.ref["out"]), case.bound("out"))], want_split=args[4:6] == (4, 4))


def test_conv_forward_up_parity_every_tune_code(nat):
    """512 -> 512 behind the nearest-2x upsample as four 2x2 parity GEMMs on pre-summed weights (up = 3)."""
    args = wc.UP_PARITY_CASE
    N, C0, _, Cout, H, W = args[:6]
    case = wc.wide_case(*args)
    d = dev(case)
    out = nan(*case.probe.shape)
    w4 = nan(4, Cout, 4, C0)
    nat.pack_conv_weight_up2x(d["w"], w4)
    kw = dict(src0=d["x0"], C0=C0, N=N, Hs=H, Ws=W, Ho=2 * H, Wo=2 * W, up=3, W=w4, bias=d["b"], Cout=Cout, out=out, ldo=Cout)
    sweep(nat, "forward", case.tag + " up=3", kw, [(out, None, ref_dev(case.ref["out"]), case.bound("out"))])


@pytest.mark.parametrize("M,K,O,res", wc.LINEAR_CASES)
def test_linear_forward_every_tune_code(nat, M, K, O, res):
    """The attention blocks' qkv and proj GEMMs (proj with its residual) on 70 and 257 rows."""
    case = bn.linear_case(M, K, O, res, True)
    d = dev(case)
    out = nan(M, O)
    kw = dict(src0=d["x"], C0=K, N=M, Hs=1, Ws=1, Ho=1, Wo=1, ksize=1, W=d["w"], bias=d["b"], Cout=O, out=out, ldo=O)
    if res:
        kw.update(res=d["res"], ldr=O)
    sweep(nat, "forward 1x1", case.tag, kw, [(out, None, ref_dev(case.ref["out"]), case.bound("out"))])


# ------------------------------------------------------------------------------------------------------------------------
# data gradient
# ------------------------------------------------------------------------------------------------------------------------
DGRAD_CASES = [a for a in wc.FORWARD_CASES]
DGRAD_WITH_RESIDUAL = wc.RESAMPLE_CASES[1]        # 512 -> 512, stride 2: the zero-inserted source with a residual riding along


@pytest.mark.parametrize("args", DGRAD_CASES, ids=lambda a: "-".join(map(str, a)))
def test_conv_data_gradient_every_tune_code(nat, args):
    """d/dx of the case: conv_igemm of the output gradient with the transposed pack; the zero-inserted source (up = 2) for a
    stride-2 conv; the 1x1 skip's share as the launch's own 1x1 segment over the same output gradient; the adjoint of the
    nearest-2x upsample as the sum of each 2x2 block of the full-resolution gradient (summed on the host, in fp64)."""
    N, C0, C1, Cout, H, W, stride, up, skip = args
    Cin = C0 + C1
    case = wc.wide_case(*args)
    d = dev(case)
    dout = case.probe.cuda().contiguous()                                   # the probe is d loss / d out
    Ho, Wo = wc.out_map(H, W, stride, up)
    Hi, Wi = (2 * H, 2 * W) if up else (H, W)
    want = torch.cat([case.ref["dx0"]] + ([case.ref["dx1"]] if C1 else []), 1)
    out = nan(N * Hi * Wi, Cin)
    kw = dict(src0=dout, C0=Cout, N=N, Hs=Ho, Ws=Wo, Ho=Hi, Wo=Wi, up=2 if stride == 2 else 0, ksize=3, W=pack_t(nat, d["w"]), Cout=Cin,
              out=out, ldo=Cin)
    if skip:
        kw.update(s2src0=dout, s2C0=Cout, W2=d["ws"].view(Cout, Cin).t().contiguous())
    if args == DGRAD_WITH_RESIDUAL:
        extra = bn.rnd(case.tag + "/slot", N * H * W, Cin)
        kw.update(res=extra.cuda(), ldr=Cin)
        want = want + extra.double()
    # src0's and src1's gradients are tensors of their own, each with its bound
    parts = [("dx0", 0, C0)] + ([("dx1", C0, Cin)] if C1 else [])
    checks = [(out, (lo, hi), ref_dev(want[:, lo:hi]), case.bound(name, want[:, lo:hi])) for name, lo, hi in parts]
    if not up:
        sweep(nat, "data gradient", case.tag, kw, checks, want_split=(Hi, Wi) == (4, 4))
        return
    # the upsampled source: the full-resolution gradient has no reference of its own here, so sum the 2x2 blocks per code
    a = nat.fill_conv_args(**kw)
    keep = private_workspace(a)
    codes = candidates(nat, a)
    assert codes
    worst = 0.0
    for code in [0] + codes:
        a.tune = code
        out.fill_(float("nan"))
        nat.conv_igemm_struct(a)
        dx = out.double().view(N, H, 2, W, 2, Cin).sum(dim=(2, 4)).reshape(N * H * W, Cin)
        worst = max(worst, held("data gradient", f"{case.tag} code {code}", dx, checks[0][2], checks[0][3]))
    assert int(keep[1].abs().sum()) == 0
    print(f"[wide] data gradient {case.tag}: {len(codes) + 1} codes, worst max|d| / bound {worst:.3f}")


@pytest.mark.parametrize("M,K,O,res", wc.LINEAR_CASES)
def test_linear_data_gradient_every_tune_code(nat, M, K, O, res):
    case = bn.linear_case(M, K, O, res, True)
    d = dev(case)
    out = nan(M, K)
    kw = dict(src0=case.probe.cuda().contiguous(), C0=O, N=M, Hs=1, Ws=1, Ho=1, Wo=1, ksize=1, W=pack_t(nat, d["w"].view(O, K, 1, 1)),
              Cout=K, out=out, ldo=K)
    sweep(nat, "data gradient 1x1", case.tag, kw, [(out, None, ref_dev(case.ref["dx"]), case.bound("dx"))])


# ------------------------------------------------------------------------------------------------------------------------
# weight and bias gradient
# ------------------------------------------------------------------------------------------------------------------------
def m_slices(code):
    return (code - 1) >> 4


def wgrad_sweep(nat, tag, a, gp, db, want_w, want_b, bound_w, bound_b, unpack):
    """Every code of _wgrad_codes, with float atomics and through the deterministic slabs (ample, and exactly one slice:
    nothing behind the capacity may be touched); the slab runs twice, bitwise equal.  unpack: gp -> OIHW."""
    codes = nat._wgrad_codes(a)
    assert codes, f"{tag}: no launch code offered"
    per = gp.numel() + db.numel()
    ample = torch.empty(16 << 20, device="cuda")
    worst = 0.0
    for code in [0] + codes:
        a.tune = code
        for cap in ("atomics", None, per):
            if cap == "atomics":
                a.splitk_ws, a.splitk_ws_floats = None, 0
                ws = None
            else:
                ws = ample if cap is None else nan(per + 256)
                a.splitk_ws, a.splitk_ws_floats = ws.data_ptr(), (ws.numel() if cap is None else cap)
            runs = []
            for _ in range(1 if cap == "atomics" else 2):
                gp.zero_(); db.zero_()
                nat.check(nat.lib().lfvdm_conv_wgrad(C.byref(a), nat.stream()), f"lfvdm_conv_wgrad code {code} {cap}")
                torch.cuda.synchronize()
                runs.append((gp.clone(), db.clone()))
            if len(runs) == 2:
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"{tag} code {code}: not reproducible"
            if cap == per:
                assert bool(torch.isnan(ws[per:]).all()), f"{tag} code {code}: wrote past the slab"
            worst = max(worst, held("weight gradient", f"{tag} code {code} {cap} dW", unpack(gp), want_w, bound_w),
                        held("weight gradient", f"{tag} code {code} {cap} db", db, want_b, bound_b))
    print(f"[wide] weight gradient {tag}: {len(codes) + 1} codes x 3 modes, M slices {sorted({m_slices(c) for c in codes})}, "
          f"worst max|d| / bound {worst:.3f}")
    return codes


def oihw(k):
    return lambda gp: gp.view(gp.shape[0], k, k, gp.shape[2]).permute(0, 3, 1, 2)


@pytest.mark.parametrize("args", wc.FORWARD_CASES + wc.WGRAD_RESAMPLED_CONCAT, ids=lambda a: "-".join(map(str, a)))
def test_conv_weight_gradient_every_tune_code(nat, args):
    """dW and db of the 3x3 conv (concat sources, stride 2, the upsampled source) and of the 1x1 skip over the same sources."""
    N, C0, C1, Cout, H, W, stride, up, skip = args
    Cin = C0 + C1
    case = wc.wide_case(*args)
    d = dev(case)
    Ho, Wo = wc.out_map(H, W, stride, up)
    dout = case.probe.cuda().contiguous()
    src = dict(src0=d["x0"], C0=C0, C1=C1, N=N, res=dout, ldr=Cout, Cout=Cout)
    if C1:
        src["src1"] = d["x1"]
    gp, db = nan(Cout, 9, Cin), nan(Cout)
    a = nat.fill_conv_args(Hs=H, Ws=W, Ho=Ho, Wo=Wo, ksize=3, stride=stride, up=up, out=gp, bias=db, **src)
    wgrad_sweep(nat, case.tag, a, gp, db, ref_dev(case.ref["dw"]), ref_dev(case.ref["db"]), case.bound("dw"), case.bound("db"), oihw(3))
    if skip:
        gp, db = nan(Cout, 1, Cin), nan(Cout)
        a = nat.fill_conv_args(Hs=H, Ws=W, Ho=H, Wo=W, ksize=1, out=gp, bias=db, **src)
        wgrad_sweep(nat, case.tag + " 1x1 skip", a, gp, db, ref_dev(case.ref["dws"]), ref_dev(case.ref["dbs"]), case.bound("dws"),
                    case.bound("dbs"), oihw(1))


def test_conv_weight_gradient_oihw_output_every_tune_code(nat):
    """out_mode = 1 at 512 + 384 -> 512: dW lands in the parameter's own layout; through the wrappers too (the tuned code, and
    lfvdm_unpack_conv_grad of the packed form)."""
    args = wc.WGRAD_OIHW_CASE
    N, C0, C1, Cout, H, W = args[:6]
    Cin = C0 + C1
    case = wc.wide_case(*args)
    d = dev(case)
    dout = case.probe.cuda().contiguous()
    g, db = nan(Cout, Cin, 3, 3), nan(Cout)
    kw = dict(src0=d["x0"], src1=d["x1"], C0=C0, C1=C1, N=N, Hs=H, Ws=W, Ho=H, Wo=W, ksize=3, res=dout, ldr=Cout, Cout=Cout)
    a = nat.fill_conv_args(out=g, bias=db, out_mode=1, **kw)
    want_w, want_b = ref_dev(case.ref["dw"]), ref_dev(case.ref["db"])
    codes = wgrad_sweep(nat, case.tag + " OIHW", a, g, db, want_w, want_b, case.bound("dw"), case.bound("db"), lambda t: t)
    assert not [c for c in codes if ((c - 1) >> 2) & 3 == 0], "tap-fused codes are offered for the packed layout only"
    gp, g2 = torch.zeros(Cout, 9, Cin, device="cuda"), nan(Cout, Cin, 3, 3)
    db.zero_()
    nat.conv_wgrad(out=gp, bias=db, **kw)
    nat.unpack_conv_grad(gp, g2, accumulate=False)
    held("weight gradient", case.tag + " wrapper + unpack", g2, want_w, case.bound("dw"))
    held("weight gradient", case.tag + " wrapper db", db, want_b, case.bound("db"))


@pytest.mark.parametrize("M,K,O,res", wc.LINEAR_CASES)
def test_linear_weight_gradient_every_tune_code(nat, M, K, O, res):
    case = bn.linear_case(M, K, O, res, True)
    d = dev(case)
    gp, db = nan(O, 1, K), nan(O)
    dout = case.probe.cuda().contiguous()
    a = nat.fill_conv_args(src0=d["x"], C0=K, N=M, Hs=1, Ws=1, Ho=1, Wo=1, ksize=1, res=dout, ldr=O, Cout=O, out=gp, bias=db)
    wgrad_sweep(nat, case.tag, a, gp, db, ref_dev(case.ref["dw"]), ref_dev(case.ref["db"]), case.bound("dw"), case.bound("db"),
                lambda t: t.view(O, K))


def test_weight_gradient_codes_reach_one_and_many_m_slices(nat):
    """The M-slice counts _wgrad_codes offers for the cases above: a single slice (the tile count of a wide layer reaches the
    targets on its own, and a 32-row map leaves nothing to slice) and several (the 257-row GEMMs)."""
    seen = {}
    for N, C0, C1, Cout, H, W, stride, up, _ in wc.FORWARD_CASES + wc.WGRAD_RESAMPLED_CONCAT:
        Ho, Wo = wc.out_map(H, W, stride, up)
        a = nat.ConvArgs()
        a.C0, a.C1, a.Cout, a.N, a.Hs, a.Ws, a.Ho, a.Wo, a.ksize, a.stride, a.up = C0, C1, Cout, N, H, W, Ho, Wo, 3, stride, up
        seen[(N, C0, C1, Cout, Ho, Wo)] = {m_slices(c) for c in nat._wgrad_codes(a)}
    for M, K, O, _ in wc.LINEAR_CASES:
        a = nat.ConvArgs()
        a.C0, a.Cout, a.N, a.Hs, a.Ws, a.Ho, a.Wo, a.ksize, a.stride = K, O, M, 1, 1, 1, 1, 1, 1
        seen[(M, K, O)] = {m_slices(c) for c in nat._wgrad_codes(a)}
    print(f"[wide] M slices per case: {seen}")
    assert all(seen.values()), "every case has launch codes"
    assert any(1 in ms for ms in seen.values()) and any(max(ms) > 1 for ms in seen.values())


# ------------------------------------------------------------------------------------------------------------------------
# conv with the next GroupNorm in its epilogue
# ------------------------------------------------------------------------------------------------------------------------
def refused_without_a_write(nat, a, tensors, tag):
    for general in (0, 1):
        a.tune, a.gn_general = 0, general
        for t in tensors:
            t.fill_(float("nan"))
        rc = nat.lib().lfvdm_conv_igemm(C.byref(a), nat.stream())
        torch.cuda.synchronize()
        assert rc != 0, f"{tag}: neither offered nor refused"
        assert all(bool(torch.isnan(t).all()) for t in tensors), f"{tag}: refused, yet something was written"


@pytest.mark.parametrize("args,skip_raw", list(zip(wc.GN_CASES, wc.GN_SKIP_RAW)), ids=lambda a: "-".join(map(str, a)) if isinstance(a, tuple) else str(a))
def test_conv_fused_output_groupnorm_every_tune_code(nat, args, skip_raw):
    """conv -> GroupNorm32 -> FiLM -> SiLU in fp64 for every offered code, in both forms of the epilogue.  Cout = 384 has 12
    channels per group, which no 32-, 64- or 128-column tile holds whole: if no code is offered, the launch must either be
    right through the general form or be refused without a write."""
    N, Cin, Cout, H, W, film = args
    case = wc.gn_case(*args)
    d = dev(case)
    M = N * H * W
    out, gn_out = nan(M, Cout), nan(M, Cout)
    kw = dict(src0=d["x"], C0=Cin, N=N, Hs=H, Ws=W, Ho=H, Wo=W, ksize=3, W=pack(nat, d["w"]), bias=d["b"], Cout=Cout, out=out, ldo=Cout,
              gn_out=gn_out, gn_gamma=d["g"], gn_beta=d["be"], gn_film=d.get("film"), gn_film_div=wc.GN_T, gn_act=nat.ACT_SILU,
              gn_skip_raw=skip_raw)
    a = nat.fill_conv_args(**kw)
    keep = private_workspace(a)
    codes = candidates(nat, a)
    print(f"[wide] fused GroupNorm {case.tag} skip_raw={skip_raw}: {len(codes)} codes offered")
    ref = ref_dev(case.ref["out"])
    (b_gn, _), (b_raw, _) = wc.part_bound(case, 0, Cout), wc.part_bound(case, Cout, 2 * Cout)
    if not codes:
        assert Cout == 384, "512 filters: 16 channels per group, whole in every tile"
        a.tune, a.gn_general = 0, 1
        rc = nat.lib().lfvdm_conv_igemm(C.byref(a), nat.stream())
        torch.cuda.synchronize()
        if rc == 0:
            held("fused GroupNorm", f"{case.tag} general path", gn_out, ref[:, :Cout], b_gn)
        else:
            refused_without_a_write(nat, a, [out, gn_out], case.tag)
        return
    worst = 0.0
    for code, general in [(c, g) for c in [0] + codes for g in (0, 1)]:
        a.tune, a.gn_general = code, general
        out.fill_(float("nan")); gn_out.fill_(float("nan"))
        nat.conv_igemm_struct(a)
        worst = max(worst, held("fused GroupNorm", f"{case.tag} code {code} general {general}", gn_out, ref[:, :Cout], b_gn))
        if skip_raw:
            assert bool(torch.isnan(out).all()), "raw output must not be written with gn_skip_raw"
        else:
            worst = max(worst, held("fused GroupNorm", f"{case.tag} code {code} general {general} raw", out, ref[:, Cout:], b_raw))
    assert int(keep[1].abs().sum()) == 0
    print(f"[wide] fused GroupNorm {case.tag}: {2 * (len(codes) + 1)} launches, worst max|d| / bound {worst:.3f}")


@pytest.mark.parametrize("args", wc.CONCAT_GN_CASES, ids=lambda a: "-".join(map(str, a)))
def test_concat_groupnorm_half_by_half_every_tune_code(nat, args):
    """GroupNorm32 + SiLU over concat(conv3x3(x), skip) half by half: the conv's half in its epilogue (gn_gw, gn_ld).
    384 + 384: 24 channels per group, whole in no tile - refused without a write if no code is offered."""
    N, Cin, C0, C1, H, W = args
    case = wc.concat_gn_case(*args)
    d = dev(case)
    Cc, M, P = C0 + C1, N * H * W, H * W
    gw = Cc // 32
    act, raw = nan(M, Cc), nan(M, C0)
    ref = ref_dev(case.ref["out"])
    # the skip half is not under test (lfvdm_gn_apply_part stops at 16 channels per group): its columns hold the reference
    # and must stay as they are
    act[:, C0:] = ref[:, C0:Cc].float()
    wp = pack(nat, d["w"])
    a = nat.fill_conv_args(src0=d["x"], C0=Cin, N=N, Hs=H, Ws=W, Ho=H, Wo=W, ksize=3, W=wp, bias=d["b"], Cout=C0, out=raw,
                           ldo=C0, gn_out=act, gn_gamma=d["g"], gn_beta=d["be"], gn_film_div=1, gn_act=nat.ACT_SILU, gn_skip_raw=0)
    a.gn_gw, a.gn_ld = gw, Cc
    keep = private_workspace(a)
    codes = candidates(nat, a)
    print(f"[wide] concat GroupNorm {case.tag}: {len(codes)} codes offered")
    (b_gn, _), (b_raw, _) = wc.part_bound(case, 0, Cc), wc.part_bound(case, Cc, Cc + C0)
    right = act[:, C0:].clone()
    if not codes:
        assert C0 == 384
        for general in (0, 1):
            a.tune, a.gn_general = 0, general
            raw.fill_(float("nan"))
            rc = nat.lib().lfvdm_conv_igemm(C.byref(a), nat.stream())
            torch.cuda.synchronize()
            assert rc != 0 and bool(torch.isnan(raw).all()) and bool(torch.isnan(act[:, :C0]).all()) and torch.equal(act[:, C0:], right)
        return
    worst = 0.0
    for code, general in [(c, g) for c in [0] + codes for g in (0, 1)]:
        a.tune, a.gn_general = code, general
        act[:, :C0].fill_(float("nan")); raw.fill_(float("nan"))
        nat.conv_igemm_struct(a)
        assert torch.equal(act[:, C0:], right), "the GEMM's epilogue must not touch the skip half's columns"
        worst = max(worst, held("fused GroupNorm", f"{case.tag} code {code} general {general}", act, ref[:, :Cc], b_gn),
                    held("fused GroupNorm", f"{case.tag} code {code} general {general} raw", raw, ref[:, Cc:], b_raw))
    assert int(keep[1].abs().sum()) == 0
    print(f"[wide] concat GroupNorm {case.tag}: {2 * (len(codes) + 1)} launches, worst max|d| / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------------
# nodes
# ------------------------------------------------------------------------------------------------------------------------
def compare(node, case, res, mode):
    for name in case.ref:
        assert res[name] is not None, f"{case.tag} {name}: no gradient"
        held(node, f"{case.tag} {mode} {name}", res[name].detach(), ref_dev(case.ref[name]).view_as(res[name]), case.bound(name))


@REDUCTION
@DELIVERY
@pytest.mark.parametrize("N,Cin,Cout,H,W,stride,up", wc.NODE_CONV_CASES)
def test_conv_node(bw, monkeypatch, N, Cin, Cout, H, W, stride, up, inplace, det):
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    case = bn.conv_case(N, Cin, Cout, H, W, stride, up)
    res = run_checked(bw, case, conv_call(bw, N, H, W, stride, up), ("w", "b"), inplace, det)
    compare("ConvFn", case, res, mode_id(inplace, det))


@REDUCTION
@DELIVERY
@pytest.mark.parametrize("C0,C1,Cout", wc.NODE_CHANNELS)
def test_resblock_node(bw, monkeypatch, C0, C1, Cout, inplace, det):
    """The node's own choice of launches at these widths, and where the FiLM and GroupNorm parameter gradients land."""
    monkeypatch.setenv("LFVDM_DETERMINISTIC", det)
    H, W = wc.NODE_MAP
    case = bn.res_case(C0, C1, Cout, H, W)
    res = run_checked(bw, case, res_call(bw, H, W), RES_PARAMS, inplace, det)
    compare("ResBlockFn", case, res, mode_id(inplace, det))
