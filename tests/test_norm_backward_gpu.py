"""Op-level fp64 parity of the GroupNorm backward kernels and of the deterministic (ordered-slab) gradient entry points.

- the small-slice spatial GroupNorm(+FiLM)(+SiLU) backward (lfvdm_gn_bwd with either destination of the sums,
  lfvdm_gn_param_grads, _stats + _apply, _apply_params) through _backward._gn_backward in its three delivery modes, at every
  channel split the models use, on both sides of the small / chunked boundary;
- temporal GroupNorm forward and backward (atomic and _det) for every kernel the dispatch can pick, up to 64 frames;
- lfvdm_rowdot_bwd_det and lfvdm_conv_wgrad with a slab (every tune code, every slab capacity class).

Every comparison prints its worst error / tolerance ratio.  GPU only."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import rnd, close, cl, hw, nsq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from improved_diffusion import _native
    _native.lib()
    return _native


def within(tag, got, want, atol, rtol=1e-4):
    """close() with the ratio max|got - want| / (atol + rtol |want|) printed first (<= 1 passes)."""
    g, w = got.detach().float().cpu(), want.detach().float().cpu()
    ratio = float(((g - w).abs() / (atol + rtol * w.abs())).max()) if g.numel() else 0.0
    print(f"[err/tol] {tag}: {ratio:.3f}")
    close(g, w, atol, rtol)


# ------------------------------------------------------------------------------------------------------------------------
# 1. small-slice spatial GroupNorm(+FiLM)(+SiLU) backward
# ------------------------------------------------------------------------------------------------------------------------
SPLITS = [(32, 0), (64, 0), (96, 0), (128, 0), (64, 32), (128, 64), (100, 28), (192, 0), (256, 0), (256, 128), (256, 256),
          (384, 0), (512, 256), (512, 512), (1024, 0)]
P_CLASSES = ["1", "3", "4", "7", "PL-1", "PL+1", "4PL+3", "64", "256", "t", "t+1"]
N_CLASSES = [(40, 20), (6, 3), (5, 1)]          # (N, T): the training shape B=2 x T=20; FiLM with T=3; odd N with T=1


def _pl(C):
    """positions per pass of the single-workgroup kernels: 256 lanes / (8 groups x C/32 channels / 4 per lane)"""
    return 256 // (2 * C // 32)


def _p_of(cls, C, t):
    PL = _pl(C)
    return {"PL-1": PL - 1, "PL+1": PL + 1, "4PL+3": 4 * PL + 3, "t": t, "t+1": t + 1}.get(cls) or int(cls)


def _small_slice_cases():
    """A pairwise covering of split x P class x (N, act, FiLM, adds).  P above the boundary t = 16 PL is kept only as t + 1
    (the first chunked size); slices with fewer than 4 elements per group are left out (ill-conditioned)."""
    cases, i = [], 0
    for si, (C0, C1) in enumerate(SPLITS):
        C = C0 + C1
        t = 16 * _pl(C)
        for cls in P_CLASSES:
            P = _p_of(cls, C, t)
            if (P > t and cls != "t+1") or P * (C // 32) < 4:
                continue
            ncls = i % 3
            N, T = N_CLASSES[ncls]
            act = (i // 3) % 2
            film = ncls == 1 or (i // 6 + si) % 2 == 0
            adds = (i + i // 3 + si) % 3
            cases.append(pytest.param(C0, C1, cls, N, T, act, film, adds, id=f"{C0}+{C1}-P{cls}-N{N}-act{act}-film{int(film)}-add{adds}"))
            i += 1
    return cases


SMALL_SLICE_CASES = _small_slice_cases()


def _boundary(nat, C, N):
    """The largest P that lfvdm_gn_bwd_ws_floats sends to the single-workgroup kernels (ws size 0)."""
    L = nat.lib()
    lo, hi = 1, 1 << 16
    assert L.lfvdm_gn_bwd_ws_floats(C, N, lo) == 0 and L.lfvdm_gn_bwd_ws_floats(C, N, hi) > 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if L.lfvdm_gn_bwd_ws_floats(C, N, mid) == 0:
            lo = mid
        else:
            hi = mid
    return lo


def test_small_slice_cases_cover_every_split_and_boundary(nat):
    """The case list reaches every split, every P class and every option at least twice, and both sides of the small /
    chunked boundary for every split; lfvdm_gn_bwd_ws_floats returns 0 at t and > 0 at t + 1 (t = 16 PL)."""
    vals = [c.values for c in SMALL_SLICE_CASES]
    for k, universe in ((0, {s[0] for s in SPLITS}), (2, set(P_CLASSES)), (3, {n for n, _ in N_CLASSES}), (5, {0, 1}),
                        (6, {False, True}), (7, {0, 1, 2})):
        for v in universe:
            assert sum(1 for row in vals if row[k] == v) >= 2, (k, v)
    for C0, C1 in SPLITS:
        C = C0 + C1
        got = {row[2] for row in vals if (row[0], row[1]) == (C0, C1)}
        assert {"t", "t+1"} <= got, (C0, C1)
        for N, _ in N_CLASSES:
            t = _boundary(nat, C, N)
            assert t == 16 * _pl(C), (C, N, t)
            assert nat.lib().lfvdm_gn_bwd_ws_floats(C, N, t) == 0 and nat.lib().lfvdm_gn_bwd_ws_floats(C, N, t + 1) > 0


def _gn_reference(a, b, C0, C1, N, P, gamma, beta, fm, T, act, da):
    """fp64 autograd of silu(group_norm(cat(a, b)) * (1 + scale) + shift) (reference nn.py:17-19, unet.py:199-203)."""
    C = C0 + C1
    xd = torch.cat([a] + ([b] if C1 else []), dim=1).double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    fd = fm.double().requires_grad_(True) if fm is not None else None
    y = F.group_norm(xd.view(N, P, C).permute(0, 2, 1), 32, gd, bd, eps=1e-5)
    if fd is not None:
        f = fd.repeat_interleave(T, dim=0)
        y = y * (1 + f[:, :C, None]) + f[:, C:, None]
    if act:
        y = F.silu(y)
    (y.permute(0, 2, 1).reshape(N * P, C) * da.double()).sum().backward()
    return xd.grad, gd.grad, bd.grad, (fd.grad if fd is not None else None)


def _rows_view(tag, M, C, pad_left=4, pad_right=4):
    """[M][C] values as a column view of a wider [M][C + 8] device buffer (row stride > C, 16-byte aligned rows)."""
    wide = rnd(tag, M, pad_left + C + pad_right).cuda()
    return wide[:, pad_left:pad_left + C]


def _film_slot(B, C, canary=1234.5):
    """A zeroed [B][2C] slot inside a wider buffer whose other elements hold a canary: (buffer, slot)."""
    buf = torch.full((B, 2 * C + 12), canary, device="cuda")
    slot = buf[:, 4:4 + 2 * C]
    slot.zero_()
    return buf, slot


def _outside_slot_untouched(buf, C, canary=1234.5):
    rest = torch.cat([buf[:, :4], buf[:, 4 + 2 * C:]], dim=1)
    return bool((rest == canary).all())


@pytest.mark.parametrize("C0,C1,pcls,N,T,act,film,adds", SMALL_SLICE_CASES)
def test_gn_backward_small_slices(nat, monkeypatch, C0, C1, pcls, N, T, act, film, adds):
    """_backward._gn_backward in the three delivery modes (atomics: lfvdm_gn_bwd; LFVDM_DETERMINISTIC=1: lfvdm_gn_bwd storing
    the sums + lfvdm_gn_param_grads; autograd: lfvdm_gn_bwd_stats + lfvdm_gn_bwd_apply) vs fp64 autograd:
    ragged position loops, idle lanes (C/32 = 3, 6, 12, 24), 4-channel vectors across group and concat boundaries, add /
    add2 rows with a stride wider than C, accumulation into preloaded .grad, the FiLM gradient in a strided slot with
    canaries.  dx is bitwise the same in the atomic and deterministic modes (same kernel) and bitwise repeatable everywhere;
    parameter / FiLM gradients are bitwise repeatable where no float atomics are involved.  On the small side of the
    boundary the raw ABI is checked as well: lfvdm_gn_bwd_apply accumulating (acc0 = acc1 = 1) and
    lfvdm_gn_bwd_apply_params (dfilm zeroed first, dgamma / dbeta / dfilm accumulated, dx per destination)."""
    from improved_diffusion import _backward as bw
    L = nat.lib()
    C = C0 + C1
    t = _boundary(nat, C, N)
    P = _p_of(pcls, C, t)
    small = L.lfvdm_gn_bwd_ws_floats(C, N, P) == 0
    assert small == (pcls != "t+1"), (P, t)
    B = N // T
    tag = f"nbs/{C0}/{C1}/{N}/{P}"
    a = rnd(tag + "/a", N * P, C0) * 1.3 + 0.7
    b = rnd(tag + "/b", N * P, C1) if C1 else None
    gamma, beta = 1 + 0.1 * rnd(tag + "/g", C), 0.1 * rnd(tag + "/be", C)
    fm = 0.3 * rnd(tag + "/film", B, 2 * C) if film else None
    da = rnd(tag + "/da", N * P, C)
    ex = [_rows_view(f"{tag}/add{i}", N * P, C) for i in range(adds)]
    dx_pure, g_ref, b_ref, f_ref = _gn_reference(a, b, C0, C1, N, P, gamma, beta, fm, T, act, da)
    dx_ref = dx_pure + sum(e.double().cpu() for e in ex) if ex else dx_pure
    tol_dx = 3e-5 * max(float(dx_ref.abs().max()), 1.0)
    tol_g, tol_b = 2e-4 * float(g_ref.abs().max()), 2e-4 * float(b_ref.abs().max())
    tol_f = 2e-4 * float(f_ref.abs().max()) if film else None

    gpar, bpar = torch.nn.Parameter(gamma.cuda()), torch.nn.Parameter(beta.cuda())
    ac, bc, dac = a.cuda(), (b.cuda() if C1 else None), da.cuda()
    fc = fm.cuda() if film else None
    _, cA, cB, st = bw._gn_apply(ac, bc, C0, C1, N, P, gpar.detach(), bpar.detach(), fc, T, act)
    g_pre, b_pre = rnd(tag + "/gpre", C).cuda(), rnd(tag + "/bpre", C).cuda()
    kw = dict(add=ex[0] if adds >= 1 else None, add2=ex[1] if adds >= 2 else None)
    dx_of = {}
    for mode in ("atomics", "deterministic", "autograd"):
        monkeypatch.setenv("LFVDM_DETERMINISTIC", "1" if mode == "deterministic" else "0")
        inplace = mode != "autograd"
        runs = []
        for _ in range(2):
            gpar.grad, bpar.grad = (g_pre.clone(), b_pre.clone()) if inplace else (None, None)
            buf, slot = _film_slot(B, C) if (film and inplace) else (None, None)
            dxa, dxb, dg, db, dfilm = bw._gn_backward(dac, ac, bc, C0, C1, N, P, cA, cB, st, act, gpar, bpar, fc, T,
                                                      dfilm_out=slot, inplace=inplace, **kw)
            if inplace:
                dg, db, dfilm = gpar.grad, bpar.grad, slot
                assert not film or _outside_slot_untouched(buf, C), f"{mode}: FiLM gradient written outside its slot"
            torch.cuda.synchronize()
            runs.append([None if v is None else v.clone() for v in (dxa, dxb, dg, db, dfilm)])
        dxa, dxb, dg, db, dfilm = runs[0]
        dx = torch.cat([dxa] + ([dxb] if C1 else []), dim=1)
        within(f"{mode} dx", dx, dx_ref, tol_dx)
        within(f"{mode} dgamma", dg, (g_ref + g_pre.double().cpu()) if inplace else g_ref, tol_g)
        within(f"{mode} dbeta", db, (b_ref + b_pre.double().cpu()) if inplace else b_ref, tol_b)
        if film:
            within(f"{mode} dfilm", dfilm, f_ref, tol_f)
        else:
            assert dfilm is None
        assert all(torch.equal(u, v) for u, v in zip(runs[0][:2], runs[1][:2]) if u is not None), f"{mode}: dx not repeatable"
        if mode != "atomics":
            assert all(torch.equal(u, v) for u, v in zip(runs[0][2:], runs[1][2:]) if u is not None), \
                f"{mode}: parameter gradients not repeatable"
        dx_of[mode] = dx
    assert torch.equal(dx_of["atomics"], dx_of["deterministic"]), "dx differs between the atomic and deterministic modes"
    if not small:
        return

    # raw ABI of the two-launch form
    ptr = nat.ptr
    sums = torch.empty(N, C, 2, device="cuda")
    nat.check(L.lfvdm_gn_bwd_stats(ptr(dac), ptr(ac), ptr(bc), C0, C1, N, P, ptr(cA), ptr(cB), ptr(st), act, ptr(sums),
                                   nat.stream()), "lfvdm_gn_bwd_stats")
    pre0, pre1 = rnd(tag + "/o0", N * P, C0), (rnd(tag + "/o1", N * P, C1) if C1 else None)
    o0, o1 = pre0.cuda(), (pre1.cuda() if C1 else None)
    nat.check(L.lfvdm_gn_bwd_apply(ptr(dac), ptr(ac), ptr(bc), C0, C1, N, P, ptr(cA), ptr(cB), ptr(st), ptr(sums), act,
                                   ptr(o0), ptr(o1), 1, 1, nat.stream()), "lfvdm_gn_bwd_apply")
    want = dx_pure + torch.cat([pre0] + ([pre1] if C1 else []), dim=1).double()
    within("apply acc0=acc1=1 dx", torch.cat([o0] + ([o1] if C1 else []), dim=1), want, 3e-5 * max(float(want.abs().max()), 1.0))
    # apply_params: out0 overwritten, out1 accumulated, `add` (strided) folded in, parameter gradients accumulated
    o0, o1 = pre0.cuda(), (pre1.cuda() if C1 else None)
    dgp, dbp = g_pre.clone(), b_pre.clone()
    buf, slot = _film_slot(B, C) if film else (None, None)
    add = ex[0] if adds >= 1 else None
    nat.check(L.lfvdm_gn_bwd_apply_params(
        ptr(dac), ptr(ac), ptr(bc), C0, C1, N, P, ptr(cA), ptr(cB), ptr(st), ptr(sums), act, ptr(o0), ptr(o1), 0, 1,
        ptr(gpar.detach()), ptr(bpar.detach()), fc.data_ptr() if film else None, fc.stride(0) if film else 0, T, ptr(dgp), ptr(dbp),
        slot.data_ptr() if film else None, slot.stride(0) if film else 0, add.data_ptr() if add is not None else None,
        add.stride(0) if add is not None else 0, nat.stream()), "lfvdm_gn_bwd_apply_params")
    want = dx_pure + (add.double().cpu() if add is not None else 0)
    if C1:
        want = want + torch.cat([torch.zeros(N * P, C0, dtype=torch.float64), pre1.double()], dim=1)
    within("apply_params dx", torch.cat([o0] + ([o1] if C1 else []), dim=1), want, 3e-5 * max(float(want.abs().max()), 1.0))
    within("apply_params dgamma", dgp, g_ref + g_pre.double().cpu(), tol_g)
    within("apply_params dbeta", dbp, b_ref + b_pre.double().cpu(), tol_b)
    if film:
        within("apply_params dfilm", slot, f_ref, tol_f)
        assert _outside_slot_untouched(buf, C), "apply_params: FiLM gradient written outside its slot"


def test_gn_backward_small_slice_refusals(nat):
    """Every single-workgroup entry point, and lfvdm_gn_bwd with either destination of the sums, refuses C % 32 != 0,
    C0 % 4 != 0, C > 1024 and (where it takes one) add_ld / add2_ld < C."""
    L, s = nat.lib(), nat.stream()
    big = torch.zeros(1 << 16, device="cuda")       # large enough for every shape below (nothing may launch anyway)
    p = big.data_ptr()
    N, P = 2, 4

    def stats(C0, C1, add_ld):
        return L.lfvdm_gn_bwd_stats(p, p, p, C0, C1, N, P, p, p, p, 1, p, s)

    def apply(C0, C1, add_ld):
        return L.lfvdm_gn_bwd_apply(p, p, p, C0, C1, N, P, p, p, p, p, 1, p, p, 0, 0, s)

    def apply_params(C0, C1, add_ld):
        return L.lfvdm_gn_bwd_apply_params(p, p, p, C0, C1, N, P, p, p, p, p, 1, p, p, 0, 0, p, p, None, 0, 1, p, p, None, 0,
                                           p, add_ld, s)

    def record(C0, C1, **kw):
        a = dict(da=p, src0=p, src1=p, coefA=p, coefB=p, stats=p, out0=p, out1=p, C0=C0, C1=C1, N=N, P=P, act=1)
        a.update(kw)
        return L.lfvdm_gn_bwd(C.byref(nat.GnBwdArgs(**a)), s)

    atomics = dict(gamma=p, beta=p, dgamma=p, dbeta=p)

    def fused(C0, C1, add_ld):
        return record(C0, C1, **atomics, add=p, add_ld=add_ld)

    def fused_add2(C0, C1, add_ld):
        return record(C0, C1, **atomics, add2=p, add2_ld=add_ld)

    def fused_sums(C0, C1, add_ld):
        return record(C0, C1, sums_out=p, add=p, add_ld=add_ld)

    def fused_sums_add2(C0, C1, add_ld):
        return record(C0, C1, sums_out=p, add2=p, add2_ld=add_ld)

    takes_add = (apply_params, fused, fused_add2, fused_sums, fused_sums_add2)
    for fn in (stats, apply) + takes_add:
        bad = [(48, 0), (30, 2), (1056, 0), (1024, 32)]
        for C0, C1 in bad:
            assert fn(C0, C1, 2048) != 0, (fn.__name__, C0, C1)
        assert fn(64, 32, 96) == 0, fn.__name__              # the same call with a valid shape is accepted
        if fn in takes_add:
            assert fn(64, 32, 92) != 0, (fn.__name__, "add_ld < C")
    # the record's own refusals: the sums go to exactly one destination; a chunked map needs its whole workspace and N
    # within the grid's z dimension
    assert record(64, 32) != 0, "neither destination"
    assert record(64, 32, sums_out=p, **atomics) != 0, "both destinations"
    Pc = 16 * _pl(96) + 1
    need = L.lfvdm_gn_bwd_ws_floats(96, N, Pc)
    assert need > 0
    assert record(64, 32, P=Pc, sums_out=p, ws=None, ws_floats=need) != 0, "chunked map without a workspace"
    assert record(64, 32, P=Pc, sums_out=p, ws=p, ws_floats=need - 1) != 0, "chunked map with a short workspace"
    assert record(64, 32, N=65536, P=Pc, sums_out=p, ws=p, ws_floats=L.lfvdm_gn_bwd_ws_floats(96, 65536, Pc)) != 0, "N = 65536, chunked"
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# 2. temporal GroupNorm, forward and backward, every kernel
# ------------------------------------------------------------------------------------------------------------------------
def _gnt_target(T, C):
    """The kernel lfvdm_gn_temporal and gn_temporal_bwd_impl pick: register kernels <8> / <16> / <32> when the channel
    quads of a frame divide a wave (per_lane = frames per lane), else the general kernel."""
    Q = C // 4
    if Q <= 64 and 64 % Q == 0:
        per_lane = -(-T // (64 // Q))
        for n in (8, 16, 32):
            if per_lane <= n:
                return f"reg{n}"
    return "general"


GNT_SHAPES = [(1, 64, 7, 32), (2, 33, 4, 64), (2, 20, 16, 128), (1, 64, 3, 128), (3, 57, 5, 128), (1, 17, 6, 256),
              (2, 40, 5, 256), (1, 64, 2, 256), (2, 64, 3, 96), (1, 48, 3, 512), (2, 2, 3, 256)]


def test_temporal_shapes_reach_every_kernel():
    assert {_gnt_target(T, C) for _, T, _, C in GNT_SHAPES} == {"reg8", "reg16", "reg32", "general"}


def _gnt_columns(x, B, T, P, C):
    return x.double().view(B, T, P, C).permute(0, 2, 3, 1).reshape(B * P, C, T)


def _gnt_rows(y, B, T, P, C):
    return y.view(B, P, C, T).permute(0, 3, 1, 2).reshape(B * T * P, C)


@pytest.mark.parametrize("B,T,P,C", GNT_SHAPES, ids=[f"{b}-{t}-{p}-{c}-{_gnt_target(t, c)}" for b, t, p, c in GNT_SHAPES])
def test_gn_temporal_forward(nat, B, T, P, C):
    """lfvdm_gn_temporal (rpe.py:135-136) vs fp64 group_norm over the (b, pixel) columns; bitwise repeatable."""
    x = (rnd("gtf/x", B * T * P, C) * 1.2 + 0.3).cuda()
    gamma, beta = (1 + 0.1 * rnd("gtf/g", C)).cuda(), (0.1 * rnd("gtf/b", C)).cuda()
    ref = _gnt_rows(F.group_norm(_gnt_columns(x.cpu(), B, T, P, C), 32, gamma.double().cpu(), beta.double().cpu(), 1e-5), B, T, P, C)
    ys = []
    for _ in range(2):
        y = torch.full((B * T * P, C), float("nan"), device="cuda")
        nat.check(nat.lib().lfvdm_gn_temporal(nat.ptr(x), nat.ptr(gamma), nat.ptr(beta), 1e-5, nat.ptr(y), B, T, P, C, nat.stream()),
                  "lfvdm_gn_temporal")
        ys.append(y)
    within("gn_temporal y", ys[0], ref, 1e-5)
    assert torch.equal(ys[0], ys[1])


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("B,T,P,C", GNT_SHAPES, ids=[f"{b}-{t}-{p}-{c}-{_gnt_target(t, c)}" for b, t, p, c in GNT_SHAPES])
def test_gn_temporal_backward_every_kernel(nat, B, T, P, C, accumulate):
    """lfvdm_gn_temporal_bwd and lfvdm_gn_temporal_bwd_det vs fp64 autograd: dx written or accumulated, dgamma / dbeta
    accumulated onto preloaded values.  The _det form takes a workspace of exactly 2 ceil(B P / 4) C floats (the floats
    behind it stay untouched), is bitwise repeatable, and refuses one float less without touching dx / dgamma / dbeta."""
    L = nat.lib()
    tag = f"gtk/{B}/{T}/{P}/{C}"
    x, dy = rnd(tag + "/x", B * T * P, C) * 1.2 + 0.3, rnd(tag + "/dy", B * T * P, C)
    gamma = 1 + 0.1 * rnd(tag + "/g", C)
    xr = _gnt_columns(x, B, T, P, C).requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.group_norm(xr, 32, gr, br, eps=1e-5).backward(_gnt_columns(dy, B, T, P, C))
    dx0, g0, b0 = rnd(tag + "/dx0", B * T * P, C), rnd(tag + "/g0", C), rnd(tag + "/b0", C)
    want_dx = _gnt_rows(xr.grad, B, T, P, C) + (dx0.double() if accumulate else 0)
    want_g, want_b = gr.grad + g0.double(), br.grad + b0.double()
    tol_g, tol_b = 1e-4 * max(1.0, float(gr.grad.abs().max())), 1e-4 * max(1.0, float(br.grad.abs().max()))
    xc, dyc, gc = x.cuda(), dy.cuda(), gamma.cuda()
    need = 2 * (-(-(B * P) // 4)) * C
    guard = 256
    ws = torch.full((need + guard,), float("nan"), device="cuda")

    def run(det, ws_floats=need):
        dx, dg, db = dx0.cuda(), g0.cuda(), b0.cuda()
        args = (nat.ptr(xc), nat.ptr(dyc), nat.ptr(gc), 1e-5, nat.ptr(dx), nat.ptr(dg), nat.ptr(db), B, T, P, C, accumulate)
        rc = (L.lfvdm_gn_temporal_bwd_det(*args, ws.data_ptr(), ws_floats, nat.stream()) if det
              else L.lfvdm_gn_temporal_bwd(*args, nat.stream()))
        torch.cuda.synchronize()
        return rc, dx, dg, db

    for det in (0, 1):
        rc, dx, dg, db = run(det)
        nat.check(rc, "lfvdm_gn_temporal_bwd" + ("_det" if det else ""))
        name = "det" if det else "atomic"
        within(f"{name} dx", dx, want_dx, 5e-5)
        within(f"{name} dgamma", dg, want_g, tol_g)
        within(f"{name} dbeta", db, want_b, tol_b)
    assert bool(torch.isnan(ws[need:]).all()), "the _det form wrote past its workspace"
    r1, r2 = run(1)[1:], run(1)[1:]
    assert all(torch.equal(u, v) for u, v in zip(r1, r2)), "the _det form is not bitwise repeatable"
    rc, dx, dg, db = run(1, need - 1)
    assert rc != 0, "one float less of workspace must be refused"
    assert torch.equal(dx.cpu(), dx0) and torch.equal(dg.cpu(), g0) and torch.equal(db.cpu(), b0), "a refused call wrote"


def test_gn_temporal_refusals(nat):
    """Channel counts the temporal GroupNorm kernels do not cover are refused (C = 0 included)."""
    L, s = nat.lib(), nat.stream()
    buf = torch.zeros(1 << 16, device="cuda")
    p = buf.data_ptr()
    for C in (0, 48, 544, 1024):
        assert L.lfvdm_gn_temporal(p, p, p, 1e-5, p, 1, 2, 2, C, s) != 0, C
        assert L.lfvdm_gn_temporal_bwd(p, p, p, 1e-5, p, p, p, 1, 2, 2, C, 0, s) != 0, C
        assert L.lfvdm_gn_temporal_bwd_det(p, p, p, 1e-5, p, p, p, 1, 2, 2, C, 0, p, 1 << 16, s) != 0, C
    assert L.lfvdm_gn_temporal_bwd_det(p, p, p, 1e-5, p, p, p, 1, 2, 2, 64, 0, None, 0, s) != 0, "no workspace"
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# 3. remaining deterministic slabs
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(3, 256), (2, 1024), (6, 512)])
def test_rowdot_backward_deterministic(nat, M, K):
    """lfvdm_rowdot_bwd_det with the two jobs of test_rowdot_backward, both `din` arrays carved from one preloaded flat
    buffer (din_base, din_n): a workspace of exactly total_tasks * din_n floats, fp64 parity, bitwise repeatable, untouched
    gap between the arrays and floats behind the workspace; one float less is refused; din_base = NULL (no job has a din)."""
    L = nat.lib()
    x = rnd("rb/x", M, K)
    Ws = [0.1 * rnd("rb/w0", 96, K), 0.1 * rnd("rb/w1", 40, K)]
    douts = [rnd("rb/d0", M, 96), rnd("rb/d1", M, 40)]
    xr = x.double().requires_grad_(True)
    wr = [w.double().requires_grad_(True) for w in Ws]
    act = F.silu(xr)
    act.retain_grad()
    y0, y1 = act @ wr[0].t(), xr @ wr[1].t()
    (y0 * douts[0].double()).sum().backward(retain_graph=True, inputs=[act, wr[0]])
    g_act = act.grad.clone()
    (y1 * douts[1].double()).sum().backward(inputs=[xr, wr[1]])
    dev = lambda t: t.cuda().contiguous()
    xd, Wd, dd = dev(x), [dev(w) for w in Ws], [dev(d) for d in douts]
    gap = 32
    din_n = 2 * M * K + 2 * gap
    flat0 = rnd("rbd/flat", din_n)
    flat = flat0.cuda()
    din = [flat[gap:gap + M * K].view(M, K), flat[2 * gap + M * K:2 * gap + 2 * M * K].view(M, K)]
    dW = [torch.zeros_like(w) for w in Wd]
    db = [torch.zeros(w.shape[0], device="cuda") for w in Wd]
    tasks = 12 + 5

    def jobs(with_din):
        return nat.jobs_to_device([
            nat.RowdotBwdJob(Wd[0].data_ptr(), xd.data_ptr(), dd[0].data_ptr(), dW[0].data_ptr(), db[0].data_ptr(),
                             din[0].data_ptr() if with_din else None, K, 96, M, K, 96, K, 1, 0),
            nat.RowdotBwdJob(Wd[1].data_ptr(), xd.data_ptr(), dd[1].data_ptr(), dW[1].data_ptr(), db[1].data_ptr(),
                             din[1].data_ptr() if with_din else None, K, 40, M, K, 40, K, 0, 12)], "cuda")

    need = tasks * din_n
    ws = torch.full((need + 256,), float("nan"), device="cuda")
    table = jobs(True)

    def run(ws_floats=need, with_din=True):
        for t in dW + db:
            t.zero_()
        flat.copy_(flat0)
        tb = table if with_din else jobs(False)
        rc = L.lfvdm_rowdot_bwd_det(tb.data_ptr(), 2, tasks, flat.data_ptr() if with_din else None, din_n if with_din else 0,
                                    ws.data_ptr() if with_din else None, ws_floats if with_din else 0, nat.stream())
        torch.cuda.synchronize()
        return rc, [t.clone() for t in dW + db + [flat]]

    rc, r1 = run()
    nat.check(rc, "lfvdm_rowdot_bwd_det")
    within("rowdot det dW0", r1[0], wr[0].grad, 2e-5)
    within("rowdot det dW1", r1[1], wr[1].grad, 2e-5)
    within("rowdot det db0", r1[2], douts[0].sum(0), 1e-5)
    within("rowdot det db1", r1[3], douts[1].sum(0), 1e-5)
    f = r1[4].cpu()
    within("rowdot det din0", f[gap:gap + M * K].view(M, K), flat0[gap:gap + M * K].view(M, K).double() + g_act, 2e-5)
    within("rowdot det din1", f[2 * gap + M * K:2 * gap + 2 * M * K].view(M, K),
           flat0[2 * gap + M * K:2 * gap + 2 * M * K].view(M, K).double() + xr.grad, 2e-5)
    assert torch.equal(f[:gap], flat0[:gap]) and torch.equal(f[gap + M * K:2 * gap + M * K], flat0[gap + M * K:2 * gap + M * K]) \
        and torch.equal(f[2 * gap + 2 * M * K:], flat0[2 * gap + 2 * M * K:]), "elements of din_base outside the arrays changed"
    assert bool(torch.isnan(ws[need:]).all()), "wrote past the workspace"
    _, r2 = run()
    assert all(torch.equal(u, v) for u, v in zip(r1, r2)), "not bitwise repeatable"
    rc, r3 = run(need - 1)
    assert rc != 0, "one float less of workspace must be refused"
    assert all(float(t.abs().max()) == 0.0 for t in r3[:4]) and torch.equal(r3[4].cpu(), flat0), "a refused call wrote"
    rc, r4 = run(with_din=False)
    nat.check(rc, "lfvdm_rowdot_bwd_det (din_base = NULL)")
    within("rowdot det (no din) dW0", r4[0], wr[0].grad, 2e-5)
    within("rowdot det (no din) dW1", r4[1], wr[1].grad, 2e-5)
    within("rowdot det (no din) db0", r4[2], douts[0].sum(0), 1e-5)
    within("rowdot det (no din) db1", r4[3], douts[1].sum(0), 1e-5)
    assert torch.equal(r4[4].cpu(), flat0)


@pytest.mark.parametrize("N,C0,C1,Cout,H,k", [(10, 128, 0, 128, 16, 3), (3, 128, 128, 256, 8, 3), (4, 256, 0, 128, 8, 1),
                                              nsq(13, 128, 0, 64, (1, 3), 3), (3, 64, 0, 32, 8, 3)])
def test_conv_wgrad_deterministic_every_tune_code(nat, N, C0, C1, Cout, H, k):
    """lfvdm_conv_wgrad with a slab (splitk_ws) for the heuristic and every code of _native._wgrad_codes - every tile, stage
    form and M-slice count, not only the tap-fused kernels - at four capacities: ample, exactly one slice (per = Cout k^2 Cin
    + Cout), 2 per - 1 and 3 per - 1 (det_fit must cut the slice count to one / two).  Each run is bitwise repeatable,
    within 2e-5 of autograd and leaves the floats behind the capacity alone; per - 1 is refused without a write.  The last
    shape (Cout = 32) has no tune codes: the wave-private kernel."""
    Cin = C0 + C1
    H, W = hw(H)
    x = rnd("wgc/x", N, Cin, H, W)
    w = (rnd("wgc/w", Cout, Cin, k, k, scale=0.05)).requires_grad_(True)
    b = rnd("wgc/b", Cout).requires_grad_(True)
    y = F.conv2d(x, w, b, padding=1 if k == 3 else 0)
    dout = rnd("wgc/d", N, Cout, H, W)
    y.backward(dout)
    gp = torch.zeros(Cout, k * k, Cin, device="cuda")
    db = torch.zeros(Cout, device="cuda")
    keep = dict(src0=cl(x[:, :C0]), res=cl(dout))
    if C1:
        keep["src1"] = cl(x[:, C0:])
    a = nat.fill_conv_args(C0=C0, C1=C1, N=N, Hs=H, Ws=W, Ho=H, Wo=W, ksize=k, ldr=Cout, out=gp, bias=db, Cout=Cout, **keep)
    codes = nat._wgrad_codes(a)
    if Cout >= 64:
        assert {((c - 1) >> 2) & 3 for c in codes} >= {1, 2, 3}, "every stage form (non-tap-fused kernels) is exercised"
    else:
        assert codes == []
    per = Cout * k * k * Cin + Cout
    scale = max(1.0, float(w.grad.abs().max()))
    bscale = max(1.0, float(b.grad.abs().max()))
    ample = torch.empty(64 << 20, device="cuda")
    guard = 256
    worst = 0.0
    for code in [0] + codes:
        a.tune = code
        for cap in (None, per, 2 * per - 1, 3 * per - 1):
            ws = ample if cap is None else torch.full((cap + guard,), float("nan"), device="cuda")
            a.splitk_ws, a.splitk_ws_floats = ws.data_ptr(), (ws.numel() if cap is None else cap)
            runs = []
            for _ in range(2):
                gp.zero_(); db.zero_()
                nat.check(nat.lib().lfvdm_conv_wgrad(C.byref(a), nat.stream()), f"lfvdm_conv_wgrad code {code} cap {cap}")
                torch.cuda.synchronize()
                runs.append((gp.clone(), db.clone()))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"code {code} cap {cap}: not reproducible"
            got_w = gp.view(Cout, k, k, Cin).permute(0, 3, 1, 2).cpu()
            err_w = float((got_w - w.grad).abs().max()) / (2e-5 * scale)
            err_b = float((db.cpu() - b.grad).abs().max()) / (2e-5 * bscale)
            worst = max(worst, err_w, err_b)
            assert err_w < 1, f"code {code} cap {cap}: dW err/tol = {err_w:.3f}"
            assert err_b < 1, f"code {code} cap {cap}: db err/tol = {err_b:.3f}"
            if cap is not None:
                assert bool(torch.isnan(ws[cap:]).all()), f"code {code} cap {cap}: wrote past the slab"
        ws = torch.full((per - 1 + guard,), float("nan"), device="cuda")
        a.splitk_ws, a.splitk_ws_floats = ws.data_ptr(), per - 1
        gp.zero_(); db.zero_()
        assert nat.lib().lfvdm_conv_wgrad(C.byref(a), nat.stream()) != 0, f"code {code}: a slab below one slice must be refused"
        torch.cuda.synchronize()
        assert float(gp.abs().max()) == 0.0 and float(db.abs().max()) == 0.0 and bool(torch.isnan(ws).all()), f"code {code}: refused call wrote"
    print(f"[err/tol] conv_wgrad det {len(codes) + 1} codes: {worst:.3f}")
