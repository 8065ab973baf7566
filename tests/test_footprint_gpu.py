"""Footprint tests of the tiled kernels: every operand of a launch sits between NaN / 1e30 / sentinel guard bands inside
one allocation (test_footprint_cpu.footprint), at shapes where some dimension overhangs a tile, and the launch must (a) leave
every band, padding column and input word alone, (b) give bit-identical results whatever the bands hold, (c) still meet the
op's existing reference at the existing test's tolerance.  The case lists and the proof that the harness rejects a wrong tail
predicate are in test_footprint_cpu.  No test provokes a fault: an overrun of up to two row tiles lands in a band.

Every reference and tolerance is an existing test's, named where the case's check is written; none is new.  GPU only."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import test_footprint_cpu as fp
from test_footprint_cpu import footprint, inp, outp, close64
from test_ops_gpu import nat, rnd, close, packed, _temporal_core_f64  # noqa: F401  (nat: the module fixture)
from test_norm_backward_gpu import _gn_reference
from test_rpe_grouped_gpu import _case as rpe_case, DET_LD
from test_dyn_threshold_gpu import check_against_host, make_input, masks_for
from test_train_glue_cpu import bits, same_bits, SENT, NAN
from oracle import recipe, unet_oracle as uo

pytestmark = pytest.mark.gpu

LAUNCHES = {}                   # family -> (entry, case, tune code) launches, one per fill counted once


def counted(family, n=1):
    LAUNCHES[family] = LAUNCHES.get(family, 0) + n


@pytest.fixture(scope="module", autouse=True)
def _launch_report():
    """Prints (with -s) how many (entry, case, tune code) launches each family ran; asserts nothing."""
    yield
    print("\nfootprint launches (entry, case, tune code) per family:", dict(sorted(LAUNCHES.items())))


def rows(x):
    """NCHW -> channels-last rows [N*H*W][C] on the host."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def ids(cases):
    return ["-".join(str(v) for k, v in c.items() if k != "entry" and not isinstance(v, dict)) for c in cases]


# ------------------------------------------------------------------------------------------------------------------------
# 1. implicit-GEMM convolution: every tune code of every case
# ------------------------------------------------------------------------------------------------------------------------
def _conv_problem(nat, c):
    """-> (inputs, outputs, fill(a, t): the lfvdm_conv_args from embedded operands, check)."""
    N, Hs, Ws, Ho, Wo, C0, C1, Cout, k, up = (c[x] for x in ("N", "Hs", "Ws", "Ho", "Wo", "C0", "C1", "Cout", "k", "up"))
    Cin, M, tag = C0 + C1, N * Ho * Wo, "fp/conv/" + c["name"]
    x, w, b = rnd(tag + "/x", N, Cin, Hs, Ws), rnd(tag + "/w", Cout, Cin, k, k, scale=0.05), rnd(tag + "/b", Cout)
    if up in (1, 3):
        xin = F.interpolate(x.double(), scale_factor=2, mode="nearest")
    elif up == 2:
        xin = torch.zeros(N, Cin, Ho, Wo, dtype=torch.float64)
        xin[:, :, ::2, ::2] = x.double()
    else:
        xin = x.double()
    ref = F.conv2d(xin, w.double(), b.double(), padding=1 if k == 3 else 0, stride=c["stride"])
    assert tuple(ref.shape[2:]) == (Ho, Wo)
    wp = packed4(nat, w) if up == 3 else w.permute(0, 2, 3, 1).reshape(Cout, k * k * Cin)      # == lfvdm_pack_conv_weight, bit for bit
    ins = dict(src0=inp(rows(x[:, :C0])), W=inp(wp), bias=inp(b))
    if C1:
        ins["src1"] = inp(rows(x[:, C0:]))
    ldo, ldr = c.get("ldo", Cout), c.get("ldr", Cout)
    if "s2" in c:
        S0, S1 = c["s2"]
        s, w2, b2 = rnd(tag + "/s", N, S0 + S1, Ho, Wo), rnd(tag + "/w2", Cout, S0 + S1, scale=0.05), rnd(tag + "/b2", Cout)
        ref = ref + F.conv2d(s.double(), w2.double().view(Cout, S0 + S1, 1, 1), b2.double())
        ins.update(s2src0=inp(rows(s[:, :S0])), s2src1=inp(rows(s[:, S0:])), W2=inp(w2), bias2=inp(b2))
    if "res" in c:
        r, rA, rB = rnd(tag + "/r", N, Cout, Ho, Wo), 1 + 0.2 * rnd(tag + "/rA", N, Cout), 0.2 * rnd(tag + "/rB", N, Cout)
        ref = ref + r.double() * rA.double()[:, :, None, None] + rB.double()[:, :, None, None]
        ins.update(res=inp(rows(r), ld=ldr), resA=inp(rA), resB=inp(rB))
    gn = c.get("gn")
    outs = {}
    if c.get("nchw"):
        outs["out"] = outp(N * Cout, Ho * Wo)
        want = {"out": ref.reshape(N * Cout, Ho * Wo)}
    else:
        outs["out"] = outp(M, Cout, ld=ldo, untouched=bool(gn and gn["skip_raw"]))
        want = {"out": rows(ref)}
    if gn:
        gamma, beta = 1 + 0.1 * rnd(tag + "/g", Cout), 0.1 * rnd(tag + "/be", Cout)
        g = F.group_norm(ref, 32, gamma.double(), beta.double(), eps=1e-5)
        ins.update(gn_gamma=inp(gamma), gn_beta=inp(beta))
        if gn["film"]:
            fm = 0.3 * rnd(tag + "/film", N, 2 * Cout)
            g = g * (1 + fm.double()[:, :Cout, None, None]) + fm.double()[:, Cout:, None, None]
            ins["gn_film"] = inp(fm, ld=2 * Cout + gn["film_pad"])
        want["gn_out"] = rows(F.silu(g))
        outs["gn_out"] = outp(M, Cout, ld=gn["gn_ld"])
    if c.get("splitk"):
        outs["splitk_ws"] = outp(2048, 128, scratch=True)
        outs["splitk_cnt"] = outp(8, 128, zero=True, ints=True)

    def fill(a, t):
        for name in ("src0", "src1", "W", "bias", "s2src0", "s2src1", "W2", "bias2", "res", "resA", "resB", "out", "gn_gamma",
                     "gn_beta", "gn_film", "gn_out", "splitk_ws", "splitk_cnt"):
            setattr(a, name, t[name].ptr if name in t else None)
        a.C0, a.C1, a.N, a.Hs, a.Ws, a.up, a.stride, a.ksize, a.Ho, a.Wo, a.Cout = C0, C1, N, Hs, Ws, up, c["stride"], k, Ho, Wo, Cout
        a.s2C0, a.s2C1 = c.get("s2", (0, 0))
        a.ldr, a.ldo, a.out_mode = ldr, ldo, nat.OUT_NCHW if c.get("nchw") else nat.OUT_ROWS
        if gn:
            a.gn_film_ld = 2 * Cout + gn["film_pad"] if gn["film"] else 0
            a.gn_film_div, a.gn_act, a.gn_skip_raw, a.gn_eps = 1, nat.ACT_SILU, gn["skip_raw"], 1e-5
            a.gn_general, a.gn_ld = gn.get("general", 0), gn["gn_ld"]
        if c.get("splitk"):
            a.splitk_ws_floats, a.splitk_cnt_ints = 2048 * 128, 8 * 128

    def check(o, fill_):
        if "out" in o:
            if up == 3:
                close64(o["out"], want["out"], 2e-5, 1e-4)
            else:
                close64(o["out"], want["out"], 5e-5, 0.0)
        if gn:
            close64(o["gn_out"], want["gn_out"], 1e-4, 0.0)

    return ins, outs, fill, check


def packed4(nat, w):
    o = torch.empty(4, w.shape[0], 4, w.shape[1], device="cuda")
    nat.pack_conv_weight_up2x(w.cuda().contiguous(), o)
    return o.cpu().reshape(4 * w.shape[0], 4 * w.shape[1])


@pytest.mark.parametrize("c", fp.CONV_CASES, ids=[c["name"] for c in fp.CONV_CASES])
def test_conv_igemm_footprint(nat, c):
    ins, outs, fill, check = _conv_problem(nat, c)
    L = nat.lib()
    probe = {k: fp.Embedded(op, SENT, "cuda") for k, op in {**ins, **outs}.items()}
    a = nat.ConvArgs()
    fill(a, probe)
    codes = (C.c_int * 256)()
    n = L.lfvdm_conv_igemm_candidates(C.byref(a), codes, 256)
    assert n > 0, "no launch code offered"
    todo = [0] + [codes[i] for i in range(n)]
    if c.get("splitk"):
        todo = [code for code in todo if code > 0 and ((code - 1) >> 5) & 7][:2]
        assert todo, "split-K candidates expected for a small-M layer with a workspace"

    for code in todo:
        def launch(t, code=code):
            a = nat.ConvArgs()
            fill(a, t)
            a.tune = code
            nat.check(L.lfvdm_conv_igemm(C.byref(a), nat.stream()), f"lfvdm_conv_igemm (tune {code})")
        footprint(f"lfvdm_conv_igemm[{c['name']}, tune {code}]", launch, ins, outs, check, device="cuda")
        counted("conv")


# ------------------------------------------------------------------------------------------------------------------------
# 2. GroupNorm forward
# ------------------------------------------------------------------------------------------------------------------------
def _gn_ref(x, N, P, Cc, groups, gamma, beta, fm, act):
    xr = x.double().view(N, P, Cc).permute(0, 2, 1)
    ref = F.group_norm(xr, groups, gamma.double(), beta.double(), eps=1e-5)
    if fm is not None:
        ref = ref * (1 + fm.double()[:, :Cc, None]) + fm.double()[:, Cc:, None]
    if act:
        ref = F.silu(ref)
    return ref.permute(0, 2, 1).reshape(N * P, Cc), xr


@pytest.mark.parametrize("c", fp.GN_CASES, ids=ids(fp.GN_CASES))
def test_groupnorm_forward_footprint(nat, c):
    L, e = nat.lib(), c["entry"]
    N, P, C0, C1 = c["N"], c["P"], c["C0"], c["C1"]
    Cc, tag = C0 + C1, f"fp/gn/{e}/{P}"
    gamma, beta = 1 + 0.1 * rnd(tag + "/g", Cc), 0.1 * rnd(tag + "/be", Cc)
    if e == "lfvdm_gn_temporal":
        B, T = N, c["T"]
        x = rnd(tag + f"/x{T}", B * T * P, Cc) * 1.3 + 0.25
        xc = x.view(B, T, P, Cc).permute(0, 2, 3, 1).reshape(B * P, Cc, T).double()
        want = F.group_norm(xc, 32, gamma.double(), beta.double(), 1e-5).view(B, P, Cc, T).permute(0, 3, 1, 2).reshape(-1, Cc)
        ins, outs = dict(x=inp(x), gamma=inp(gamma), beta=inp(beta)), dict(y=outp(B * T * P, Cc))
        launch = lambda t: nat.check(L.lfvdm_gn_temporal(t["x"].ptr, t["gamma"].ptr, t["beta"].ptr, 1e-5, t["y"].ptr, B, T, P, Cc,
                                                         nat.stream()), e)
        footprint(e, launch, ins, outs, lambda o, f: close(o["y"], want, 1e-5), device="cuda")
        return counted("gn")
    a = rnd(tag + "/a", N * P, C0) * 1.3 + 0.2
    ins = dict(src0=inp(a), gamma=inp(gamma), beta=inp(beta))
    if e == "lfvdm_gn_apply_part":
        want, _ = _gn_ref(a, N, P, C0, C0 // c["cg"], gamma, beta, None, c["act"])
        outs = dict(out=outp(N * P, C0, ld=c["ldo"]))
        launch = lambda t: nat.check(L.lfvdm_gn_apply_part(t["src0"].ptr, C0, N, P, c["cg"], t["gamma"].ptr, t["beta"].ptr, 1e-5, c["act"],
                                                           t["out"].ptr, c["ldo"], nat.stream()), e)
        footprint(e, launch, ins, outs, lambda o, f: close64(o["out"], want, 1e-4, 0.0), device="cuda")
        return counted("gn")
    b = rnd(tag + "/b", N * P, C1) if C1 else None
    if C1:
        ins["src1"] = inp(b)
    fm = 0.3 * rnd(tag + "/film", N, 2 * Cc)
    film_ld = 2 * Cc + c["film_pad"]
    ins["film"] = inp(fm, ld=film_ld)
    act = c.get("act", 0)
    want, xr = _gn_ref(torch.cat([a] + ([b] if C1 else []), 1), N, P, Cc, 32, gamma, beta, fm, act)
    mean = xr.reshape(N, 32, -1).mean(-1)
    outs = dict(coefA=outp(N, Cc), coefB=outp(N, Cc))
    if e != "lfvdm_gn_coef":
        outs["stats"] = outp(N, 64)
    if "apply" in e:
        outs["out"] = outp(N * P, Cc)
    need = int(L.lfvdm_gn_apply_ws_floats(Cc, N, P)) if e == "lfvdm_gn_apply_ws" else 0
    if e == "lfvdm_gn_apply_ws":
        assert need > 0
        outs["ws"] = outp(need // 64, 64, scratch=True) if need % 64 == 0 else outp(1, need, scratch=True)

    def launch(t):
        head = (t["src0"].ptr, t["src1"].ptr if C1 else None, C0, C1, N, P, t["gamma"].ptr, t["beta"].ptr, t["film"].ptr, 1, film_ld, 1e-5)
        if e == "lfvdm_gn_coef":
            rc = L.lfvdm_gn_coef(*head, t["coefA"].ptr, t["coefB"].ptr, nat.stream())
        elif e == "lfvdm_gn_coef_stats":
            rc = L.lfvdm_gn_coef_stats(*head, t["coefA"].ptr, t["coefB"].ptr, t["stats"].ptr, nat.stream())
        elif e == "lfvdm_gn_apply":
            rc = L.lfvdm_gn_apply(*head, act, t["out"].ptr, t["coefA"].ptr, t["coefB"].ptr, t["stats"].ptr, nat.stream())
        else:
            rc = L.lfvdm_gn_apply_ws(*head, act, t["out"].ptr, t["coefA"].ptr, t["coefB"].ptr, t["stats"].ptr, t["ws"].ptr, need, nat.stream())
        nat.check(rc, e)

    def check(o, f):
        if "out" in o:
            close(o["out"], want.float(), 3e-5)
        if "stats" in o:
            close(o["stats"].view(N, 32, 2)[..., 0], mean.float(), 1e-5)
        pre = (xr.permute(0, 2, 1) * o["coefA"].double()[:, None, :] + o["coefB"].double()[:, None, :]).reshape(N * P, Cc)
        close(F.silu(pre) if act else pre, want.float(), 5e-5)

    footprint(e, launch, ins, outs, check, device="cuda")
    counted("gn")


# ------------------------------------------------------------------------------------------------------------------------
# 3. attention cores
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fp.ATTN_SPATIAL_CASES, ids=ids(fp.ATTN_SPATIAL_CASES))
def test_spatial_attention_footprint(nat, c):
    L, e = nat.lib(), c["entry"]
    N, P, Cc, heads = c["N"], c["P"], c["C"], c["heads"]
    Fh, M = Cc // heads, N * P
    if e == "lfvdm_attn_spatial":
        qkv = rnd(f"fp/as/{P}", N, P, 3 * Cc)
        q, k, v = (qkv.double().view(N, P, 3, heads, Fh)[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        logits = (q * Fh ** -0.5) @ k.transpose(-1, -2)
        attn = torch.softmax(logits, -1)
        want = dict(o=(attn @ v).permute(0, 2, 1, 3).reshape(M, Cc), attn=attn.reshape(-1, P), lse=torch.logsumexp(logits, -1).reshape(-1, P))
        ins = dict(qkv=inp(qkv.view(M, 3 * Cc)))
        outs = dict(o=outp(M, Cc), attn=outp(N * heads * P, P), lse=outp(N * heads, P))
        launch = lambda t: nat.check(L.lfvdm_attn_spatial(t["qkv"].ptr, t["o"].ptr, t["attn"].ptr, t["lse"].ptr, N, P, Cc, heads,
                                                          nat.stream()), e)

        def check(o, f):
            close(o["o"], want["o"], 2e-5)
            close(o["attn"], want["attn"], 1e-5)
            close(o["lse"], want["lse"], 2e-5)
    else:
        assert L.lfvdm_attn_spatial_fused_ok(N, P, Cc, heads) == 0
        xn = rnd(f"fp/asf/{P}", M, Cc)
        W, bias = rnd("fp/asf/w", 3 * Cc, Cc) * Cc ** -0.5, 0.1 * rnd("fp/asf/b", 3 * Cc)
        qkv, two = torch.empty(M, 3 * Cc, device="cuda"), torch.empty(M, Cc, device="cuda")      # the two-launch form
        nat.conv_igemm(src0=xn.cuda(), C0=Cc, N=N, Hs=P, Ws=1, Ho=P, Wo=1, ksize=1, W=W.cuda(), bias=bias.cuda(), Cout=3 * Cc, out=qkv,
                       ldo=3 * Cc)
        nat.attn_spatial(qkv, two, None, N, P, Cc, heads)
        two = two.cpu()
        ins, outs = dict(xn=inp(xn), W=inp(W), bias=inp(bias)), dict(o=outp(M, Cc))
        launch = lambda t: nat.check(L.lfvdm_attn_spatial_fused(t["xn"].ptr, t["W"].ptr, t["bias"].ptr, t["o"].ptr, N, P, Cc, heads,
                                                                nat.stream()), e)
        check = lambda o, f: close(o["o"], two, 2e-5)
    footprint(e, launch, ins, outs, check, device="cuda")
    counted("attn_spatial")


def _temporal_probs_f64(qkv, Rq, Rk, mask, B, T, P, Cc, heads):
    """The softmax of test_ops_gpu._temporal_core_f64 (same logits, same mask), returned: rows [B*P*heads*T][T]."""
    Fh = Cc // heads
    scale = Fh ** -0.5
    x = qkv.view(B, T, P, 3, heads, Fh).permute(3, 0, 2, 4, 1, 5)
    q, k = x[0] * scale, x[1]
    logits = q @ k.transpose(-1, -2)
    logits = logits + torch.einsum("bdhtf,btshf->bdhts", q, Rk.view(B, T, T, heads, Fh))
    logits = logits + torch.einsum("bdhtf,btshf->bdhts", k * scale, Rq.view(B, T, T, heads, Fh)).transpose(-1, -2)
    m = mask.view(B, T)
    same = m[:, None, :] * m[:, :, None] + (1 - m[:, None, :]) * (1 - m[:, :, None])
    logits = logits.masked_fill((same == 0).view(B, 1, 1, T, T), float("-inf"))
    return torch.softmax(logits, dim=-1).reshape(-1, T).float()


def _mask(kind, B, T):
    if kind == "ones":
        return torch.ones(B, T)
    return torch.tensor([[float((t + b) % 3 != 0) for t in range(T)] for b in range(B)])


@pytest.mark.parametrize("c", fp.ATTN_TEMPORAL_CASES, ids=ids(fp.ATTN_TEMPORAL_CASES))
def test_temporal_attention_footprint(nat, c):
    L, e = nat.lib(), c["entry"]
    B, T, P, Cc, heads = c["B"], c["T"], c["P"], c["C"], c["heads"]
    M, tag = B * T * P, f"fp/at/{T}/{P}/{Cc}"
    qkv = rnd(tag + "/qkv", M, 3 * Cc)
    Rs = [0.3 * rnd(tag + f"/R{i}", B, T, T, Cc) for i in range(3)]
    mask = _mask(c["mask"], B, T)
    ins = dict(qkv=inp(qkv), mask=inp(mask))
    outs = dict(o=outp(M, Cc))
    if c["attn"]:
        outs["attn"] = outp(B * P * heads * T, T)
    picked, sel, ring = Rs, None, 0
    if e != "lfvdm_attn_temporal":
        # tables over 3 timesteps [3][B][T][T][C]; the ring form holds exactly `ring` slots: the band starts after slot ring - 1
        tabs = [torch.stack([(0.5 + 0.25 * i) * r for i in range(3)]) for r in Rs]
        slot = [(2 * b + 1) % 3 for b in range(B)]
        picked = [torch.stack([(0.5 + 0.25 * slot[b]) * r[b] for b in range(B)]) for r in Rs]
        ring = 3 if e.endswith("_ring") else 0
        sel = torch.tensor([slot[b] + (3 * (7 + b) if ring else 0) for b in range(B)], dtype=torch.int64, device="cuda")
        Rs = tabs
    for name, r in zip(("Rq", "Rk", "Rv"), Rs):
        ins[name] = inp(r.reshape(-1, Cc))
    want = _temporal_core_f64(qkv.double(), *(r.double() for r in picked), mask.double(), B, T, P, Cc, heads).float()
    want_attn = _temporal_probs_f64(qkv.double(), picked[0].double(), picked[1].double(), mask.double(), B, T, P, Cc, heads)

    def launch(t):
        head = (t["qkv"].ptr, t["Rq"].ptr, t["Rk"].ptr, t["Rv"].ptr, t["mask"].ptr, t["o"].ptr, t["attn"].ptr if c["attn"] else None,
                B, T, P, Cc, heads)
        if e == "lfvdm_attn_temporal":
            rc = L.lfvdm_attn_temporal(*head, nat.stream())
        elif ring:
            rc = L.lfvdm_attn_temporal_ring(*head, sel.data_ptr(), ring, nat.stream())
        else:
            rc = L.lfvdm_attn_temporal_sel(*head, sel.data_ptr(), nat.stream())
        nat.check(rc, e)

    def check(o, f):
        close(o["o"], want, 5e-5)
        if c["attn"]:
            assert float((o["attn"].sum(-1) - 1).abs().max()) < 1e-5
            close(o["attn"], want_attn, 2e-5)           # test_temporal_attention_block

    footprint(e, launch, ins, outs, check, device="cuda")
    counted("attn_temporal")


# ------------------------------------------------------------------------------------------------------------------------
# 4. glue with tiles
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fp.GLUE_CASES, ids=ids(fp.GLUE_CASES))
def test_glue_footprint(nat, c):
    L, e = nat.lib(), c["entry"]
    keep = []
    if e == "lfvdm_conv_in":
        B, T, Cc, H, Cout = c["B"], c["T"], c["C"], c["H"], c["Cout"]
        x, x0 = rnd("fp/ci/x", B, T, Cc, H, H), rnd("fp/ci/x0", B, T, Cc, H, H)
        obs = torch.tensor([1., 0, 1])[:T].repeat(B).reshape(B, T, 1, 1, 1)
        w, b = rnd("fp/ci/w", Cout, Cc + 1, 3, 3, scale=0.2), rnd("fp/ci/b", Cout)
        comp = torch.cat([x * (1 - obs) + x0 * obs, torch.ones_like(x[:, :, :1]) * obs], 2).reshape(B * T, Cc + 1, H, H)
        want = rows(F.conv2d(comp, w, b, padding=1))
        ins = dict(x=inp(x), x0=inp(x0), obs=inp(obs.reshape(-1)), w=inp(w.reshape(Cout, -1)), b=inp(b))
        outs = dict(out=outp(B * T * H * H, Cout))
        launch = lambda t: nat.check(L.lfvdm_conv_in(t["x"].ptr, t["x0"].ptr, t["obs"].ptr, t["w"].ptr, t["b"].ptr, t["out"].ptr, B * T, Cc,
                                                     H, H, Cout, nat.stream()), e)
        check = lambda o, f: close(o["out"], want, 1e-5)
    elif e == "lfvdm_rowdot":
        M, K, O, ldin, ldout = c["M"], c["K"], c["O"], c["ldin"], c["ldout"]
        W, b, x = rnd("fp/rd/w", O, K, scale=0.05), rnd("fp/rd/b", O, scale=0.1), rnd("fp/rd/x", M, K)
        want = F.linear(uo.silu(x), W, b)
        ins, outs = dict(W=inp(W), b=inp(b), x=inp(x, ld=ldin)), dict(out=outp(M, O, ld=ldout))

        def launch(t):
            job = nat.RowdotJob(t["W"].ptr, t["b"].ptr, t["x"].ptr, t["out"].ptr, K, O, M, ldin, ldout, 1, 0, 0)
            keep.append(nat.jobs_to_device([job], "cuda"))
            nat.rowdot(keep[-1], 1, O)
        check = lambda o, f: close(o["out"], want, 2e-5)
    else:
        B, T, ted, widths, pad = c["B"], c["T"], 128, c["widths"], c["tproj_pad"]
        fi = torch.tensor([[0, 1, 2, 3, 4], [3, 17, 18, 400, 999]])[:B, :T]
        temb_b = rnd("fp/rn/temb", B, ted)
        rel = fi.unsqueeze(-1) - fi.unsqueeze(-2)
        ins, outs, want = {}, {}, {}
        for i, Cc in enumerate(widths):
            shapes = {"embed_distances.weight": (Cc, 3), "embed_distances.bias": (Cc,), "embed_diffusion_time.weight": (Cc, ted),
                      "embed_diffusion_time.bias": (Cc,), "out.weight": (Cc, Cc), "out.bias": (Cc,)}
            sd = {"p." + k: torch.from_numpy(recipe.fill_param(f"fprn{i}." + k, s)) for k, s in shapes.items()}
            want[f"R{i}"] = uo.rpe_net(sd, "p", temb_b.repeat_interleave(T, 0), rel, 2).reshape(B * T * T, Cc)
            tproj = F.linear(temb_b, sd["p.embed_diffusion_time.weight"], sd["p.embed_diffusion_time.bias"])
            ins.update({f"tproj{i}": inp(tproj, ld=Cc + pad), f"Wd{i}": inp(sd["p.embed_distances.weight"]),
                        f"bd{i}": inp(sd["p.embed_distances.bias"]), f"Wout{i}": inp(sd["p.out.weight"]), f"bout{i}": inp(sd["p.out.bias"])})
            outs[f"R{i}"] = outp(B * T * T, Cc)
        tiles = (B * T * T + 31) // 32
        fid = fi.cuda()

        def launch(t):
            jobs = [nat.RpeJob(t[f"tproj{i}"].ptr, t[f"Wd{i}"].ptr, t[f"bd{i}"].ptr, t[f"Wout{i}"].ptr, t[f"bout{i}"].ptr, t[f"R{i}"].ptr,
                               Cc, i * tiles, Cc + pad, 0, None) for i, Cc in enumerate(widths)]
            keep.append(nat.jobs_to_device(jobs, "cuda"))
            jp = nat.ptr(keep[-1], torch.uint8)
            if c["maxc"]:
                rc = L.lfvdm_rpe_nets_maxc(jp, len(jobs), len(jobs) * tiles, fid.data_ptr(), B, T, c["maxc"], nat.stream())
            else:
                rc = L.lfvdm_rpe_nets(jp, len(jobs), len(jobs) * tiles, fid.data_ptr(), B, T, nat.stream())
            nat.check(rc, e)

        def check(o, f):
            for k_, w_ in want.items():
                close(o[k_], w_, 2e-5)
    footprint(e, launch, ins, outs, check, device="cuda")
    counted("glue")


# ------------------------------------------------------------------------------------------------------------------------
# 5. backward launches (the atomics forms under the relaxed rule of fp.RELAXED, their deterministic siblings bitwise)
# ------------------------------------------------------------------------------------------------------------------------
def _grad_close(got, want, rel, floor):
    """The bound of test_attn_spatial_backward / test_attn_temporal_backward: rel * (1 + max|g|) + floor."""
    want = want.float()
    err = float((got - want).abs().max())
    assert err <= rel * (1.0 + float(want.abs().max())) + floor, (err, float(want.abs().max()))


@pytest.mark.parametrize("c", fp.BWD_CASES, ids=ids(fp.BWD_CASES))
def test_backward_footprint(nat, c):
    L, e = nat.lib(), c["entry"]
    keep = []
    if e.startswith("lfvdm_gn_temporal_bwd"):
        B, T, P, Cc, acc = c["B"], c["T"], c["P"], c["C"], c["accumulate"]
        x, dy = rnd("fp/gtb/x", B * T * P, Cc) * 1.2 + 0.3, rnd("fp/gtb/dy", B * T * P, Cc)
        gamma, beta = 1 + 0.1 * rnd("fp/gtb/g", Cc), 0.1 * rnd("fp/gtb/b", Cc)
        xr = x.double().view(B, T, P, Cc).permute(0, 2, 3, 1).reshape(B * P, Cc, T).requires_grad_(True)
        gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        F.group_norm(xr, 32, gr, br, eps=1e-5).backward(dy.double().view(B, T, P, Cc).permute(0, 2, 3, 1).reshape(B * P, Cc, T))
        dx0 = rnd("fp/gtb/dx0", B * T * P, Cc)
        want_dx = (xr.grad.view(B, P, Cc, T).permute(0, 3, 1, 2).reshape(B * T * P, Cc) + (dx0.double() if acc else 0)).float()
        ins = dict(x=inp(x), dy=inp(dy), gamma=inp(gamma))
        outs = dict(dx=outp(B * T * P, Cc, init=dx0 if acc else None), dg=outp(1, Cc, init=torch.zeros(Cc)), db=outp(1, Cc, init=torch.zeros(Cc)))
        det = e.endswith("_det")
        if det:
            need = 2 * ((B * P + 3) // 4) * Cc
            outs["ws"] = outp(need // 64, 64, scratch=True)

        def launch(t):
            head = (t["x"].ptr, t["dy"].ptr, t["gamma"].ptr, 1e-5, t["dx"].ptr, t["dg"].ptr, t["db"].ptr, B, T, P, Cc, acc)
            nat.check(L.lfvdm_gn_temporal_bwd_det(*head, t["ws"].ptr, need, nat.stream()) if det
                      else L.lfvdm_gn_temporal_bwd(*head, nat.stream()), e)

        def check(o, f):            # test_gn_temporal_backward
            close(o["dx"], want_dx, 5e-5)
            close(o["dg"].view(-1), gr.grad.float(), 1e-4 * max(1.0, float(gr.grad.abs().max())))
            close(o["db"].view(-1), br.grad.float(), 1e-4 * max(1.0, float(br.grad.abs().max())))
    elif e == "lfvdm_rowdot_bwd":
        M, K, Os, lddout, lddin = c["M"], c["K"], c["O"], c["lddout"], c["lddin"]
        x = rnd("fp/rb/x", M, K)
        Ws = [0.1 * rnd(f"fp/rb/w{i}", O, K) for i, O in enumerate(Os)]
        douts = [rnd(f"fp/rb/d{i}", M, O) for i, O in enumerate(Os)]
        xr = x.double().requires_grad_(True)
        wr = [w.double().requires_grad_(True) for w in Ws]
        act = F.silu(xr)
        act.retain_grad()
        y0, y1 = act @ wr[0].t(), xr @ wr[1].t()
        (y0 * douts[0].double()).sum().backward(retain_graph=True, inputs=[act, wr[0]])
        g_act = act.grad.clone()
        (y1 * douts[1].double()).sum().backward(inputs=[xr, wr[1]])
        want_din = [g_act.float(), xr.grad.float()]
        ins, outs = dict(x=inp(x)), {}
        for i, O in enumerate(Os):
            ld = lddout if O < lddout else O
            ins.update({f"W{i}": inp(Ws[i]), f"d{i}": inp(douts[i], ld=ld)})
            outs.update({f"dW{i}": outp(O, K, init=torch.zeros(O, K)), f"db{i}": outp(1, O, init=torch.zeros(O)),
                         f"din{i}": outp(M, K, ld=lddin, init=torch.zeros(M, K))})
        tasks = [(O + 7) // 8 for O in Os]

        def launch(t):
            jobs = [nat.RowdotBwdJob(t[f"W{i}"].ptr, t["x"].ptr, t[f"d{i}"].ptr, t[f"dW{i}"].ptr, t[f"db{i}"].ptr, t[f"din{i}"].ptr, K, O, M, K,
                                     t[f"d{i}"].ld, lddin, 1 - i, sum(tasks[:i])) for i, O in enumerate(Os)]
            keep.append(nat.jobs_to_device(jobs, "cuda"))
            nat.check(L.lfvdm_rowdot_bwd(keep[-1].data_ptr(), len(jobs), sum(tasks), nat.stream()), e)

        def check(o, f):            # test_rowdot_backward
            for i in range(len(Os)):
                close(o[f"dW{i}"], wr[i].grad.float(), 2e-5)
                close(o[f"db{i}"].view(-1), douts[i].sum(0), 1e-5)
                close(o[f"din{i}"], want_din[i], 2e-5)
    elif e == "lfvdm_attn_spatial_bwd":
        N, P, Cc, heads = c["N"], c["P"], c["C"], c["heads"]
        Fh, M = Cc // heads, N * P
        qkv, d_o = rnd("fp/asb/qkv", N, P, 3 * Cc), rnd("fp/asb/do", M, Cc)
        xg = qkv.double().requires_grad_(True)
        q, k, v = (xg.view(N, P, 3, heads, Fh)[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        attn = torch.softmax((q * Fh ** -0.5) @ k.transpose(-1, -2), -1)
        ((attn @ v).permute(0, 2, 1, 3).reshape(M, Cc) * d_o.double()).sum().backward()
        o, lse = torch.empty(M, Cc, device="cuda"), torch.empty(N * heads, P, device="cuda")
        nat.attn_spatial(qkv.cuda().view(M, 3 * Cc), o, None, N, P, Cc, heads, lse=lse)          # the forward's own o and lse
        ins = dict(qkv=inp(qkv.view(M, 3 * Cc)), o=inp(o.cpu()), d_o=inp(d_o), lse=inp(lse.cpu()))
        outs = dict(delta=outp(N * heads, P, scratch=True), dqkv=outp(M, 3 * Cc))
        launch = lambda t: nat.check(L.lfvdm_attn_spatial_bwd(t["qkv"].ptr, t["o"].ptr, t["d_o"].ptr, t["lse"].ptr, t["delta"].ptr,
                                                              t["dqkv"].ptr, N, P, Cc, heads, nat.stream()), e)
        check = lambda o_, f: _grad_close(o_["dqkv"], xg.grad.view(M, 3 * Cc), 2e-5, 3e-5)
    else:
        B, T, P, Cc, heads = c["B"], c["T"], c["P"], c["C"], c["heads"]
        M = B * T * P
        qkv, d_o = rnd("fp/tb/qkv", M, 3 * Cc), rnd("fp/tb/do", M, Cc)
        Rs = [0.3 * rnd(f"fp/tb/R{i}", B, T, T, Cc) for i in range(3)]
        mask = _mask("mixed", B, T)
        leaves = [t.double().requires_grad_(True) for t in [qkv] + Rs]
        (_temporal_core_f64(*leaves, mask.double(), B, T, P, Cc, heads) * d_o.double()).sum().backward()
        ins = dict(qkv=inp(qkv), d_o=inp(d_o), mask=inp(mask), **{n_: inp(r.reshape(-1, Cc)) for n_, r in zip(("Rq", "Rk", "Rv"), Rs)})
        outs = dict(ws_p=outp(B * P * heads * T, T, scratch=True), ws_ds=outp(B * P * heads * T, T, scratch=True), dqkv=outp(M, 3 * Cc),
                    dRq=outp(B * T * T, Cc), dRk=outp(B * T * T, Cc), dRv=outp(B * T * T, Cc))
        launch = lambda t: nat.check(L.lfvdm_attn_temporal_bwd(*(t[n_].ptr for n_ in ("qkv", "d_o", "Rq", "Rk", "Rv", "mask", "ws_p", "ws_ds",
                                                                                      "dqkv", "dRq", "dRk", "dRv")), B, T, P, Cc, heads,
                                                               nat.stream()), e)

        def check(o, f):            # test_attn_temporal_backward
            for n_, leaf in zip(("dqkv", "dRq", "dRk", "dRv"), leaves):
                _grad_close(o[n_], leaf.grad.reshape(o[n_].shape), 3e-5, 3e-5)
    footprint(e, launch, ins, outs, check, device="cuda")
    counted("bwd")


def test_the_harness_rejects_on_the_device(nat):
    """The device path of the harness is not vacuous: torch ops on the embedded buffers play a launch that writes the first
    float of the trailing band (a), one that multiplies a band word by zero (b), and a correct one."""
    x = rnd("fp/dev/x", 5, 24)
    ins, outs = dict(x=inp(x, ld=32)), dict(y=outp(5, 24, ld=32))
    check = lambda o, f: close64(o["y"], 2 * x, 0.0, 0.0)

    def launch(t, bug=None):
        t["y"].view.copy_(2 * t["x"].view + (t["x"].buf[t["x"].off - 1] * 0 if bug == "mul_zero" else 0))
        if bug == "band_write":
            t["y"].buf[t["y"].off + 5 * 32] = 0.0

    footprint("device_copy", launch, ins, outs, check, device="cuda")
    for bug, rule in (("band_write", "a"), ("mul_zero", "b")):
        with pytest.raises(fp.FootprintError) as err:
            footprint("device_copy", lambda t: launch(t, bug), ins, outs, check, device="cuda")
        assert err.value.rules == {rule}, str(err.value)


# ------------------------------------------------------------------------------------------------------------------------
# 6. operands the header promises are never read
# ------------------------------------------------------------------------------------------------------------------------
def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _all_nan_words(t):
    return bool((t.view(torch.int32) == int(bits(torch.tensor([NAN]))[0])).all())


def test_never_read_operands(nat):
    B, T, Cc, H = 2, 3, 4, 6
    dev = lambda tag, *s: rnd("fp/nr/" + tag, *s).cuda()
    x, out, noise = dev("x", B, T, Cc, H, H), 0.5 * dev("out", B, T, Cc, H, H), dev("noise", B, T, Cc, H, H)
    tabs = {k: (0.5 + 0.4 * rnd("fp/nr/tab/" + k, 1000).abs()).cuda() for k in ("recip", "recipm1", "c1", "c2", "sg", "k3")}
    t = torch.tensor([417, 0], device="cuda")
    new = lambda: [torch.full_like(x, SENT) for _ in range(3)]
    done = []

    def same(a, b, what):
        torch.cuda.synchronize()
        assert all(same_bits(u, v) for u, v in zip(a, b)), what
        done.append(what)

    # the two x0-hat tables under LFVDM_MEAN_X0: lfvdm_update_x0, _rng_x0, _ms_x0
    n1, n2 = _nan(1000), _nan(1000)
    a, b = new(), new()
    nat.update_x0(x, out, noise, t, None, None, tabs["c1"], tabs["c2"], tabs["sg"], nat.RULE_ANCESTRAL, nat.MEAN_X0, True, *a)
    nat.update_x0(x, out, noise, t, n1, n2, tabs["c1"], tabs["c2"], tabs["sg"], nat.RULE_ANCESTRAL, nat.MEAN_X0, True, *b)
    same(a, b, fp.NEVER_READ_CASES[0]["what"])
    seed = torch.tensor([1234], dtype=torch.int64, device="cuda")
    a, b = new(), new()
    nat.update_rng_x0(x, out, None, t, None, None, tabs["c1"], tabs["c2"], tabs["sg"], nat.RULE_ANCESTRAL, nat.MEAN_X0, True, a[0], seed, a[1], a[2])
    nat.update_rng_x0(x, out, None, t, n1, n2, tabs["c1"], tabs["c2"], tabs["sg"], nat.RULE_ANCESTRAL, nat.MEAN_X0, True, b[0], seed, b[1], b[2])
    same(a, b, fp.NEVER_READ_CASES[3]["what"])
    a, b = new(), new()
    nat.update_ms_x0(x, out, None, t, None, None, tabs["c1"], tabs["c2"], tabs["k3"], nat.MEAN_X0, True, a[0], a[1])
    nat.update_ms_x0(x, out, None, t, n1, n2, tabs["c1"], tabs["c2"], tabs["k3"], nat.MEAN_X0, True, b[0], b[1])
    same(a[:2], b[:2], fp.NEVER_READ_CASES[5]["what"])
    # noise / noise_out / seed under the deterministic DDIM rule (sg == NULL)
    nn_ = _nan(B, T, Cc, H, H)
    a, b = new(), new()
    nat.update_x0(x, out, None, t, tabs["recip"], tabs["recipm1"], tabs["c1"], tabs["c2"], None, nat.RULE_DDIM, nat.MEAN_EPS, True, *a)
    nat.update_x0(x, out, nn_, t, tabs["recip"], tabs["recipm1"], tabs["c1"], tabs["c2"], None, nat.RULE_DDIM, nat.MEAN_EPS, True, *b)
    same(a, b, fp.NEVER_READ_CASES[1]["what"])
    bad_seed = torch.tensor([-1], dtype=torch.int64, device="cuda")
    a, b = new(), new()
    nat.update_rng_x0(x, out, None, t, tabs["recip"], tabs["recipm1"], tabs["c1"], tabs["c2"], None, nat.RULE_DDIM, nat.MEAN_EPS, True, a[0],
                      None, a[1], a[2])
    nat.update_rng_x0(x, out, nn_, t, tabs["recip"], tabs["recipm1"], tabs["c1"], tabs["c2"], None, nat.RULE_DDIM, nat.MEAN_EPS, True, b[0],
                      bad_seed, b[1], b[2])
    same(a, b, fp.NEVER_READ_CASES[4]["what"])
    # noise rows with t[b] == 0: the row of batch element 1 may hold anything
    nz = noise.clone()
    nz[1] = NAN
    a, b = new(), new()
    nat.update_x0(x, out, noise, t, tabs["recip"], tabs["recipm1"], tabs["c1"], tabs["c2"], tabs["sg"], nat.RULE_ANCESTRAL, nat.MEAN_EPS, True, *a)
    nat.update_x0(x, out, nz, t, tabs["recip"], tabs["recipm1"], tabs["c1"], tabs["c2"], tabs["sg"], nat.RULE_ANCESTRAL, nat.MEAN_EPS, True, *b)
    same(a, b, fp.NEVER_READ_CASES[2]["what"])
    # hist rows with k3[t] == 0: a first-order step in that row
    k3 = tabs["k3"].clone()
    k3[0] = 0.0
    hist = dev("hist", B, T, Cc, H, H)
    hz = hist.clone()
    hz[1] = NAN
    a, b = new(), new()
    nat.update_ms_x0(x, out, hist, t, tabs["recip"], tabs["recipm1"], tabs["c1"], tabs["c2"], k3, nat.MEAN_EPS, True, a[0], a[1])
    nat.update_ms_x0(x, out, hz, t, tabs["recip"], tabs["recipm1"], tabs["c1"], tabs["c2"], k3, nat.MEAN_EPS, True, b[0], b[1])
    same(a[:2], b[:2], fp.NEVER_READ_CASES[6]["what"])
    # seed / noise_out of lfvdm_known_blend with eps given
    known, m = dev("known", B, T, Cc, H, H), (dev("m", B, T, H, H) > 0).float()
    xa, xb = x.clone(), x.clone()
    nat.known_blend(xa, known, m, t, tabs["c1"], tabs["c2"], eps=noise)
    nat.known_blend(xb, known, m, t, tabs["c1"], tabs["c2"], eps=noise, seed=bad_seed, noise_out=nn_)
    same([xa], [xb], fp.NEVER_READ_CASES[7]["what"])
    torch.cuda.synchronize()
    assert _all_nan_words(n1) and _all_nan_words(n2) and _all_nan_words(nn_), "a never-read buffer was written"
    assert int(bad_seed[0]) == -1 and sorted(done) == sorted(c["what"] for c in fp.NEVER_READ_CASES)
    counted("never_read", len(done))


# ------------------------------------------------------------------------------------------------------------------------
# 7. weight gradients: the three staging variants, every tune code, OIHW, staged affine + SiLU, the grouped launch;
#    with the deterministic slab (bitwise rule) and without (relaxed: float atomics)
# ------------------------------------------------------------------------------------------------------------------------
def _wgrad_bound(got, want):
    """test_conv_wgrad_matches_autograd: max|d| < 2e-5 max(1, max|g|)."""
    err = float((got - want).abs().max())
    assert err < 2e-5 * max(1.0, float(want.abs().max())), err


@pytest.mark.parametrize("c", fp.WGRAD_CASES, ids=[c["entry"].split("/")[-1] + "-" + c["name"] for c in fp.WGRAD_CASES])
def test_conv_wgrad_footprint(nat, monkeypatch, c):
    L, e = nat.lib(), c["entry"]
    for key in ("LFVDM_WGRAD_NO_DMA", "LFVDM_WGRAD_STAGES"):
        monkeypatch.delenv(key, raising=False)
    if e == "lfvdm_conv_wgrad_grouped":
        M, widths, keep = c["M"], c["widths"], []
        ins, outs, want = {}, {}, {}
        for i, Cc in enumerate(widths):
            act, dR = rnd(f"fp/wgg/act{i}", M, Cc), rnd(f"fp/wgg/dR{i}", M, Cc)
            want[i] = ((dR.double().t() @ act.double()).float(), dR.double().sum(0).float())
            ins.update({f"act{i}": inp(act), f"dR{i}": inp(dR)})
            outs.update({f"dW{i}": outp(Cc, Cc, init=torch.zeros(Cc, Cc)), f"db{i}": outp(1, Cc, init=torch.zeros(Cc))})

        def launch(t):
            jobs, task0 = [], 0
            for i, Cc in enumerate(widths):
                a = nat.ConvArgs()
                a.src0, a.res, a.out, a.bias = t[f"act{i}"].ptr, t[f"dR{i}"].ptr, t[f"dW{i}"].ptr, t[f"db{i}"].ptr
                a.C0, a.N, a.Hs, a.Ws, a.Ho, a.Wo, a.ksize, a.stride, a.Cout, a.ldr, a.ldo = Cc, M, 1, 1, 1, 1, 1, 1, Cc, Cc, Cc
                jobs.append(nat.WgradJob(a, 1, task0))
                task0 += (Cc // 32) * (Cc // 32)
            keep.append(nat.jobs_to_device(jobs, "cuda"))
            nat.check(L.lfvdm_conv_wgrad_grouped(keep[-1].data_ptr(), len(jobs), task0, nat.stream()), e)

        def check(o, f):
            for i in range(len(widths)):
                _wgrad_bound(o[f"dW{i}"], want[i][0])
                _wgrad_bound(o[f"db{i}"].view(-1), want[i][1])
        footprint(e, launch, ins, outs, check, device="cuda")
        return counted("wgrad")
    if c["variant"] == "regs":
        monkeypatch.setenv("LFVDM_WGRAD_NO_DMA", "1")
    elif c["variant"]:
        monkeypatch.setenv("LFVDM_WGRAD_STAGES", c["variant"][-1])
    N, H, C0, Cout, k = c["N"], c["H"], c["C0"], c["Cout"], c["k"]
    Cin, M, tag = C0, N * H * H, "fp/wg/" + c["name"]
    x, dout = rnd(tag + "/x", N, Cin, H, H), rnd(tag + "/d", N, Cout, H, H)
    w, b = rnd(tag + "/w", Cout, Cin, k, k, scale=0.05).requires_grad_(True), rnd(tag + "/b", Cout).requires_grad_(True)
    ins = dict(src0=inp(rows(x)), res=inp(rows(dout)))
    xin = x
    if c.get("coef"):
        cA, cB = 1 + 0.2 * rnd(tag + "/cA", N, Cin), 0.2 * rnd(tag + "/cB", N, Cin)
        xin = F.silu(x * cA[:, :, None, None] + cB[:, :, None, None])
        ins.update(coefA=inp(cA), coefB=inp(cB))
    F.conv2d(xin, w, b, padding=1).backward(dout)
    want_w = w.grad if c.get("oihw") else w.grad.permute(0, 2, 3, 1)
    outs = dict(out=outp(Cout, k * k * Cin, init=torch.zeros(Cout, k * k * Cin)), bias=outp(1, Cout, init=torch.zeros(Cout)))
    slab = e.endswith("/slab")
    slab_floats = 16 * (Cout * k * k * Cin + Cout)
    if slab:
        outs["slab"] = outp(slab_floats // 64, 64, scratch=True)

    def fill(a, t):
        a.src0, a.res, a.out, a.bias = t["src0"].ptr, t["res"].ptr, t["out"].ptr, t["bias"].ptr
        a.C0, a.N, a.Hs, a.Ws, a.Ho, a.Wo, a.ksize, a.stride, a.Cout, a.ldr, a.ldo = Cin, N, H, H, H, H, k, 1, Cout, Cout, Cout
        a.out_mode = 1 if c.get("oihw") else 0
        if c.get("coef"):
            a.coefA, a.coefB, a.act = t["coefA"].ptr, t["coefB"].ptr, nat.ACT_SILU
        if slab:
            a.splitk_ws, a.splitk_ws_floats = t["slab"].ptr, slab_floats

    def check(o, f):
        _wgrad_bound(o["out"].reshape(want_w.shape), want_w.detach())
        _wgrad_bound(o["bias"].view(-1), b.grad)

    codes = [0]
    if c.get("codes"):
        a = nat.ConvArgs()
        fill(a, {k_: fp.Embedded(op, SENT, "cuda") for k_, op in {**ins, **outs}.items()})
        codes += nat._wgrad_codes(a)
        assert len(codes) > 1
    for code in codes:
        def launch(t, code=code):
            a = nat.ConvArgs()
            fill(a, t)
            a.tune = code
            nat.check(L.lfvdm_conv_wgrad(C.byref(a), nat.stream()), f"{e} (tune {code})")
        footprint(e, launch, ins, outs, check, device="cuda")
        counted("wgrad")


# ------------------------------------------------------------------------------------------------------------------------
# 8. spatial GroupNorm backward: atomics (relaxed) and deterministic (sums_out, bitwise), every channel split + one large map
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fp.GN_BWD_CASES, ids=[c["entry"].split("_")[-1] + "-" + i for c, i in zip(fp.GN_BWD_CASES, ids(fp.GN_BWD_CASES))])
def test_groupnorm_backward_footprint(nat, c):
    L, e = nat.lib(), c["entry"]
    if e == "lfvdm_gn_param_grads":
        N, T, Cc, ld = c["N"], c["T"], c["C"], 2 * c["C"] + c["pad"]
        sums, gamma, beta = rnd("fp/gg/s", N, Cc, 2), 1 + 0.1 * rnd("fp/gg/g", Cc), 0.1 * rnd("fp/gg/b", Cc)
        film, dg0, db0 = 0.3 * rnd("fp/gg/f", N // T, 2 * Cc), rnd("fp/gg/dg", Cc), rnd("fp/gg/db", Cc)
        s1, s2 = sums[..., 0].double(), sums[..., 1].double()
        sc1 = 1 + film[:, :Cc].double().repeat_interleave(T, 0)
        dsc = (s2 * gamma.double() + s1 * beta.double()).view(N // T, T, Cc).sum(1)
        ins = dict(sums=inp(sums.reshape(N, 2 * Cc)), gamma=inp(gamma), beta=inp(beta), film=inp(film, ld=ld))
        outs = dict(dg=outp(1, Cc, init=dg0), db=outp(1, Cc, init=db0), dfilm=outp(N // T, 2 * Cc, ld=ld))
        launch = lambda t: nat.check(L.lfvdm_gn_param_grads(t["sums"].ptr, t["gamma"].ptr, t["beta"].ptr, t["film"].ptr, ld, T, t["dg"].ptr,
                                                            t["db"].ptr, t["dfilm"].ptr, ld, N, Cc, nat.stream()), e)

        def check(o, f):            # test_gn_param_grads
            close(o["dg"].view(-1), (dg0.double() + (s2 * sc1).sum(0)).float(), 2e-5)
            close(o["db"].view(-1), (db0.double() + (s1 * sc1).sum(0)).float(), 2e-5)
            close(o["dfilm"], torch.cat([dsc, s1.view(N // T, T, Cc).sum(1)], 1).float(), 2e-5)
        footprint(e, launch, ins, outs, check, device="cuda")
        return counted("gn_bwd")
    C0, C1, N, T, P, act = c["C0"], c["C1"], c["N"], c["T"], c["P"], c["act"]
    Cc, tag = C0 + C1, f"fp/gb/{C0}/{C1}/{P}"
    a = rnd(tag + "/a", N * P, C0) * 1.3 + 0.7
    b = rnd(tag + "/b", N * P, C1) if C1 else None
    gamma, beta = 1 + 0.1 * rnd(tag + "/g", Cc), 0.1 * rnd(tag + "/be", Cc)
    fm, da, add = 0.3 * rnd(tag + "/film", N // T, 2 * Cc), rnd(tag + "/da", N * P, Cc), rnd(tag + "/add", N * P, Cc)
    dx_ref, g_ref, b_ref, f_ref = _gn_reference(a, b, C0, C1, N, P, gamma, beta, fm, T, act, da)
    dx_ref = dx_ref + add.double()
    dev = lambda t: None if t is None else t.cuda().contiguous()
    ad, bd, gd, bed, fd = dev(a), dev(b), dev(gamma), dev(beta), dev(fm)
    cA, cB, st = torch.empty(N, Cc, device="cuda"), torch.empty(N, Cc, device="cuda"), torch.empty(N, 64, device="cuda")
    nat.check(L.lfvdm_gn_coef_stats(nat.ptr(ad), nat.ptr(bd), C0, C1, N, P, nat.ptr(gd), nat.ptr(bed), nat.ptr(fd), T, 2 * Cc, 1e-5,
                                    nat.ptr(cA), nat.ptr(cB), nat.ptr(st), nat.stream()), "lfvdm_gn_coef_stats")
    film_ld, add_ld = 2 * Cc + c["pad"], Cc + c["pad"]
    ins = dict(da=inp(da), src0=inp(a), coefA=inp(cA.cpu()), coefB=inp(cB.cpu()), stats=inp(st.cpu()), add=inp(add, ld=add_ld),
               gamma=inp(gamma), beta=inp(beta), film=inp(fm, ld=film_ld))
    outs = dict(out0=outp(N * P, C0))
    if C1:
        ins["src1"], outs["out1"] = inp(b), outp(N * P, C1)
    det = e.endswith("/det")
    if det:
        outs["sums"] = outp(N, 2 * Cc)
    else:
        outs.update(dg=outp(1, Cc, init=torch.zeros(Cc)), db=outp(1, Cc, init=torch.zeros(Cc)),
                    dfilm=outp(N // T, 2 * Cc, ld=film_ld, init=torch.zeros(N // T, 2 * Cc)))
    need = int(L.lfvdm_gn_bwd_ws_floats(Cc, N, P))
    assert (need > 0) == (P == 1061)
    if need:
        outs["ws"] = outp(need // 64, 64, scratch=True) if need % 64 == 0 else outp(1, need, scratch=True)

    def launch(t):
        g = nat.GnBwdArgs()
        for name in ("da", "src0", "src1", "coefA", "coefB", "stats", "out0", "out1", "add", "gamma", "beta", "film", "ws"):
            setattr(g, name, t[name].ptr if name in t else None)
        if det:
            g.sums_out = t["sums"].ptr
        else:
            g.dgamma, g.dbeta, g.dfilm = t["dg"].ptr, t["db"].ptr, t["dfilm"].ptr
        g.ws_floats, g.C0, g.C1, g.N, g.P, g.act = need, C0, C1, N, P, act
        g.add_ld, g.add2_ld, g.film_ld, g.T, g.dfilm_ld = add_ld, 0, film_ld, T, film_ld
        nat.check(L.lfvdm_gn_bwd(C.byref(g), nat.stream()), e)

    def check(o, f):                # bounds of test_norm_backward_gpu.test_gn_backward_small_slices
        dx = torch.cat([o["out0"]] + ([o["out1"]] if C1 else []), 1)
        close(dx, dx_ref.float(), 3e-5 * max(float(dx_ref.abs().max()), 1.0))
        if det:                     # the stored sums, folded as lfvdm_gn_param_grads folds them
            s = o["sums"].view(N, Cc, 2).double()
            sc1 = 1 + fm[:, :Cc].double().repeat_interleave(T, 0)
            dg, db = (s[..., 1] * sc1).sum(0), (s[..., 0] * sc1).sum(0)
        else:
            dg, db = o["dg"].view(-1), o["db"].view(-1)
            close(o["dfilm"], f_ref.float(), 2e-4 * float(f_ref.abs().max()))
        close(dg, g_ref.float(), 2e-4 * float(g_ref.abs().max()))
        close(db, b_ref.float(), 2e-4 * float(b_ref.abs().max()))

    footprint(e, launch, ins, outs, check, device="cuda")
    counted("gn_bwd")


# ------------------------------------------------------------------------------------------------------------------------
# 9. the deterministic row-dot backward, the grouped RPE backward (both forms), the RPE hidden layer
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fp.TRAIN_GLUE_CASES, ids=[c["entry"] for c in fp.TRAIN_GLUE_CASES])
def test_training_glue_footprint(nat, c):
    L, e = nat.lib(), c["entry"]
    keep = []
    if e == "lfvdm_rowdot_bwd_det":
        M, K, Os, lddout, lddin = c["M"], c["K"], c["O"], c["lddout"], c["lddin"]
        x = rnd("fp/rbd/x", M, K)
        Ws = [0.1 * rnd(f"fp/rbd/w{i}", O, K) for i, O in enumerate(Os)]
        douts = [rnd(f"fp/rbd/d{i}", M, O) for i, O in enumerate(Os)]
        xr = x.double().requires_grad_(True)
        wr = [w.double().requires_grad_(True) for w in Ws]
        act = F.silu(xr)
        act.retain_grad()
        y0, y1 = act @ wr[0].t(), xr @ wr[1].t()
        (y0 * douts[0].double()).sum().backward(retain_graph=True, inputs=[act, wr[0]])
        g_act = act.grad.clone()
        (y1 * douts[1].double()).sum().backward(inputs=[xr, wr[1]])
        want_din = torch.cat([g_act, xr.grad]).float()
        ins = dict(x=inp(x))
        # both din arrays are rows of ONE array (din_base, din_n); its padding columns must keep the fill
        outs = dict(din=outp(2 * M, K, ld=lddin, init=torch.zeros(2 * M, K)))
        tasks = [(O + 7) // 8 for O in Os]
        din_n = 2 * M * lddin
        outs["ws"] = outp(sum(tasks) * din_n // 64, 64, scratch=True)
        for i, O in enumerate(Os):
            ins.update({f"W{i}": inp(Ws[i]), f"d{i}": inp(douts[i], ld=max(O, lddout))})
            outs.update({f"dW{i}": outp(O, K, init=torch.zeros(O, K)), f"db{i}": outp(1, O, init=torch.zeros(O))})

        def launch(t):
            jobs = [nat.RowdotBwdJob(t[f"W{i}"].ptr, t["x"].ptr, t[f"d{i}"].ptr, t[f"dW{i}"].ptr, t[f"db{i}"].ptr,
                                     t["din"].ptr + 4 * i * M * lddin, K, O, M, K, t[f"d{i}"].ld, lddin, 1 - i, sum(tasks[:i]))
                    for i, O in enumerate(Os)]
            keep.append(nat.jobs_to_device(jobs, "cuda"))
            nat.check(L.lfvdm_rowdot_bwd_det(keep[-1].data_ptr(), len(jobs), sum(tasks), t["din"].ptr, din_n, t["ws"].ptr,
                                             sum(tasks) * din_n, nat.stream()), e)

        def check(o, f):            # test_norm_backward_gpu.test_rowdot_backward_deterministic
            for i in range(len(Os)):
                close(o[f"dW{i}"], wr[i].grad.float(), 2e-5)
                close(o[f"db{i}"].view(-1), douts[i].sum(0), 1e-5)
            close(o["din"], want_din, 2e-5)
    elif e.startswith("lfvdm_rpe_nets_bwd"):
        B, T, widths, pad = c["B"], c["T"], c["widths"], c["pad"]
        fi, nets = rpe_case(B, T, widths)
        fid = fi.cuda()
        tiles = (B * T * T + 31) // 32
        ins, outs = {}, {}
        for i, net in enumerate(nets):
            Cc = net["C"]
            ins.update({f"tproj{i}": inp(net["tproj"], ld=Cc + pad), f"Wd{i}": inp(net["Wd"]), f"bd{i}": inp(net["bd"]),
                        f"Wt{i}": inp(net["Wout"].t().contiguous()), f"dR{i}": inp(net["dR"])})
            outs.update({f"dtproj{i}": outp(B, Cc, ld=Cc + pad, init=torch.zeros(B, Cc)), f"dWd{i}": outp(Cc, 3, init=torch.zeros(Cc, 3)),
                         f"dbd{i}": outp(1, Cc, init=torch.zeros(Cc))})
        det = e.endswith("_det")
        if det:
            outs["ws"] = outp(len(nets) * tiles * DET_LD // 64, 64, scratch=True)

        def launch(t):
            jobs = [nat.RpeBwdJob(t[f"tproj{i}"].ptr, t[f"Wd{i}"].ptr, t[f"bd{i}"].ptr, t[f"Wt{i}"].ptr, t[f"dR{i}"].ptr, t[f"dtproj{i}"].ptr,
                                  t[f"dWd{i}"].ptr, t[f"dbd{i}"].ptr, net["C"], i * tiles, net["C"] + pad, net["C"] + pad)
                    for i, net in enumerate(nets)]
            keep.append(nat.jobs_to_device(jobs, "cuda"))
            head = (keep[-1].data_ptr(), len(jobs), len(jobs) * tiles, fid.data_ptr(), B, T)
            nat.check(L.lfvdm_rpe_nets_bwd_det(*head, t["ws"].ptr, len(jobs) * tiles * DET_LD, nat.stream()) if det
                      else L.lfvdm_rpe_nets_bwd(*head, nat.stream()), e)

        def check(o, f):            # test_rpe_grouped_gpu.Launch.check_grads: within 8 e32 of the fp64 gradient
            for i, net in enumerate(nets):
                for k_ in ("dtproj", "dWd", "dbd"):
                    g64 = net["g64"][k_]
                    err = float((o[f"{k_}{i}"].double().reshape(g64.shape) - g64).abs().max()) / max(float(g64.abs().max()), 1e-30)
                    assert err <= 8.0 * net["e32"][k_], (i, k_, err, net["e32"][k_])
    elif e == "lfvdm_rpe_front_bwd":
        B, T, Cc, pad = c["B"], c["T"], c["C"], c["pad"]
        n = B * T * T
        tp, feats = rnd("fp/rfb/tp", B, Cc), rnd("fp/rfb/f", n, 3).abs()
        wd, bd, d_act = 0.5 * rnd("fp/rfb/wd", Cc, 3), 0.1 * rnd("fp/rfb/bd", Cc), rnd("fp/rfb/da", n, Cc)
        tpr, wdr, bdr = (v.double().requires_grad_(True) for v in (tp, wd, bd))
        (F.silu(tpr.repeat_interleave(T * T, 0) + feats.double() @ wdr.t() + bdr) * d_act.double()).sum().backward()
        ins = dict(tp=inp(tp, ld=Cc + pad), f=inp(feats), wd=inp(wd), bd=inp(bd), da=inp(d_act))
        outs = dict(dtp=outp(B, Cc, ld=Cc + pad, init=torch.zeros(B, Cc)), dwd=outp(Cc, 3, init=torch.zeros(Cc, 3)),
                    dbd=outp(1, Cc, init=torch.zeros(Cc)))
        launch = lambda t: nat.check(L.lfvdm_rpe_front_bwd(t["tp"].ptr, Cc + pad, t["f"].ptr, t["wd"].ptr, t["bd"].ptr, t["da"].ptr, t["dtp"].ptr,
                                                           Cc + pad, t["dwd"].ptr, t["dbd"].ptr, B, T * T, Cc, nat.stream()), e)

        def check(o, f):            # test_rpe_front_and_backward
            close(o["dtp"], tpr.grad.float(), 1e-4)
            close(o["dwd"], wdr.grad.float(), 1e-4)
            close(o["dbd"].view(-1), bdr.grad.float(), 1e-4)
    else:
        B, T, Cc, pad = c["B"], c["T"], c["C"], c["pad"]
        n = B * T * T
        tp, feats = rnd("fp/rf/tp", B, Cc), rnd("fp/rf/f", n, 3).abs()
        wd, bd = 0.5 * rnd("fp/rf/wd", Cc, 3), 0.1 * rnd("fp/rf/bd", Cc)
        want = F.silu(tp.double().repeat_interleave(T * T, 0) + feats.double() @ wd.double().t() + bd.double()).float()
        ins, outs = dict(tp=inp(tp, ld=Cc + pad), f=inp(feats), wd=inp(wd), bd=inp(bd)), dict(act=outp(n, Cc))
        launch = lambda t: nat.check(L.lfvdm_rpe_front(t["tp"].ptr, Cc + pad, t["f"].ptr, t["wd"].ptr, t["bd"].ptr, t["act"].ptr, B, T * T, Cc,
                                                       nat.stream()), e)
        check = lambda o, f: close(o["act"], want, 2e-5)          # test_rpe_front_and_backward
    footprint(e, launch, ins, outs, check, device="cuda")
    counted("train_glue")


# ------------------------------------------------------------------------------------------------------------------------
# 10. fused launches and the sampler's step seam
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fp.FUSED_CASES, ids=[c["entry"] for c in fp.FUSED_CASES])
def test_fused_launches_footprint(nat, c):
    L, e = nat.lib(), c["entry"]
    if e == "lfvdm_gn_temporal_qkv":
        B, T, P, Cc = c["B"], c["T"], c["P"], c["C"]
        assert L.lfvdm_gn_temporal_qkv_ok(B, T, P, Cc) == 0
        M = B * T * P
        x = rnd("fp/tq/x", M, Cc) * 1.3 + 0.25
        gam, bet = rnd("fp/tq/g", Cc) * 0.3 + 1.0, rnd("fp/tq/b", Cc) * 0.2
        W, bias = rnd("fp/tq/w", 3 * Cc, Cc) * (Cc ** -0.5), rnd("fp/tq/bias", 3 * Cc) * 0.1
        xc = x.view(B, T, P, Cc).permute(0, 2, 3, 1).reshape(B * P, Cc, T).double()
        ref_n = F.group_norm(xc, 32, gam.double(), bet.double(), 1e-5).view(B, P, Cc, T).permute(0, 3, 1, 2).reshape(M, Cc)
        ref_q = ref_n @ W.double().t() + bias.double()
        ins = dict(x=inp(x), g=inp(gam), b=inp(bet), W=inp(W), bias=inp(bias))
        outs = dict(xn=outp(M, Cc), qkv=outp(M, 3 * Cc))
        launch = lambda t: nat.check(L.lfvdm_gn_temporal_qkv(t["x"].ptr, t["g"].ptr, t["b"].ptr, 1e-5, t["xn"].ptr, t["W"].ptr, t["bias"].ptr,
                                                             t["qkv"].ptr, B, T, P, Cc, nat.stream()), e)

        def check(o, f):            # test_temporal_groupnorm_with_the_qkv_projection_inside
            close(o["xn"], ref_n, 1e-5)
            close(o["qkv"], ref_q, 2e-5)
    elif e == "lfvdm_proj_gn":
        N, P, Cc = c["N"], c["P"], c["C"]
        assert L.lfvdm_proj_gn_ok(N, P, Cc) == 0
        M = N * P
        o_, res = rnd("fp/pg/o", M, Cc) * 0.8, rnd("fp/pg/res", M, Cc) * 1.2 + 0.3
        W, bias = rnd("fp/pg/w", Cc, Cc) * (Cc ** -0.5), rnd("fp/pg/bias", Cc) * 0.1
        gam, bet = rnd("fp/pg/g", Cc) * 0.3 + 1.0, rnd("fp/pg/b", Cc) * 0.2
        y64 = o_.double() @ W.double().t() + bias.double() + res.double()
        ref = F.group_norm(y64.view(N, P, Cc).permute(0, 2, 1), 32, gam.double(), bet.double(), 1e-5).permute(0, 2, 1).reshape(M, Cc)
        ins = dict(o=inp(o_), W=inp(W), bias=inp(bias), res=inp(res), g=inp(gam), b=inp(bet))
        outs = dict(out=outp(M, Cc), raw=outp(M, Cc))
        launch = lambda t: nat.check(L.lfvdm_proj_gn(t["o"].ptr, t["W"].ptr, t["bias"].ptr, t["res"].ptr, t["g"].ptr, t["b"].ptr, 1e-5,
                                                     nat.ACT_NONE, t["out"].ptr, t["raw"].ptr, N, P, Cc, nat.stream()), e)

        def check(o, f):            # test_projection_with_the_next_groupnorm_inside
            close(o["out"], ref, 2e-5)
            close(o["raw"], y64, 2e-5)
    elif e == "lfvdm_conv_igemm+lfvdm_gn_apply_part":
        N, H, Cin, C0, C1 = c["N"], c["H"], c["Cin"], c["C0"], c["C1"]
        Cc, P, M = C0 + C1, H * H, N * H * H
        gw = Cc // 32
        x, w, b = rnd("fp/cat/x", N, Cin, H, H), rnd("fp/cat/w", C0, Cin, 3, 3, scale=0.05), rnd("fp/cat/b", C0)
        skip = rnd("fp/cat/skip", N, C1, H, H)
        gamma, beta = 1 + 0.1 * rnd("fp/cat/g", Cc), 0.1 * rnd("fp/cat/be", Cc)
        h = F.conv2d(x.double(), w.double(), b.double(), padding=1)
        ref = rows(F.silu(F.group_norm(torch.cat([h, skip.double()], 1), 32, gamma.double(), beta.double(), eps=1e-5)))
        ins = dict(src0=inp(rows(x)), W=inp(w.permute(0, 2, 3, 1).reshape(C0, 9 * Cin)), bias=inp(b), skip=inp(rows(skip)), gamma=inp(gamma),
                   beta=inp(beta))
        outs = dict(act=outp(M, Cc), raw=outp(M, C0))

        def fill(a, t):
            a.src0, a.W, a.bias, a.out, a.gn_out = t["src0"].ptr, t["W"].ptr, t["bias"].ptr, t["raw"].ptr, t["act"].ptr
            a.gn_gamma, a.gn_beta = t["gamma"].ptr, t["beta"].ptr
            a.C0, a.N, a.Hs, a.Ws, a.Ho, a.Wo, a.ksize, a.stride, a.Cout, a.ldo, a.ldr = Cin, N, H, H, H, H, 3, 1, C0, C0, C0
            a.gn_film_div, a.gn_act, a.gn_eps, a.gn_gw, a.gn_ld = 1, nat.ACT_SILU, 1e-5, gw, Cc

        a0 = nat.ConvArgs()
        fill(a0, {k_: fp.Embedded(op, SENT, "cuda") for k_, op in {**ins, **outs}.items()})
        codes = (C.c_int * 256)()
        n = L.lfvdm_conv_igemm_candidates(C.byref(a0), codes, 256)
        assert n > 0

        def check(o, f):            # test_concat_groupnorm_half_by_half_every_tune_code
            close64(o["act"], ref, 1e-4, 0.0)
            close64(o["raw"], rows(h), 5e-5, 0.0)
        for code, general in [(cd, g) for cd in [0] + [codes[i] for i in range(n)] for g in (0, 1)]:
            def launch(t, code=code, general=general):
                nat.check(L.lfvdm_gn_apply_part(t["skip"].ptr, C1, N, P, gw, t["gamma"].ptr + 4 * C0, t["beta"].ptr + 4 * C0, 1e-5, nat.ACT_SILU,
                                                t["act"].ptr + 4 * C0, Cc, nat.stream()), "lfvdm_gn_apply_part")
                a = nat.ConvArgs()
                fill(a, t)
                a.tune, a.gn_general = code, general
                nat.check(L.lfvdm_conv_igemm(C.byref(a), nat.stream()), f"lfvdm_conv_igemm (tune {code}, general {general})")
            footprint(e, launch, ins, outs, check, device="cuda")
            counted("fused")
        return
    elif e.startswith("lfvdm_conv_out_update"):
        B, T, H, W_, Cc, Cout = c["B"], c["T"], c["H"], c["W"], c["C"], c["Cout"]
        N, ms = B * T, e.endswith("_ms_x0")
        a_, w, bias = rnd("fp/co/a", N, Cc, H, W_), rnd("fp/co/w", Cout, Cc, 3, 3, scale=0.05), rnd("fp/co/b", Cout)
        ref_eps = F.conv2d(a_, w, bias, padding=1).view(B, T, Cout, H, W_)
        x, given = rnd("fp/co/x", B, T, Cout, H, W_), rnd("fp/co/n", B, T, Cout, H, W_)
        tabs = [0.5 + rnd(f"fp/co/tab{i}", 1000).abs() for i in range(4)] + [0.3 * rnd("fp/co/tab4", 1000)]
        t_ = torch.tensor([7], dtype=torch.int64, device="cuda")
        ins = dict(act=inp(rows(a_)), wp=inp(w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cc)), bias=inp(bias), x=inp(x), z=inp(given),
                   **{f"tab{i}": inp(tb) for i, tb in enumerate(tabs)})
        outs = dict(eps=outp(B * T * Cout * H, W_), sample=outp(B * T * Cout * H, W_), pred=outp(B * T * Cout * H, W_))
        tabs_d, xd, zd = [tb.cuda() for tb in tabs], x.cuda(), given.cuda()

        def launch(t):
            tb = [t[f"tab{i}"].ptr for i in range(5)]
            if ms:
                rc = L.lfvdm_conv_out_update_ms_x0(t["act"].ptr, t["wp"].ptr, t["bias"].ptr, t["eps"].ptr, t["x"].ptr, t["z"].ptr, t_.data_ptr(),
                                                   *tb, nat.MEAN_EPS, 1, t["sample"].ptr, t["pred"].ptr, B, T, H, W_, Cc, Cout, nat.stream())
            else:
                rc = L.lfvdm_conv_out_update_x0(t["act"].ptr, t["wp"].ptr, t["bias"].ptr, t["eps"].ptr, t["x"].ptr, t["z"].ptr, None,
                                                t_.data_ptr(), *tb, nat.RULE_ANCESTRAL, nat.MEAN_EPS, 1, t["sample"].ptr, t["pred"].ptr, None,
                                                B, T, H, W_, Cc, Cout, None, nat.stream())
            nat.check(rc, e)

        def check(o, f):            # test_conv_out_psample_equals_conv_then_update: eps < 5e-5, the update bitwise the two-launch form's
            close64(o["eps"].view(-1), ref_eps.reshape(-1), 5e-5, 0.0)
            eps_d = o["eps"].reshape(x.shape).cuda()
            s2, p2 = torch.empty_like(xd), torch.empty_like(xd)
            if ms:
                nat.update_ms_x0(xd, eps_d, zd, t_, *tabs_d, nat.MEAN_EPS, True, s2, p2)
            else:
                nat.update_x0(xd, eps_d, zd, t_, *tabs_d, nat.RULE_ANCESTRAL, nat.MEAN_EPS, True, s2, p2)
            torch.cuda.synchronize()
            assert same_bits(o["sample"].reshape(x.shape), s2) and same_bits(o["pred"].reshape(x.shape), p2)
    elif e == "lfvdm_dyn_threshold":
        B, T, Fi, pct = c["B"], c["T"], c["F"], c["pct"]
        p0, mask = make_input("gauss", (B, T, Fi)), masks_for(B, T)[c["mask"]]
        nbytes = nat.dyn_threshold_workspace(B, T * Fi)
        assert nbytes > 0 and nbytes % 4 == 0
        nw = nbytes // 4
        t_ = torch.zeros(B, dtype=torch.int64, device="cuda")
        ins = dict(mo=inp(p0.reshape(B * T, Fi)), mask=inp(mask))
        # the workspace is zero-filled once by the caller; the words past its documented size are the band
        outs = dict(xhat=outp(B * T, Fi), stats=outp(B, 3),
                    ws=outp(nw // 64, 64, init=torch.zeros(nw), scratch=True) if nw % 64 == 0 else outp(1, nw, init=torch.zeros(nw), scratch=True))
        launch = lambda t: nat.check(L.lfvdm_dyn_threshold(t["mo"].ptr, t["mo"].ptr, t_.data_ptr(), None, None, nat.MEAN_X0, 0, t["mask"].ptr,
                                                           B, T, Fi, pct, float("inf"), t["xhat"].ptr, t["stats"].ptr, t["ws"].ptr,
                                                           nat.stream()), e)
        check = lambda o, f: check_against_host(p0, mask, pct, None, o["xhat"].view(B, T, Fi), o["stats"])     # test_dyn_threshold_gpu
    else:
        B, rf, ld, S = c["B"], c["row_floats"], c["rows_ld"], 5
        t0 = torch.tensor([5, 0, 3], dtype=torch.int64)[:B]
        table = torch.tensor([0.0, 250.25, 500.5, 750.75, 999.0, 1000.0])
        rows_all = torch.arange(S * B * rf, dtype=torch.float32).view(S * B, rf) + 0.5
        t_new = (t0 - 1).clamp_min(0)
        ins = dict(table=inp(table), rows_all=inp(rows_all, ld=ld))
        outs = dict(model_t=outp(1, B), rows=outp(B, rf, ld=ld))
        clocks = []

        def launch(t):
            clocks.append(t0.cuda())
            nat.check(L.lfvdm_sampler_tick_fetch(clocks[-1].data_ptr(), t["table"].ptr, t["model_t"].ptr, B, t["rows_all"].ptr, ld,
                                                 t["rows"].ptr, rf, nat.stream()), e)

        def check(o, f):            # test_glue_ops_gpu.clock_ref: a copy, bit for bit
            assert clocks[-1].cpu().tolist() == t_new.tolist()
            assert same_bits(o["model_t"].view(-1), table[t_new]) and same_bits(o["rows"], rows_all.view(S, B, rf)[t_new, torch.arange(B)])
    footprint(e, launch, ins, outs, check, device="cuda")
    counted("fused")
