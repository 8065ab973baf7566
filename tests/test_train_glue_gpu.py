"""Bit-exact op tests of the kernels that move and fold data around a training step: lfvdm_prepare_batch, lfvdm_det_reduce,
det_reduce2_kernel through lfvdm_conv_wgrad and the deterministic GroupNorm parameter gradients, lfvdm_pack_conv_weights /
lfvdm_unpack_conv_grads and their single-tensor forms, and the host query lfvdm_conv_igemm_config.

The cases, the host restatements and the proof that the cases can tell a wrong kernel from a right one are in
test_train_glue_cpu.  Every output, workspace and padding region starts as NaN or a sentinel; sections 1, 2 and 4 compare
words (torch.equal on the raw bits, so a NaN left behind cannot hide), section 3 uses the bounds of
test_backward_nodes_cpu.Case ("wgrad") and of test_norm_backward_gpu and nothing new.

det_reduce2_kernel is reached by lfvdm_conv_wgrad (slab + bias gradient) and by lfvdm_gn_temporal_bwd_det.  The SPATIAL
GroupNorm backward (lfvdm_gn_bwd) takes its deterministic parameter gradients another way - the per-sample sums go to
sums_out and lfvdm_gn_param_grads adds them in sample order - so section 3 runs both: the temporal entry for the kernel,
lfvdm_gn_bwd (through _backward._gn_backward, as test_norm_backward_gpu builds the record) for the path a training step
takes.

Observed on an MI355X (gfx950):
- section 1 (batch gather): 198 comparisons of words, all equal; every refusal returned LFVDM_E_SHAPE and wrote nothing.
- section 2 (ordered reduction): 59 comparisons, all equal, both second-trip cases included.
- section 3 (two destinations): 64 comparisons; worst error / bound 0.009 (packed weight gradient of the 32 x 32 3x3 case,
  one slice), bias gradients <= 0.006, GroupNorm parameter gradients <= 0.002; every run repeated bit for bit.
- section 4 (pack / unpack): 68 comparisons, all equal; test_ops_gpu.test_grouped_pack_and_unpack now asks for equal words
  too (its two jobs held bitwise).
- section 5 (lfvdm_conv_igemm_config): 484 queries, none failed, none launched.
- no kernel had to change.  The whole file ran in 4 s, no test above 0.8 s.
GPU only."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import test_train_glue_cpu as tg
from test_train_glue_cpu import NAN, SENT, GUARD, bits, same_bits
from test_ops_gpu import rnd
from test_backward_nodes_cpu import Case, to_rows, nchw
from test_norm_backward_gpu import _gn_reference, _pl, _gnt_columns, _gnt_rows

pytestmark = pytest.mark.gpu

E_SHAPE, E_UNSUPPORTED = 1, 3
COUNT = {}                      # comparisons per section, printed by the last test


def counted(section, ok, what=""):
    COUNT[section] = COUNT.get(section, 0) + 1
    assert ok, what


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from improved_diffusion import _native
    _native.lib()
    return _native


def guarded(values, before=GUARD, after=GUARD):
    """-> (buffer, view): `values` (or that many NaN) between two guard bands of the sentinel."""
    n = values if isinstance(values, int) else values.numel()
    buf = torch.full((before + n + after,), SENT, device="cuda")
    view = buf[before:before + n]
    if isinstance(values, int):
        view.fill_(NAN)
    else:
        view.copy_(values.reshape(-1))
    return buf, view


def guards_intact(buf, n, before=GUARD):
    return bool((buf[:before] == SENT).all()) and bool((buf[before + n:] == SENT).all())


# ------------------------------------------------------------------------------------------------------------------------
# 1. batch gather
# ------------------------------------------------------------------------------------------------------------------------
def _gather_outputs(B, F, fe):
    buf, batch = guarded(B * F * fe)
    return dict(buf=buf, batch=batch, fi=torch.full((B, F), -7777, dtype=torch.int64, device="cuda"),
                obs=torch.full((B, F), NAN, device="cuda"), lat=torch.full((B, F), NAN, device="cuda"))


def _gather_launch(nat, pool_ptr, table_ptr, out, B, F, Tp, fe, **null):
    p = dict(pool=pool_ptr, table=table_ptr, batch=out["batch"].data_ptr(), fi=out["fi"].data_ptr(), obs=out["obs"].data_ptr(),
             lat=out["lat"].data_ptr())
    p.update(null)
    rc = nat.lib().lfvdm_prepare_batch(p["pool"], p["table"], p["batch"], p["fi"], p["obs"], p["lat"], B, F, Tp, fe, nat.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("B,F,Tp,fe", tg.GATHER_CASES)
def test_prepare_batch_is_the_host_gather(nat, B, F, Tp, fe):
    """Frames, sign-extended int64 indices and 0 / 1 masks, for the ordinary and the adversarial table of the shape; the
    guard bands around the batch survive; a second launch on the same buffers gives the same words."""
    pool = tg.gather_pool(B, F, Tp, fe)
    pd = pool.cuda()
    for name, table in tg.gather_tables(B, F, Tp, fe).items():
        td = table.cuda()
        out = _gather_outputs(B, F, fe)
        want = tg.gather_ref(pool, table)
        first = None
        for launch in range(2):
            assert _gather_launch(nat, pd.data_ptr(), td.data_ptr(), out, B, F, Tp, fe) == 0
            got = (out["batch"].view(B, F, fe), out["fi"], out["obs"], out["lat"])
            for g, w, what in zip(got, want, ("frames", "frame indices", "observed mask", "latent mask")):
                counted("gather", g.dtype == w.dtype and same_bits(g, w), f"{name} table, launch {launch}: {what}")
            counted("gather", guards_intact(out["buf"], B * F * fe), f"{name} table: guard band around the batch")
            words = [bits(out[k]).clone() for k in ("buf", "fi", "obs", "lat")]
            if first is not None:
                counted("gather", all(torch.equal(a, b) for a, b in zip(first, words)), "second launch differs")
            first = words


def test_prepare_batch_refusals_write_nothing(nat):
    B, F, Tp, fe = 2, 3, 4, 8
    pool = torch.zeros(B * Tp * fe + 8, device="cuda")
    table = torch.zeros(B, F, 4, dtype=torch.int32, device="cuda")
    out = _gather_outputs(B, F, fe)
    before = {k: bits(v).clone() for k, v in out.items()}
    pp, tp = pool.data_ptr(), table.data_ptr()
    assert _gather_launch(nat, pp, tp, out, B, F, Tp, fe) == 0          # the same call, accepted
    out = _gather_outputs(B, F, fe)
    refused = [("pool + 4 bytes", dict(pool=pp + 4), (B, F, Tp, fe)), ("batch + 4 bytes", dict(batch=out["batch"].data_ptr() + 4), (B, F, Tp, fe)),
               ("frame_elems = 6", {}, (B, F, Tp, 6)), ("B = 65536", {}, (65536, F, Tp, fe)), ("F = 0", {}, (B, 0, Tp, fe))]
    refused += [(f"{k} = NULL", {k: None}, (B, F, Tp, fe)) for k in ("pool", "table", "batch", "fi", "obs", "lat")]
    for what, null, shape in refused:
        counted("gather", _gather_launch(nat, pp, tp, out, *shape, **null) == E_SHAPE, what)
        for k, v in out.items():
            counted("gather", torch.equal(bits(v), before[k]), f"{what}: the refused call wrote {k}")


# ------------------------------------------------------------------------------------------------------------------------
# 2. ordered slab reduction
# ------------------------------------------------------------------------------------------------------------------------
def _reduce_run(nat, dst0, slab, od, os_):
    """dst0 / slab (device) into buffers whose views start od / os_ floats behind a 16-byte boundary -> (got, buffers ok)."""
    parts, n = slab.shape
    dbuf, dst = guarded(dst0, before=od)
    sbuf, sl = guarded(slab, before=os_)
    assert dbuf.data_ptr() % 16 == 0 and sbuf.data_ptr() % 16 == 0
    slab_words = bits(sbuf).clone()
    rc = nat.lib().lfvdm_det_reduce(dst.data_ptr(), sl.data_ptr(), n, parts, nat.stream())
    torch.cuda.synchronize()
    assert rc == 0
    ok = guards_intact(dbuf, n, od) and torch.equal(bits(sbuf), slab_words)
    return dst.clone(), ok


@pytest.mark.parametrize("n,parts,od,os_", tg.REDUCE_SMALL)
def test_det_reduce_is_the_sequential_sum(nat, n, parts, od, os_):
    """Both kernels, every remainder of the four-loads-in-flight unroll, the scalar kernel through n % 4 and through either
    misaligned pointer: the words of dst0 + slab[0] + slab[1] + ... in that order (host loop and device loop)."""
    dst0, slab = tg.reduce_inputs(n, parts)
    got, ok = _reduce_run(nat, dst0.cuda(), slab.cuda(), od, os_)
    counted("reduce", same_bits(got, tg.reduce_ref(dst0, slab)), "host loop")
    want = dst0.cuda()
    for p in range(parts):
        want += slab[p].cuda()
    counted("reduce", same_bits(got, want), "device loop")
    counted("reduce", ok, "guard bands / the slab changed")


@pytest.mark.parametrize("n,parts,od,os_", tg.REDUCE_LARGE)
def test_det_reduce_second_trip_of_the_capped_grid(nat, n, parts, od, os_):
    """More elements than 4096 workgroups cover in one trip (float4 body: 100 threads, scalar body: 101 threads go round
    again).  Inputs generated on the device; every element behind the first trip must have moved."""
    g = torch.Generator(device="cuda").manual_seed(n)
    scale = torch.tensor([tg.ROW_SCALE[p % 3] for p in range(parts)], device="cuda")[:, None]
    slab = torch.randn(parts, n, device="cuda", generator=g) * scale
    dst0 = torch.randn(n, device="cuda", generator=g)
    got, ok = _reduce_run(nat, dst0, slab, od, os_)
    want = dst0.clone()
    for p in range(parts):
        want += slab[p]
    counted("reduce", torch.equal(bits(got), bits(want)), "device loop")
    first = tg.reduce_first_trip(n, parts, od, os_)
    counted("reduce", n - first in (400, 101) and bool((got[first:] != dst0[first:]).all()), "elements behind the first trip kept dst0")
    counted("reduce", ok, "guard bands / the slab changed")


def test_det_reduce_refusals_write_nothing(nat):
    dbuf, dst = guarded(rnd("tg/rr/d", 16))
    sbuf, slab = guarded(rnd("tg/rr/s", 3, 16))
    before = bits(dbuf).clone(), bits(sbuf).clone()
    L, s = nat.lib(), nat.stream()
    for what, args in (("n = 0", (dst.data_ptr(), slab.data_ptr(), 0, 3)), ("parts = 0", (dst.data_ptr(), slab.data_ptr(), 16, 0)),
                       ("dst = NULL", (None, slab.data_ptr(), 16, 3)), ("slab = NULL", (dst.data_ptr(), None, 16, 3))):
        counted("reduce", L.lfvdm_det_reduce(*args, s) == E_SHAPE, what)
        torch.cuda.synchronize()
        counted("reduce", torch.equal(bits(dbuf), before[0]) and torch.equal(bits(sbuf), before[1]), f"{what}: the refused call wrote")


# ------------------------------------------------------------------------------------------------------------------------
# 3. the two-destination reduction through its callers
# ------------------------------------------------------------------------------------------------------------------------
RATIO = {}


def bounded(tag, got, want, bound):
    ratio = float((got.detach().cpu().double() - want).abs().max()) / bound
    RATIO[tag] = max(RATIO.get(tag, 0.0), ratio)
    print(f"[err/bound] {tag}: {ratio:.3f}")
    counted("reduce2", ratio <= 1.0, f"{tag}: err/bound = {ratio:.3f}")


def _wgrad_case(N, Cin, Cout, H, k):
    tag = f"tg/wgrad/{N}/{Cin}/{Cout}/{H}/{k}"
    inputs = dict(x=rnd(tag + "/x", N * H * H, Cin), w=rnd(tag + "/w", Cout, Cin, k, k) * (Cin * k * k) ** -0.5, b=0.1 * rnd(tag + "/b", Cout))
    fn = lambda t, h, w: to_rows(F.conv2d(nchw(t["x"], N, h, w), t["w"], t["b"], padding=k // 2))
    return Case(tag, inputs, fn, dict(out="igemm", dx="igemm", dw="wgrad", db="wgrad"), (N * H * H, Cout), (H, H))


@pytest.mark.parametrize("N,Cin,Cout,H,k,db_off", [(2, 32, 3, 4, 3, 0), (3, 64, 36, 4, 1, 0), (2, 32, 32, 5, 3, 1)])
def test_conv_wgrad_slab_accumulates_both_destinations(nat, N, Cin, Cout, H, k, db_off):
    """The wave-private weight-gradient kernel with a slab and a bias gradient: det_reduce2_kernel folds the slices into the
    packed weight gradient (float4 pair) and the bias gradient (Cout = 3: scalar pair; 36: float4 pair; 32 one float off a
    16-byte boundary: scalar pair) ON TOP of what they held.  Slab capacities: exactly one pixel slice, and ample (as many
    slices as the launcher wants: one where the map has 32 pixels, two otherwise)."""
    case = _wgrad_case(N, Cin, Cout, H, k)
    ldr = (Cout + 3) // 4 * 4
    dout = torch.zeros(N * H * H, ldr)
    dout[:, :Cout] = case.probe
    x, doutd = case.inputs["x"].cuda(), dout.cuda()
    gp0, db0 = rnd(case.tag + "/gp0", Cout, k * k, Cin), rnd(case.tag + "/db0", Cout)
    gbuf, gp = guarded(gp0)
    bbuf, db = guarded(db0, before=GUARD + db_off)
    assert (db.data_ptr() % 16 != 0) == bool(db_off)
    a = nat.fill_conv_args(src0=x, C0=Cin, N=N, Hs=H, Ws=H, Ho=H, Wo=H, ksize=k, res=doutd, ldr=ldr, out=gp, bias=db, Cout=Cout)
    assert nat._wgrad_codes(a) == [], "the wave-private kernel"
    want_w = gp0.double() + case.ref["dw"].permute(0, 2, 3, 1).reshape(Cout, k * k, Cin)
    want_b = db0.double() + case.ref["db"]
    per = Cout * k * k * Cin + Cout
    for cap in (per, 8 * per):
        ws = torch.full((cap + GUARD,), NAN, device="cuda")
        a.splitk_ws, a.splitk_ws_floats = ws.data_ptr(), cap
        runs = []
        for _ in range(2):
            gp.copy_(gp0.reshape(-1)); db.copy_(db0)
            nat.check(nat.lib().lfvdm_conv_wgrad(C.byref(a), nat.stream()), f"lfvdm_conv_wgrad cap {cap}")
            torch.cuda.synchronize()
            runs.append((bits(gbuf).clone(), bits(bbuf).clone()))
        counted("reduce2", torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"cap {cap}: not repeatable")
        bounded(f"wgrad {Cout}x{Cin}x{k} cap {cap // per} dW", gp.view(Cout, k * k, Cin), want_w, case.bound("dw", want_w))
        bounded(f"wgrad {Cout}x{Cin}x{k} cap {cap // per} db", db, want_b, case.bound("db", want_b))
        counted("reduce2", guards_intact(gbuf, gp.numel()) and guards_intact(bbuf, Cout, GUARD + db_off), f"cap {cap}: guard bands")
        counted("reduce2", bool(torch.isnan(ws[cap:]).all()), f"cap {cap}: wrote past the slab")
        slices = 1 if (cap == per or N * H * H <= 32) else 2
        counted("reduce2", int((~torch.isnan(ws[:cap])).sum()) == slices * per, f"cap {cap}: {slices} slab rows expected")


@pytest.mark.parametrize("B,T,P,C", [(1, 5, 3, 32), (2, 6, 7, 32), (1, 5, 3, 96), (2, 6, 7, 96)])
def test_gn_temporal_det_accumulates_both_destinations(nat, B, T, P, C):
    """lfvdm_gn_temporal_bwd_det: one workgroup ((1, ., 3): one slab row) and several ((2, ., 7): four); dgamma and dbeta
    are added to what they held (bound of test_gn_temporal_backward_every_kernel), bitwise repeatable."""
    tag = f"tg/gnt/{B}/{T}/{P}/{C}"
    x, dy = rnd(tag + "/x", B * T * P, C) * 1.2 + 0.3, rnd(tag + "/dy", B * T * P, C)
    gamma = 1 + 0.1 * rnd(tag + "/g", C)
    xr = _gnt_columns(x, B, T, P, C).requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.group_norm(xr, 32, gr, br, eps=1e-5).backward(_gnt_columns(dy, B, T, P, C))
    g0, b0 = rnd(tag + "/g0", C), rnd(tag + "/b0", C)
    tol_g, tol_b = 1e-4 * max(1.0, float(gr.grad.abs().max())), 1e-4 * max(1.0, float(br.grad.abs().max()))
    nwg = -(-(B * P) // 4)
    assert nwg == (1 if B == 1 else 4)
    need = 2 * nwg * C
    ws = torch.full((need + GUARD,), NAN, device="cuda")
    xc, dyc, gc = x.cuda(), dy.cuda(), gamma.cuda()
    runs = []
    for _ in range(2):
        dx = torch.full((B * T * P, C), NAN, device="cuda")
        gbuf, dg = guarded(g0)
        bbuf, db = guarded(b0)
        nat.check(nat.lib().lfvdm_gn_temporal_bwd_det(nat.ptr(xc), nat.ptr(dyc), nat.ptr(gc), 1e-5, nat.ptr(dx), dg.data_ptr(), db.data_ptr(),
                                                      B, T, P, C, 0, ws.data_ptr(), need, nat.stream()), "lfvdm_gn_temporal_bwd_det")
        torch.cuda.synchronize()
        runs.append((bits(dx).clone(), bits(gbuf).clone(), bits(bbuf).clone()))
    counted("reduce2", all(torch.equal(u, v) for u, v in zip(*runs)), "not repeatable")
    bounded(f"gn temporal C{C} nwg{nwg} dgamma", dg, g0.double() + gr.grad, tol_g)
    bounded(f"gn temporal C{C} nwg{nwg} dbeta", db, b0.double() + br.grad, tol_b)
    counted("reduce2", guards_intact(gbuf, C) and guards_intact(bbuf, C) and bool(torch.isnan(ws[need:]).all()), "guard bands")


@pytest.mark.parametrize("C,chunked", [(32, False), (32, True), (96, False), (96, True)])
def test_gn_bwd_deterministic_parameter_gradients_accumulate(nat, monkeypatch, C, chunked):
    """lfvdm_gn_bwd in deterministic mode (sums_out + lfvdm_gn_param_grads; chunked: its workspace, several workgroups per
    sample): dgamma / dbeta onto preloaded .grad within test_norm_backward_gpu's 2e-4 |ref|max, bitwise repeatable."""
    from improved_diffusion import _backward as bw
    monkeypatch.setenv("LFVDM_DETERMINISTIC", "1")
    N, T, act = 2, 1, 1
    P = 16 * _pl(C) + 1 if chunked else 16
    assert (nat.lib().lfvdm_gn_bwd_ws_floats(C, N, P) > 0) == chunked
    tag = f"tg/gnb/{C}/{P}"
    a = rnd(tag + "/a", N * P, C) * 1.3 + 0.7
    gamma, beta = 1 + 0.1 * rnd(tag + "/g", C), 0.1 * rnd(tag + "/be", C)
    da = rnd(tag + "/da", N * P, C)
    _, g_ref, b_ref, _ = _gn_reference(a, None, C, 0, N, P, gamma, beta, None, T, act, da)
    gpar, bpar = torch.nn.Parameter(gamma.cuda()), torch.nn.Parameter(beta.cuda())
    ac, dac = a.cuda(), da.cuda()
    _, cA, cB, st = bw._gn_apply(ac, None, C, 0, N, P, gpar.detach(), bpar.detach(), None, T, act)
    g_pre, b_pre = rnd(tag + "/gpre", C), rnd(tag + "/bpre", C)
    runs = []
    for _ in range(2):
        gpar.grad, bpar.grad = g_pre.cuda(), b_pre.cuda()
        bw._gn_backward(dac, ac, None, C, 0, N, P, cA, cB, st, act, gpar, bpar, None, T, dfilm_out=None, inplace=True)
        torch.cuda.synchronize()
        runs.append((gpar.grad.clone(), bpar.grad.clone()))
    counted("reduce2", torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "not repeatable")
    bounded(f"gn_bwd C{C} P{P} dgamma", runs[0][0], g_ref + g_pre.double(), 2e-4 * float(g_ref.abs().max()))
    bounded(f"gn_bwd C{C} P{P} dbeta", runs[0][1], b_ref + b_pre.double(), 2e-4 * float(b_ref.abs().max()))


# ------------------------------------------------------------------------------------------------------------------------
# 4. grouped pack / unpack and the single-tensor forms
# ------------------------------------------------------------------------------------------------------------------------
def _pack_launch(nat, jobs):
    ws = [tg.pack_weight(j) for j in jobs]
    wd = [w.cuda() for w in ws]
    dst = [tg.pack_prefill(j).cuda() for j in jobs]
    table, blk = [], 0
    for j, w, d in zip(jobs, wd, dst):
        Cout, Cin, k, tr, ld = j
        table.append(nat.PackJob(w.data_ptr(), d.data_ptr(), Cout, Cin, k * k, tr, blk, ld))
        blk += tg.pack_tiles(Cout, Cin)
    dev = nat.jobs_to_device(table, "cuda")
    nat.check(nat.lib().lfvdm_pack_conv_weights(dev.data_ptr(), len(jobs), blk, nat.stream()), "lfvdm_pack_conv_weights")
    torch.cuda.synchronize()
    for j, w, d in zip(jobs, ws, dst):
        counted("pack", same_bits(d, tg.pack_expected(j, w)), f"pack job {j}")


def test_grouped_pack_ragged_padded_and_wide(nat):
    """One launch with every job of PACK_JOBS (the first has one tile), then a single-job launch: every real element is the
    host permutation, every padding column and the guard band still hold the sentinel."""
    _pack_launch(nat, tg.PACK_JOBS)
    _pack_launch(nat, [tg.PACK_SINGLE])


def _unpack_buffers():
    bufs = []
    for j, job in enumerate(tg.UNPACK_JOBS):
        g0, gp0 = tg.unpack_inputs(j, job)
        bufs.append((g0, gp0) + guarded(g0) + guarded(gp0))
    return bufs


def test_grouped_unpack_is_one_add_per_element(nat):
    """Six jobs in one launch - 9 taps and 1 tap, ragged Cin, ldp > Cin, a 9216-float row, a one-float row - with
    max_row_floats exactly the largest row: g == g0 + unpack(gp0) in words, every float of gp (padding included) +0.0."""
    bufs = _unpack_buffers()
    table, row0 = [], 0
    for (Cout, Cin, taps, ldp), (_, _, gbuf, g, pbuf, gp) in zip(tg.UNPACK_JOBS, bufs):
        table.append(nat.UnpackJob(gp.data_ptr(), g.data_ptr(), Cout, Cin, taps, row0, ldp))
        row0 += Cout
    dev = nat.jobs_to_device(table, "cuda")
    nat.check(nat.lib().lfvdm_unpack_conv_grads(dev.data_ptr(), len(table), row0, tg.UNPACK_MAX_ROW, nat.stream()), "lfvdm_unpack_conv_grads")
    torch.cuda.synchronize()
    for j, (job, (g0, gp0, gbuf, g, pbuf, gp)) in enumerate(zip(tg.UNPACK_JOBS, bufs)):
        want_g, want_gp = tg.unpack_ref(j, job, g0, gp0)
        counted("pack", same_bits(g.view(g0.shape), want_g), f"unpack job {job}: g")
        counted("pack", same_bits(gp.view(gp0.shape), want_gp), f"unpack job {job}: gp not +0.0 everywhere")
        counted("pack", guards_intact(gbuf, g0.numel()) and guards_intact(pbuf, gp0.numel()), f"unpack job {job}: guard bands")
    # refusals
    bufs = _unpack_buffers()
    table = nat.jobs_to_device([nat.UnpackJob(b[5].data_ptr(), b[3].data_ptr(), *job[:3], 0, job[3]) for job, b in zip(tg.UNPACK_JOBS[:1], bufs)], "cuda")
    before = [(bits(b[2]).clone(), bits(b[4]).clone()) for b in bufs]
    L, s = nat.lib(), nat.stream()
    for what, args, code in (("max_row_floats = 16385", (table.data_ptr(), 1, 64, 16385), E_UNSUPPORTED), ("0 jobs", (table.data_ptr(), 0, 64, 288), E_SHAPE),
                             ("0 rows", (table.data_ptr(), 1, 0, 288), E_SHAPE), ("no table", (None, 1, 64, 288), E_SHAPE)):
        counted("pack", L.lfvdm_unpack_conv_grads(*args, s) == code, what)
        torch.cuda.synchronize()
        counted("pack", all(torch.equal(bits(b[2]), w[0]) and torch.equal(bits(b[4]), w[1]) for b, w in zip(bufs, before)), f"{what}: wrote")
    for what, args in (("pack: 0 jobs", (table.data_ptr(), 0, 1)), ("pack: 0 blocks", (table.data_ptr(), 1, 0)), ("pack: no table", (None, 1, 1))):
        counted("pack", L.lfvdm_pack_conv_weights(*args, s) == E_SHAPE, what)


@pytest.mark.parametrize("Cout,Cin,k", [(600, 300, 3), (3, 5, 1)])
def test_single_tensor_pack_and_unpack(nat, Cout, Cin, k):
    """(600, 300, 3): 1.62 M elements, more than 2048 workgroups of 256 - the grid-stride loops wrap.  accumulate = 0 into a
    NaN-filled gradient leaves no NaN; accumulate = 1 is one add per element."""
    w = rnd(f"tg/single/{Cout}/{Cin}/{k}", Cout, Cin, k, k)
    wd = w.cuda()
    n = w.numel()
    assert (n + 255) // 256 > 2048 or Cout == 3
    obuf, o = guarded(n)
    nat.pack_conv_weight(wd, o)
    torch.cuda.synchronize()
    counted("pack", same_bits(o, w.permute(0, 2, 3, 1).reshape(-1)) and guards_intact(obuf, n), "lfvdm_pack_conv_weight")
    tbuf, t = guarded(n)
    nat.pack_conv_weight_t(wd, t)
    torch.cuda.synchronize()
    counted("pack", same_bits(t, w.flip(2, 3).permute(1, 2, 3, 0).reshape(-1)) and guards_intact(tbuf, n), "lfvdm_pack_conv_weight_t")
    gp = rnd(f"tg/single/{Cout}/{Cin}/{k}/gp", Cout, k * k, Cin)
    unpacked = gp.permute(0, 2, 1).reshape(Cout, Cin, k, k)
    gbuf, g = guarded(n)
    nat.unpack_conv_grad(gp.cuda(), g.view(Cout, Cin, k, k), 0)
    torch.cuda.synchronize()
    counted("pack", not bool(torch.isnan(g).any()) and same_bits(g.view(w.shape), unpacked) and guards_intact(gbuf, n), "accumulate = 0")
    g0 = rnd(f"tg/single/{Cout}/{Cin}/{k}/g0", Cout, Cin, k, k)
    gbuf, g = guarded(g0)
    nat.unpack_conv_grad(gp.cuda(), g.view(Cout, Cin, k, k), 1)
    torch.cuda.synchronize()
    counted("pack", same_bits(g.view(w.shape), g0 + unpacked) and guards_intact(gbuf, n), "accumulate = 1")
    # refusals: nothing written
    L, s = nat.lib(), nat.stream()
    rbuf, r = guarded(n)
    for what, shape in (("ksize = 2", (Cout, Cin, 2)), ("Cout = 0", (0, Cin, k))):
        counted("pack", L.lfvdm_pack_conv_weight(wd.data_ptr(), r.data_ptr(), *shape, s) == E_SHAPE, what)
        counted("pack", L.lfvdm_pack_conv_weight_t(wd.data_ptr(), r.data_ptr(), *shape, s) == E_SHAPE, what)
        counted("pack", L.lfvdm_unpack_conv_grad(wd.data_ptr(), r.data_ptr(), *shape, 0, s) == E_SHAPE, what)
        torch.cuda.synchronize()
        counted("pack", bool(torch.isnan(r).all()) and guards_intact(rbuf, n), f"{what}: wrote")


# ------------------------------------------------------------------------------------------------------------------------
# 5. lfvdm_conv_igemm_config
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Cin,Cout,H", [(3, 64, 64, 16), (5, 128, 96, 8), (40, 256, 128, 2), (2, 32, 4, 16), (1, 64, 192, 5)])
def test_conv_igemm_config_is_a_host_query(nat, N, Cin, Cout, H):
    """The shapes of test_conv3x3_plain: LFVDM_OK with a template instance at code 0 and at every candidate code, nothing
    launched (the NaN output stays), Cin = 0 refused."""
    L = nat.lib()
    x, w, b = torch.zeros(N * H * H, Cin, device="cuda"), torch.zeros(Cout, 9, Cin, device="cuda"), torch.zeros(Cout, device="cuda")
    out = torch.full((N * H * H, Cout), NAN, device="cuda")
    a = nat.fill_conv_args(src0=x, C0=Cin, N=N, Hs=H, Ws=H, Ho=H, Wo=H, W=w, bias=b, Cout=Cout, out=out, ldo=Cout)
    ws, cnt = nat.splitk_workspace(out.device)
    a.splitk_ws, a.splitk_cnt, a.splitk_ws_floats, a.splitk_cnt_ints = ws.data_ptr(), cnt.data_ptr(), ws.numel(), cnt.numel()
    codes = (C.c_int * 512)()
    ncodes = L.lfvdm_conv_igemm_candidates(C.byref(a), codes, 512)
    assert 0 < ncodes <= 512
    for code in [0] + list(codes[:ncodes]):
        a.tune = code
        nt, nw = C.c_int(-1), C.c_int(-1)
        counted("config", L.lfvdm_conv_igemm_config(C.byref(a), C.byref(nt), C.byref(nw)) == 0 and nt.value > 0 and nw.value > 0, f"code {code}")
    a.tune, a.C0 = 0, 0
    nt, nw = C.c_int(-1), C.c_int(-1)
    counted("config", L.lfvdm_conv_igemm_config(C.byref(a), C.byref(nt), C.byref(nw)) == E_SHAPE and nt.value == -1 and nw.value == -1, "Cin = 0")
    torch.cuda.synchronize()
    counted("config", bool(torch.isnan(out).all()), "the query launched something")


def test_report_comparisons():
    print("[train glue] comparisons per section:", dict(sorted(COUNT.items())))
    print("[train glue] worst err/bound of section 3:", {k: round(v, 3) for k, v in sorted(RATIO.items())})
