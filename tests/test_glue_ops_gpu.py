"""Direct fp64 parity of the small kernels every sampler step and every training step runs: lfvdm_rowdot (all three input
modes), lfvdm_silu, every lfvdm_conv_in instance, the sampler's clock (lfvdm_conv_in_tick, lfvdm_sampler_tick_fetch),
lfvdm_compose_rows, lfvdm_prepare_batch and lfvdm_q_sample.

Every reference is plain torch / numpy in float64 on the CPU, computed from the very float32 operands the kernel reads.
Every bound is evaluated per output element from those operands (u = 2^-24, the float32 unit roundoff); none is a measured
figure.  Every output buffer starts as NaN, padding and guard elements as a sentinel that must survive bit for bit.  The
case builders (``*_case`` / ``*_ref``) touch no GPU, so the references can be exercised on their own.  GPU only."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from test_ops_gpu import rnd, close, cl, from_cl

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                  # float32 unit roundoff: one rounding moves a value by at most U * |value|
NAN = float("nan")
SENT = -724531.25               # exactly representable; no kernel under test produces it


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from improved_diffusion import _native
    _native.lib()
    return _native


def bits(t):
    """The raw words of a float32 / int tensor, on the CPU (NaN-safe equality)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def within(tag, got, ref, bound):
    """|got - ref| <= bound element by element; prints the worst error / bound ratio first.  NaN (an element never
    written, or a padding NaN read) and inf fail."""
    g = got.detach().cpu().double()
    assert g.shape == ref.shape, (tag, g.shape, ref.shape)
    assert not torch.isnan(g).any(), f"{tag}: NaN in the output"
    err = (g - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    worst = float(ratio.max())
    print(f"[err/bound] {tag}: {worst:.3f}")
    assert bool((err <= bound).all()), f"{tag}: err/bound = {worst:.3f} at flat index {int(ratio.argmax())}"


def silu64(x):
    x = x.double()
    return x / (1.0 + torch.exp(-x))


def silu_rel(x):
    """Relative bound of the embedding kernels' SiLU, x * v_rcp(1 + v_exp(-x * log2e)): the rounding of x * log2e moves the
    exponent by at most |x| U; v_exp, v_rcp, the add and the multiply give one more each."""
    return (x.double().abs() + 4.0) * U


# ------------------------------------------------------------------------------------------------------------------------
# 1. lfvdm_rowdot, in_mode 0 and 1
# ------------------------------------------------------------------------------------------------------------------------
def dot_mult(K):
    """Roundings a product passes before it reaches the output of rowdot_kernel: its own, the three adds of its group of
    four, one add into the lane's accumulator per later k pass (ceil(K / 256) passes), six shuffle steps and the bias -
    ceil(K / 256) + 11.  Charged as four per pass + 6 + 3, which is K / 64 + 6 + 3 at the multiples of 256 and never below
    the count above."""
    return 4 * math.ceil(K / 256) + 6 + 3


def rowdot_ref(W, b, x, mode):
    """fp64 out[m][o] = sum_k act(x[m][k]) W[o][k] + b[o] and its bound dot_mult(K) U sum|w v| + U |ref|
    (+ sum_k silu_rel(x_k) |w_k v_k| in in_mode 1)."""
    Wd, xd = W.double(), x.double()
    v = silu64(xd) if mode == 1 else xd
    ref = v @ Wd.T
    if b is not None:
        ref = ref + b.double()
    bound = dot_mult(W.shape[1]) * U * (v.abs() @ Wd.abs().T) + U * ref.abs()
    if mode == 1:
        bound = bound + (silu_rel(x) * v.abs()) @ Wd.abs().T
    return ref, bound


ROWDOT_JOBS = ((5, True, 8, 4), (96, False, 0, 0), (2, True, 0, 0))          # O, bias, ldin - K, ldout - O


def rowdot_case(M, K):
    jobs = []
    for j, (O, has_b, pin, pout) in enumerate(ROWDOT_JOBS):
        tag = f"glue/rd/{M}/{K}/{j}"
        jobs.append(dict(W=rnd(tag + "/w", O, K, scale=K ** -0.5), b=rnd(tag + "/b", O, scale=0.5) if has_b else None,
                         x=rnd(tag + "/x", M, K, scale=2.0), O=O, ldin=K + pin, ldout=O + pout))
    return jobs


def padded(x, ld, fill):
    out = torch.full((x.shape[0], ld), fill, dtype=x.dtype)
    out[:, :x.shape[1]] = x
    return out


def launch_rowdot(nat, recs):
    """recs: (W, b or None, in, out, K, O, M, ldin, ldout, in_mode) with device tensors; row0 is the running sum of O."""
    jobs, row0 = [], 0
    for W, b, inp, out, K, O, M, ldin, ldout, mode in recs:
        jobs.append(nat.RowdotJob(W.data_ptr(), b.data_ptr() if b is not None else None, inp.data_ptr(), out.data_ptr(), K, O, M,
                                  ldin, ldout, mode, row0, 0))
        row0 += O
    nat.rowdot(nat.jobs_to_device(jobs, "cuda"), len(jobs), row0)
    torch.cuda.synchronize()
    return row0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", [32, 64, 256, 260, 1024])
@pytest.mark.parametrize("M", [1, 8, 9, 17])
def test_rowdot_fp64(nat, M, K, mode):
    """rowdot_kernel, in_mode 0 / 1, three jobs in one launch with O = 5, 96, 2: row0 = 0, 5, 101 and 103 rows, so the first
    4-wave workgroup holds waves of two jobs and the last one holds three live waves and one that returns.  M = 9 and 17
    take a second and third trip of the m0 loop and leave it through the `break` (one live row of eight); K = 260 and 1024
    take more than one k pass (K = 260: lane 0 alone), K = 32 and 64 leave 56 / 48 lanes without work.  Job 0 has
    ldin = K + 8 (NaN in the padding: reading it shows) and ldout = O + 4 (sentinel: must survive), job 1 a NULL bias.
    Bound: see dot_mult and rowdot_ref."""
    case = rowdot_case(M, K)
    recs, outs = [], []
    for J in case:
        out = torch.full((M, J["ldout"]), NAN)
        out[:, J["O"]:] = SENT
        outs.append(out.cuda())
        recs.append((J["W"].cuda(), J["b"].cuda() if J["b"] is not None else None, padded(J["x"], J["ldin"], NAN).cuda(), outs[-1],
                     K, J["O"], M, J["ldin"], J["ldout"], mode))
    assert launch_rowdot(nat, recs) == 103
    for j, (J, out) in enumerate(zip(case, outs)):
        ref, bound = rowdot_ref(J["W"], J["b"], J["x"], mode)
        within(f"rowdot M={M} K={K} mode={mode} job {j}", out[:, :J["O"]], ref, bound)
        assert same_bits(out[:, J["O"]:], torch.full((M, J["ldout"] - J["O"]), SENT)), f"job {j}: ldout padding written"


# ------------------------------------------------------------------------------------------------------------------------
# 2. lfvdm_rowdot, in_mode 2: the sinusoidal embedding
# ------------------------------------------------------------------------------------------------------------------------
def sinus_timesteps():
    """Every integer timestep, the model timesteps of a 250-step respacing (t * 1000 / 250), and fractional ones."""
    return np.concatenate([np.arange(1000.0), np.arange(250.0) * (1000.0 / 250), [999.75, 37.5]]).astype(np.float32)


def sinus_freqs(K):
    half = K // 2
    return torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)


def sinus_ref(t, fr, W, b):
    """[cos(a) | sin(a)] W^T + b in fp64 with a = float32(t) * float32(fr), the one rounding the kernel makes too.
    Bound: cosf / sinf within 4 U of the true value (2 ulp of a value below 1), times sum|w|, plus the dot product's."""
    arg = t[:, None] * fr.numpy()[None, :]
    assert arg.dtype == np.float32
    a = torch.from_numpy(arg.astype(np.float64))
    emb = torch.cat([a.cos(), a.sin()], 1)
    Wd = W.double()
    ref = emb @ Wd.T + b.double()
    bound = 4 * U * Wd.abs().sum(1)[None, :] + dot_mult(W.shape[1]) * U * (emb.abs() @ Wd.abs().T) + U * ref.abs()
    return ref, bound


def sinus_case(K, O=11):
    tag = f"glue/sin/{K}"
    return sinus_timesteps(), sinus_freqs(K), rnd(tag + "/w", O, K, scale=K ** -0.5), rnd(tag + "/b", O, scale=0.5)


@pytest.mark.parametrize("K", [32, 36, 64, 128, 256])
def test_rowdot_sinusoid_every_timestep(nat, K):
    """rowdot_kernel, in_mode 2, K = ch of the models plus K = 36: M = 1252 timesteps (0..999, the 250-step respacing's,
    999.75, 37.5), so 157 trips of the m0 loop; 11 output rows leave a ragged last workgroup.  half = K / 2 = 16, 32, 64,
    128 puts the [cos | sin] seam on a lane boundary; K = 36 (half = 18) puts it inside the float4 of lane 4 (k = 16..19:
    two cosines, then the sines of the first two frequencies).  Input as the engine lays it out: timesteps, padding (NaN)
    up to ldin, K / 2 frequencies.  Bound: see sinus_ref."""
    t, fr, W, b = sinus_case(K)
    M, O = len(t), W.shape[0]
    ldin = (M + 7) // 8 * 8 + 8
    tin = torch.cat([torch.from_numpy(t), torch.full((ldin - M,), NAN), fr]).cuda()
    out = torch.full((M, O), NAN, device="cuda")
    launch_rowdot(nat, [(W.cuda(), b.cuda(), tin, out, K, O, M, ldin, O, 2)])
    ref, bound = sinus_ref(t, fr, W, b)
    within(f"sinusoid K={K}", out, ref, bound)


# ------------------------------------------------------------------------------------------------------------------------
# 3. lfvdm_silu
# ------------------------------------------------------------------------------------------------------------------------
SILU_N = 4 * (4096 * 256 + 257)
SILU_SPECIAL = [0.0, -0.0, 87.5, -87.5, 88.8, -88.8, -104.0, 104.0, 1.17549435e-38, -1.17549435e-38, 1e-40, -1e-40]


def silu_case():
    """[-110, 110] swept over SILU_N points; the special values sit at the head and again inside the last 1028 floats, the
    part the second grid-stride pass handles."""
    x = torch.linspace(-110.0, 110.0, SILU_N, dtype=torch.float64).float()
    sp = torch.tensor(SILU_SPECIAL, dtype=torch.float32)
    x[:len(sp)] = sp
    x[SILU_N - 1000:SILU_N - 1000 + len(sp)] = sp
    return x


def silu_ref(x):
    ref = silu64(x)
    return ref, silu_rel(x) * ref.abs() + 1e-37


def test_silu_fp64(nat):
    """silu_kernel at n = 4 (4096 * 256 + 257) floats: the grid is capped at 4096 workgroups and 257 threads take a second
    grid-stride trip.  Saturating inputs: e^-x overflows below -88.72, 1 / (1 + e^-x) is denormal below -87.34, e^-x
    underflows above 87.3; +-0, the smallest normal and a denormal.  Relative bound silu_rel (|x| + 4) U, absolute floor
    1e-37.  The plain x * v_rcp(1 + __expf(-x)) misses this twice, hence silu_full_f: between -89.7 and -87.34 the true
    value, up to 1.03e-36 in size, is a normal float above the floor and it returned 0 (10.3 times the bound at -87.34);
    and __expf's one-float log2(e) adds 0.22 |x| U to the |x| U of the rounding (1.16 times the bound at -44.68, just below
    a power of two of x log2(e), where the rounding alone can use up |x| U).  The 8 floats behind the output keep their
    sentinel; n % 4 != 0 is refused and writes nothing."""
    x = silu_case()
    out = torch.full((SILU_N + 8,), NAN, device="cuda")
    out[SILU_N:] = SENT
    xd = x.cuda()
    L = nat.lib()
    assert L.lfvdm_silu(xd.data_ptr(), out.data_ptr(), SILU_N, nat.stream()) == 0
    torch.cuda.synchronize()
    ref, bound = silu_ref(x)
    within("silu", out[:SILU_N], ref, bound)
    assert same_bits(out[SILU_N:], torch.full((8,), SENT)), "written past n"
    out2 = torch.full((16,), NAN, device="cuda")
    for n in (6, 7, 0):
        assert L.lfvdm_silu(xd.data_ptr(), out2.data_ptr(), n, nat.stream()) != 0, n
    torch.cuda.synchronize()
    assert same_bits(out2, torch.full((16,), NAN)), "a refused call wrote"


def test_silu_then_rowdot_is_rowdot_silu(nat):
    """What _engine.Plan.build_time_tables relies on: lfvdm_silu followed by rowdot in in_mode 0 gives the bits of rowdot in
    in_mode 1 on the raw input (both inline silu_full_f; the accumulation order is the same).  M = 17, K = 260, O = 96 with
    ldin = K + 8: three m0 trips, two k passes.  The in_mode 1 result is held to the bound of rowdot_ref as well."""
    M, K, O, ldin = 17, 260, 96, 268
    W, b, x = rnd("glue/sr/w", O, K, scale=K ** -0.5), rnd("glue/sr/b", O, scale=0.5), rnd("glue/sr/x", M, K, scale=3.0)
    x[0, :4] = torch.tensor([-87.5, -88.8, 87.5, -20.0])
    xin = padded(x, ldin, 0.0).cuda()
    sx = torch.full((M, ldin), NAN, device="cuda")
    assert nat.lib().lfvdm_silu(xin.data_ptr(), sx.data_ptr(), M * ldin, nat.stream()) == 0
    o0, o1 = torch.full((M, O), NAN, device="cuda"), torch.full((M, O), NAN, device="cuda")
    Wd, bd = W.cuda(), b.cuda()
    launch_rowdot(nat, [(Wd, bd, sx, o0, K, O, M, ldin, O, 0)])
    launch_rowdot(nat, [(Wd, bd, xin, o1, K, O, M, ldin, O, 1)])
    ref, bound = rowdot_ref(W, b, x, 1)
    within("rowdot(silu) in_mode 1", o1, ref, bound)
    assert same_bits(o0, o1), f"{int((bits(o0) != bits(o1)).sum())} of {M * O} outputs differ between the two paths"


# ------------------------------------------------------------------------------------------------------------------------
# 4. lfvdm_conv_in: every instance
# ------------------------------------------------------------------------------------------------------------------------
OBS3 = (0.0, 1.0, 0.25)


def conv_in_case(N, C, H, W, Cout):
    tag = f"glue/ci/{N}/{C}/{H}x{W}/{Cout}"
    obs = torch.tensor(OBS3).repeat((N + 2) // 3)[:N].contiguous()
    return dict(x=rnd(tag + "/x", N, C, H, W), x0=rnd(tag + "/x0", N, C, H, W), obs=obs,
                w=rnd(tag + "/w", Cout, C + 1, 3, 3, scale=0.2), b=rnd(tag + "/b", Cout), dims=(N, C, H, W, Cout))


def conv_in_ref(c):
    """F.conv2d in fp64 of [x (1 - obs) + x0 obs | obs].  Bound (9 (C + 1) + 4) U sum|w v| + U |ref|: a product is rounded,
    added into a chain of 9 (C + 1) terms behind the bias, and its input carries the blend's roundings."""
    N, C, H, W, Cout = c["dims"]
    o = c["obs"].double().view(N, 1, 1, 1)
    comp = torch.cat([c["x"].double() * (1 - o) + c["x0"].double() * o, o.expand(N, 1, H, W)], 1)
    wd = c["w"].double()
    ref = F.conv2d(comp, wd, c["b"].double(), padding=1)
    bound = (9 * (C + 1) + 4) * U * F.conv2d(comp.abs(), wd.abs(), None, padding=1) + U * ref.abs()
    return ref, bound


def conv_in_dev(c):
    N, C, H, W, Cout = c["dims"]
    d = {k: c[k].cuda() for k in ("x", "x0", "obs", "w", "b")}
    d["out"] = torch.full((N * H * W + 1, Cout), NAN, device="cuda")     # one guard row behind the last pixel
    d["out"][-1] = SENT
    return d


def run_conv_in(nat, c):
    N, C, H, W, Cout = c["dims"]
    d = conv_in_dev(c)
    nat.conv_in(d["x"], d["x0"], d["obs"], d["w"], d["b"], d["out"], N, C, H, W, Cout)
    torch.cuda.synchronize()
    assert same_bits(d["out"][-1], torch.full((Cout,), SENT)), "written past the last pixel"
    return d["out"][:-1]


def check_conv_in(nat, tag, N, C, H, W, Cout):
    c = conv_in_case(N, C, H, W, Cout)
    ref, bound = conv_in_ref(c)
    within(f"{tag} C={C} Cout={Cout} N={N} {H}x{W}", from_cl(run_conv_in(nat, c), N, H, W, Cout), ref, bound)


@pytest.mark.parametrize("H,W", [(10, 10), (6, 10)])
@pytest.mark.parametrize("C,Cout", [(4, 64), (4, 128), (3, 64), (3, 128)])
def test_conv_in_mfma_instances(nat, C, Cout, H, W):
    """conv_in_mfma_kernel<4,5>, <8,5>, <4,4>, <8,4> (K = 45 padded to 48, K = 36): N = 3 frames with obs = 0, 1, 0.25.
    10x10: 300 pixels, 44 live lanes in the last workgroup (its last wave has none), frames change inside a wave.  6x10:
    rows and columns differ, so a swapped H / W in the tap decode shows.  Bound: see conv_in_ref."""
    check_conv_in(nat, "conv_in mfma", 3, C, H, W, Cout)


SCALAR_CASES = ([(C, 16 * Q) for C in (4, 3) for Q in range(1, 17) if Q not in (4, 8)] +
                [(C, 16 * Q) for C in (2, 5) for Q in (1, 4, 9, 16)])


@pytest.mark.parametrize("C,Cout", SCALAR_CASES)
def test_conv_in_scalar_instances(nat, C, Cout):
    """conv_in_kernel<Q, 5> (C = 4), <Q, 4> (C = 3) for every Q = Cout / 16 the dispatcher does not give to the matrix-core
    form, and <Q, 0> (run-time channel loop) at C = 2, 5 with Q = 1, 4, 9, 16.  N = 7 frames of 5x3: a wave holds pixels
    of up to five frames, 105 pixels leave 41 live lanes in the second workgroup; obs cycles 0, 1, 0.25.  C = 5, Cout = 256
    is the largest filter block LDS holds: the reciprocal index split of the transpose sees i up to 54 * 256.  Bound: see
    conv_in_ref."""
    check_conv_in(nat, "conv_in scalar", 7, C, 5, 3, Cout)


def _scalar_child():
    """Body of the child process of test_conv_in_scalar_switch (LFVDM_CONV_IN_SCALAR is set before the library loads)."""
    assert os.environ.get("LFVDM_CONV_IN_SCALAR")
    from improved_diffusion import _native
    _native.lib()
    for C, Cout in ((4, 64), (4, 128)):
        for H, W in ((10, 10), (5, 3)):
            check_conv_in(_native, "conv_in scalar (switch)", 3 if H == 10 else 7, C, H, W, Cout)


def test_conv_in_scalar_switch():
    """LFVDM_CONV_IN_SCALAR=1 (read once per process, so one fresh child): (4, 64) and (4, 128) go through
    conv_in_kernel<4, 5> and <8, 5>, the two scalar instances nothing else can reach, under the bound of conv_in_ref."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--scalar-child"], env=dict(os.environ, LFVDM_CONV_IN_SCALAR="1"),
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(p.stdout[-2000:])
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.count("[err/bound] conv_in scalar (switch)") == 4, p.stdout[-2000:]


# ------------------------------------------------------------------------------------------------------------------------
# 5. the clock: lfvdm_sampler_tick_fetch and lfvdm_conv_in_tick
# ------------------------------------------------------------------------------------------------------------------------
TABLE5 = (0.0, 250.25, 500.5, 750.75, 999.0)


def clock_case(B, row_floats, shift, pad=12, T=5):
    """t = (5 b + shift) % 6 (0 and T both occur at B > 1); rows_all[T][B][rows_ld] holds its own flat index + 0.5 (every
    value distinct and exact below 2^24), padding included, so a wrong row, a wrong offset or a copied pad shows."""
    ld = row_floats + pad
    t = (5 * torch.arange(B, dtype=torch.int64) + shift) % (T + 1)
    rows_all = (torch.arange(T * B * ld, dtype=torch.float32) + 0.5).view(T, B, ld)
    rows = torch.full((B, ld), NAN)
    rows[:, row_floats:] = SENT
    model_t = torch.full((B + 1,), NAN)
    model_t[B] = SENT
    return dict(t=t, table=torch.tensor(TABLE5), rows_all=rows_all, rows=rows, model_t=model_t, B=B, ld=ld, rf=row_floats)


def clock_ref(c):
    t_new = (c["t"] - 1).clamp_min(0)
    rows = c["rows"].clone()
    rows[:, :c["rf"]] = c["rows_all"][t_new, torch.arange(c["B"]), :c["rf"]]
    model_t = c["model_t"].clone()
    model_t[:c["B"]] = c["table"][t_new]
    return t_new, model_t, rows


def clock_dev(c):
    return {k: c[k].cuda() for k in ("t", "table", "rows_all", "rows", "model_t")}


def tick_fetch(nat, c, d, **over):
    a = dict(t=d["t"].data_ptr(), table=d["table"].data_ptr(), B=c["B"], ld=c["ld"], rf=c["rf"])
    a.update(over)
    rc = nat.lib().lfvdm_sampler_tick_fetch(a["t"], a["table"], d["model_t"].data_ptr(), a["B"], d["rows_all"].data_ptr(), a["ld"],
                                            d["rows"].data_ptr(), a["rf"], nat.stream())
    torch.cuda.synchronize()
    return rc


def conv_in_tick(nat, cc, cd, c, d, **over):
    N, C, H, W, Cout = cc["dims"]
    a = dict(t=d["t"].data_ptr(), table=d["table"].data_ptr(), B=c["B"], ld=c["ld"], rf=c["rf"])
    a.update(over)
    rc = nat.lib().lfvdm_conv_in_tick(cd["x"].data_ptr(), cd["x0"].data_ptr(), cd["obs"].data_ptr(), cd["w"].data_ptr(),
                                      cd["b"].data_ptr(), cd["out"].data_ptr(), N, C, H, W, Cout, a["t"], a["table"],
                                      d["model_t"].data_ptr(), a["B"], d["rows_all"].data_ptr(), a["ld"], d["rows"].data_ptr(),
                                      a["rf"], nat.stream())
    torch.cuda.synchronize()
    return rc


def check_clock(tag, c, d):
    t_new, model_t, rows = clock_ref(c)
    assert torch.equal(d["t"].cpu(), t_new), f"{tag}: t {d['t'].cpu().tolist()} != {t_new.tolist()}"
    assert same_bits(d["model_t"], model_t), f"{tag}: model_t (or the element behind it)"
    assert same_bits(d["rows"][:, :c["rf"]], rows[:, :c["rf"]]), f"{tag}: fetched rows"
    assert same_bits(d["rows"][:, c["rf"]:], rows[:, c["rf"]:]), f"{tag}: row padding written"


CONV_FOR_TICK = ((3, 4, 6, 10, 64), (3, 4, 6, 10, 32))          # conv_in_mfma_kernel<4,5> and conv_in_kernel<2,5>


@pytest.fixture(scope="module")
def tick_convs(nat):
    """The two convolutions the clock rides on, with lfvdm_conv_in's own output of each."""
    out = []
    for dims in CONV_FOR_TICK:
        cc = conv_in_case(*dims)
        out.append((cc, run_conv_in(nat, cc).clone()))
    return out


@pytest.mark.parametrize("row_floats", [4, 1028, 8196])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_sampler_clock(nat, tick_convs, B, row_floats):
    """sampler_tick_fetch_kernel (1024 threads, e / q4 split) and conv_in_clock (the extra workgroup of both conv_in forms;
    eight float4 per thread with a tail guard) at q4 = 1 (one float4), 257 (one past a 256-thread stride) and 2049 (one
    past the 8 x 256 unroll), B = 1, 3, 64 (the last fills the 64-entry tnew array), rows_ld = row_floats + 12, 5 table rows.
    t = (5 b + s) % 6 for s = 0, 3: a 0 that stays 0 and fetches row 0, and a 5 that fetches the last row.  Exact: t, model_t
    (guard element behind it), the fetched floats, the 12 padding floats of every row.  conv_in_tick's `out` equals
    lfvdm_conv_in's bit for bit and its clock equals sampler_tick_fetch's."""
    for shift in (0, 3):
        c = clock_case(B, row_floats, shift)
        d = clock_dev(c)
        assert tick_fetch(nat, c, d) == 0
        check_clock(f"tick_fetch s={shift}", c, d)
        for cc, conv_out in tick_convs:
            cd, d2 = conv_in_dev(cc), clock_dev(c)
            assert conv_in_tick(nat, cc, cd, c, d2) == 0
            check_clock(f"conv_in_tick Cout={cc['dims'][4]} s={shift}", c, d2)
            for k in ("t", "model_t", "rows"):
                assert same_bits(d2[k], d[k]), k
            assert same_bits(cd["out"][:-1], conv_out), "conv_in_tick's convolution differs from lfvdm_conv_in's"
            assert same_bits(cd["out"][-1], torch.full((cc["dims"][4],), SENT)), "written past the last pixel"


def test_sampler_clock_refusals(nat, tick_convs):
    """Both entries return non-zero and launch nothing at B = 65, row_floats % 4 != 0, rows_ld < row_floats and a NULL
    table: t, model_t, rows and the convolution's output keep their bits.  (Buffers are sized for B = 65.)"""
    c = clock_case(65, 8, 0)
    cc = tick_convs[0][0]
    for over in (dict(B=65), dict(B=3, rf=6), dict(B=3, ld=4), dict(B=3, table=None), dict(B=0), dict(B=3, t=None)):
        for entry in ("fetch", "conv"):
            d, cd = clock_dev(c), conv_in_dev(cc)
            before = {k: bits(d[k]).clone() for k in ("t", "model_t", "rows")}
            out0 = bits(cd["out"]).clone()
            rc = tick_fetch(nat, c, d, **over) if entry == "fetch" else conv_in_tick(nat, cc, cd, c, d, **over)
            assert rc != 0, (entry, over)
            for k in before:
                assert torch.equal(bits(d[k]), before[k]), (entry, over, k)
            assert torch.equal(bits(cd["out"]), out0), (entry, over)


# ------------------------------------------------------------------------------------------------------------------------
# 6. lfvdm_compose_rows, lfvdm_prepare_batch, lfvdm_q_sample
# ------------------------------------------------------------------------------------------------------------------------
def compose_case(Cx, N=7, H=5, W=3):
    tag = f"glue/cr/{Cx}"
    obs = torch.tensor(OBS3).repeat((N + 2) // 3)[:N].contiguous()
    return rnd(tag + "/x", N, Cx, H, W), rnd(tag + "/x0", N, Cx, H, W), obs


def compose_ref(x, x0, obs):
    """Channels-last fp64 blend [N][H][W][Cx] and its bound 2 U (|x| + |x0|): each product is rounded once, then the sum."""
    o = obs.double().view(-1, 1, 1, 1)
    ref = (x.double() * (1 - o) + x0.double() * o).permute(0, 2, 3, 1).contiguous()
    bound = (2 * U * (x.double().abs() + x0.double().abs())).permute(0, 2, 3, 1).contiguous()
    return ref, bound


def compose_rows(nat, x, x0, obs, rows, N, Cx, H, W, ld):
    rc = nat.lib().lfvdm_compose_rows(x.data_ptr(), x0.data_ptr(), obs.data_ptr(), rows.data_ptr(), N, Cx, H, W, ld, nat.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("ld", [8, 32])
@pytest.mark.parametrize("Cx", [2, 3, 4])
def test_compose_rows(nat, Cx, ld):
    """compose_rows_kernel, one thread per (frame, pixel, 4 channels): N = 7 frames of 5x3 (105 rows; ld = 32 needs four
    workgroups, the last one ragged), obs cycles 0, 1, 0.25.  Cx = 4 puts the indicator into the second float4, Cx = 2, 3
    into the first.  Channels below Cx against the fp64 blend (bound: compose_ref); channel Cx is obs exactly; the
    channels above are +0 exactly; the guard row behind the last pixel keeps its sentinel.  ld = Cx and ld = 6 are refused."""
    N, H, W = 7, 5, 3
    x, x0, obs = compose_case(Cx)
    xd, x0d, od = x.cuda(), x0.cuda(), obs.cuda()
    rows = torch.full((N * H * W + 1, ld), NAN, device="cuda")
    rows[-1] = SENT
    assert compose_rows(nat, xd, x0d, od, rows, N, Cx, H, W, ld) == 0
    got = rows[:-1].cpu().view(N, H, W, ld)
    ref, bound = compose_ref(x, x0, obs)
    within(f"compose_rows Cx={Cx} ld={ld}", got[..., :Cx], ref, bound)
    assert same_bits(got[..., Cx], obs.view(N, 1, 1).expand(N, H, W)), "indicator channel"
    assert same_bits(got[..., Cx + 1:], torch.zeros(N, H, W, ld - Cx - 1)), "channels above the indicator"
    assert same_bits(rows[-1], torch.full((ld,), SENT)), "written past the last row"
    close(rows[:-1, Cx:Cx + 1].reshape(N, H, W, 1), cl(obs.view(N, 1, 1, 1).expand(N, 1, H, W)), 0.0, 0.0)   # (equality)
    fresh = torch.full((N * H * W + 1, 8), NAN, device="cuda")
    for bad in (Cx, 6):
        assert compose_rows(nat, xd, x0d, od, fresh, N, Cx, H, W, bad) != 0, bad
    assert same_bits(fresh, torch.full((N * H * W + 1, 8), NAN)), "a refused call wrote"


def prepare_case(frame_elems, B=3, F=5, Tp=9):
    """A hand-written table (B, F, 4) = {pool row, frame index, observed, latent}: rows -1 and Tp + 3 (clamped), the two
    ends, repeats; frame indices with a negative and a large one; mask words 0, 1, 7, -2."""
    pool = (torch.arange(B * Tp * frame_elems, dtype=torch.float32) + 0.5).view(B, Tp, frame_elems)
    rows = [-1, Tp + 3, 0, Tp - 1, 4, 4, 7, 1, Tp, -5, 3, 8, 2, 6, 5]
    fidx = [0, 1, -3, 100000, 19, 7, 7, 2, 999, 5, 11, 12, 13, 14, 2 ** 31 - 1]
    obs = [0, 1, 7, -2, 0, 1, 1, 0, 0, 3, 0, 0, 1, 1, 0]
    lat = [1, 0, 0, 7, -2, 0, 1, 1, 0, 0, 5, 1, 0, 0, 1]
    table = torch.tensor(list(zip(rows, fidx, obs, lat)), dtype=torch.int32).view(B, F, 4)
    return pool, table


def prepare_ref(pool, table):
    B, Tp = pool.shape[:2]
    row = table[..., 0].long().clamp(0, Tp - 1)
    batch = pool[torch.arange(B)[:, None], row]
    return batch, table[..., 1].long(), (table[..., 2] != 0).float(), (table[..., 3] != 0).float()


def prepare_batch(nat, pool_ptr, table, out, B, F, Tp, fe):
    rc = nat.lib().lfvdm_prepare_batch(pool_ptr, table.data_ptr(), out["batch"].data_ptr(), out["fi"].data_ptr(),
                                       out["obs"].data_ptr(), out["lat"].data_ptr(), B, F, Tp, fe, nat.stream())
    torch.cuda.synchronize()
    return rc


def prepare_out(B, F, fe):
    batch = torch.full((B * F * fe + 4,), NAN, device="cuda")
    batch[-4:] = SENT
    return dict(batch=batch, fi=torch.full((B, F), -999, dtype=torch.int64, device="cuda"),
                obs=torch.full((B, F), NAN, device="cuda"), lat=torch.full((B, F), NAN, device="cuda"))


@pytest.mark.parametrize("frame_elems", [4, 300, 1028])
def test_prepare_batch_direct(nat, frame_elems):
    """prepare_batch_kernel called directly, one workgroup per (frame slot, video): frame_elems = 4 (one float4, 255 idle
    threads), 300 (75 float4: one ragged trip), 1028 (257 float4: one thread takes a second trip).  Table rows -1 and
    Tp + 3 clamp to the first and last pool row of the SAME video.  Exact: the frames, the int64 frame indices (sign
    extended), the masks (any non-zero word is 1.0), the 4 floats behind the batch.  frame_elems = 6 and a pool pointer
    moved by one float are refused and write nothing."""
    B, F, Tp = 3, 5, 9
    pool, table = prepare_case(frame_elems)
    pd, td = pool.cuda(), table.cuda()
    out = prepare_out(B, F, frame_elems)
    assert prepare_batch(nat, pd.data_ptr(), td, out, B, F, Tp, frame_elems) == 0
    batch, fi, obs, lat = prepare_ref(pool, table)
    assert same_bits(out["batch"][:-4].view(B, F, frame_elems), batch), "gathered frames"
    assert same_bits(out["batch"][-4:], torch.full((4,), SENT)), "written past the batch"
    assert torch.equal(out["fi"].cpu(), fi)
    assert same_bits(out["obs"], obs) and same_bits(out["lat"], lat)
    fresh = prepare_out(B, F, frame_elems)
    before = {k: bits(v).clone() for k, v in fresh.items()}
    big = torch.zeros(B * Tp * frame_elems + 8, device="cuda")
    assert prepare_batch(nat, pd.data_ptr(), td, fresh, B, F, Tp, 6) != 0
    assert prepare_batch(nat, big.data_ptr() + 4, td, fresh, B, F, Tp, frame_elems) != 0
    for k, v in fresh.items():
        assert torch.equal(bits(v), before[k]), f"a refused call wrote {k}"


Q_INNER = 4 * (1024 * 256 + 100) + 3


def q_sample_case():
    g = torch.Generator().manual_seed(20240607)
    x0 = torch.randn(2, Q_INNER, generator=g)
    noise = torch.randn(2, Q_INNER, generator=g)
    acp = torch.cumprod(1.0 - torch.linspace(1e-4, 0.02, 1000, dtype=torch.float64), 0)
    return x0, noise, torch.tensor([0, 999]), acp.sqrt().float(), (1.0 - acp).sqrt().float()


def q_sample_ref(x0, noise, t, sa, sb):
    """fp64 a[t] x0 + b[t] noise; bound 3 U (|a x0| + |b n|): two products and one add."""
    a, b = sa[t].double().view(-1, 1), sb[t].double().view(-1, 1)
    p, q = a * x0.double(), b * noise.double()
    return p + q, 3 * U * (p.abs() + q.abs())


def test_q_sample_past_grid_cap(nat):
    """q_sample_kernel at inner = 4 (1024 * 256 + 100) + 3: the grid is capped at 1024 workgroups, 100 threads take a second
    grid-stride trip and the last of them the scalar tail of 3 floats (the kernel has one: no multiple of 4 is required;
    the second batch row then starts off a 16-byte boundary).  t = [0, 999]: both ends of the tables.  The 8 floats behind
    the output keep their sentinel.  Bound: see q_sample_ref."""
    x0, noise, t, sa, sb = q_sample_case()
    out = torch.full((2 * Q_INNER + 8,), NAN, device="cuda")
    out[-8:] = SENT
    d = [v.cuda() for v in (x0, noise, t, sa, sb)]
    rc = nat.lib().lfvdm_q_sample(*(v.data_ptr() for v in d), out.data_ptr(), 2, Q_INNER, nat.stream())
    torch.cuda.synchronize()
    assert rc == 0
    ref, bound = q_sample_ref(x0, noise, t, sa, sb)
    within("q_sample", out[:-8].view(2, Q_INNER), ref, bound)
    assert same_bits(out[-8:], torch.full((8,), SENT)), "written past the output"


if __name__ == "__main__":
    assert sys.argv[1:] == ["--scalar-child"], sys.argv
    _scalar_child()
