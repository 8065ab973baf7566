"""Footprint harness: every operand of a launch sits inside one larger allocation between two guard bands, the launch runs
once per fill of the bands (a finite sentinel, NaN, 1e30), and three things are asserted -

(a) writes stay inside: output bands and padding columns keep the fill's words, input buffers are word for word unchanged;
(b) the result does not depend on what lies outside: the outputs of the three runs are bit-identical, none holds a NaN or
    a magnitude >= 1e29 (NaN catches `v * 0` masking and unmasked loads, 1e30 what a NaN-swallowing max hides);
(c) the result is still right: the sentinel run meets the op's existing reference at the existing test's tolerance.

Launches whose summation order is not fixed (RELAXED, float atomics) cannot be compared across runs: for those (b) is "no
NaN, nothing >= 1e29" and every fill's run has to meet (c).  The list is a constant and `footprint` takes the entry's NAME,
so a broken harness cannot relax anything else.

This file holds the harness, the case lists of test_footprint_gpu and the proof that the harness can fail: host
restatements of a 3x3 conv over channels-last rows and of a row softmax play the kernel, and each of six plausible
tail-predicate bugs is rejected by the rule named in MUTATIONS.  The restatements index the flat allocation the way a
kernel indexes a pointer, so an overrun really lands in a band.  Runs without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import numpy as np

from oracle import recipe
from test_train_glue_cpu import NAN, SENT, bits, same_bits


def rnd(tag, *shape, scale=1.0):
    """The suite's tagged pseudo-random float32 tensor (test_ops_gpu.rnd, restated so that this file imports no GPU module)."""
    return torch.from_numpy((scale * recipe.gaussianish(tag, int(np.prod(shape)))).reshape(shape).astype(np.float32))

FILLS = (SENT, NAN, 1e30)
BIG = 1e29
ROW_TILE = 64                   # the tallest row tile of any kernel under test (conv: 32 / 64 rows)

# launches under the relaxed rule (b): atomics, order of summation not fixed.  The deterministic sibling of each
# ("lfvdm_gn_bwd/det", "lfvdm_rowdot_bwd_det", "lfvdm_rpe_nets_bwd_det", "lfvdm_gn_temporal_bwd_det",
# "lfvdm_conv_wgrad/slab") gets the full bitwise rule.
RELAXED = ("lfvdm_gn_bwd/atomics", "lfvdm_rowdot_bwd", "lfvdm_rpe_nets_bwd", "lfvdm_gn_temporal_bwd", "lfvdm_conv_wgrad/atomics")


def band_floats(ld):
    """Two full row tiles of the operand's rows, not fewer than 1024 floats; a multiple of 64 floats (256 bytes)."""
    return max(1024, 2 * ROW_TILE * int(ld))


def embed(values_or_count, fill, band, width=None, ld=None, device="cpu"):
    """-> (buffer, view): the operand between two bands of `fill` inside one allocation.  `values_or_count`: a tensor (its
    last axis is the row; 1-D = one row) or a number of floats (then the operand itself starts as `fill` too).  ld > width
    leaves padding columns, which hold the fill; the view is [rows][width] with row stride ld."""
    assert band % 64 == 0 and band >= 1024
    if isinstance(values_or_count, int):
        width = width or values_or_count
        rows, values = values_or_count // width, None
        assert rows * width == values_or_count
    else:
        values = values_or_count.reshape(-1, values_or_count.shape[-1]) if values_or_count.dim() > 1 else values_or_count.reshape(1, -1)
        rows, width = values.shape
    ld = ld or width
    assert ld >= width and band >= band_floats(ld)
    buf = torch.full((band + rows * ld + band,), fill, dtype=torch.float32, device=device)
    view = buf[band:band + rows * ld].view(rows, ld)[:, :width]
    if values is not None:
        view.copy_(values)
    return buf, view


class Op:
    """Description of one operand.  role "in": `values` (rows, width).  role "out": a shape, optionally `init` (accumulated
    outputs), `scratch` (a workspace: contents free, words past its documented size = the band), `untouched` (handed in but
    never to be written), `zero` (starts zero and must be zero afterwards: split-K tickets), `ints` (int32 words)."""

    def __init__(self, role, values=None, rows=None, width=None, ld=None, init=None, scratch=False, untouched=False, zero=False,
                 ints=False):
        if values is not None:
            values = values.float()
            values = values.reshape(-1, values.shape[-1]) if values.dim() > 1 else values.reshape(1, -1)
            rows, width = values.shape
        if init is not None:
            init = init.float().reshape(rows, width)
        self.role, self.values, self.rows, self.width, self.ld = role, values, int(rows), int(width), int(ld or width)
        self.init, self.scratch, self.untouched, self.zero, self.ints = init, scratch, untouched, zero, ints
        assert self.ld >= self.width


def inp(values, ld=None):
    return Op("in", values=values, ld=ld)


def outp(rows, width, ld=None, **kw):
    return Op("out", rows=rows, width=width, ld=ld, **kw)


class Embedded:
    def __init__(self, op, fill, device):
        self.op, self.fill, self.band = op, fill, band_floats(op.ld)
        src = op.values if op.role == "in" else (op.init if op.init is not None else op.rows * op.width)
        self.buf, self.view = embed(src, fill, self.band, width=op.width, ld=op.ld, device=device)
        if op.zero:
            self.view.zero_()
        self.off = self.band                              # index of the operand's first float in buf
        self.ld = op.ld

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    def outside(self):
        """Mask over buf: bands and padding columns."""
        m = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        m[self.off:self.off + self.op.rows * self.op.ld].view(self.op.rows, self.op.ld)[:, :self.op.width] = False
        return m

    def inside(self):
        v = self.view.detach().cpu().contiguous()
        return v.view(torch.int32) if self.op.ints else v


class FootprintError(AssertionError):
    def __init__(self, found):
        self.found = found
        self.rules = {r for r, _ in found}
        super().__init__("; ".join(f"({r}) {m}" for r, m in found))


def footprint(entry, launch, inputs, outputs, check, fills=FILLS, device="cpu"):
    """Run `launch(t)` once per fill; t maps names to Embedded operands (t[k].ptr / .ld on a device, .buf / .off on the
    host).  `check(out, fill)` asserts rule (c) on {name: tensor [rows][width]}.  Raises FootprintError naming every
    violated rule; returns the outputs of the first run."""
    relaxed = entry in RELAXED
    found, runs = [], []
    for run, fill in enumerate(fills):
        fbits = int(bits(torch.tensor([fill], dtype=torch.float32))[0])
        t = {k: Embedded(op, fill, device) for k, op in {**inputs, **outputs}.items()}
        before = {k: t[k].buf.view(torch.int32).clone() for k in inputs}      # words, compared where the buffer lives
        launch(t)
        if device != "cpu":
            torch.cuda.synchronize()
        tag = "nan" if fill != fill else f"{fill:g}"
        for k in outputs:                                               # (a)
            words, e = t[k].buf.view(torch.int32), t[k]
            bad = (words != fbits) & e.outside()
            if bool(bad.any()):
                i = int(bad.nonzero()[0])
                found.append(("a", f"{entry}: fill {tag}: {k} written outside at float {i - e.off} of the operand ({int(bad.sum())} words)"))
            if e.op.untouched and not bool((words == fbits).all()):
                found.append(("a", f"{entry}: fill {tag}: {k} must keep the fill entirely"))
            if e.op.zero and bool((e.inside() != 0).any()):
                found.append(("a", f"{entry}: fill {tag}: {k} must return to zero"))
        for k in inputs:
            if not torch.equal(t[k].buf.view(torch.int32), before[k]):
                found.append(("a", f"{entry}: fill {tag}: input {k} was written"))
        got = {k: t[k].inside() for k, op in outputs.items() if not (op.scratch or op.untouched or op.zero)}
        for k, v in got.items():                                        # (b), the part that holds under either rule
            if not outputs[k].ints and (bool(torch.isnan(v).any()) or bool((v.abs() >= BIG).any())):
                found.append(("b", f"{entry}: fill {tag}: {k} holds NaN or a magnitude >= 1e29"))
        runs.append(got)
        if run == 0 or relaxed:                                  # (c)
            try:
                check(got, fill)
            except AssertionError as e:
                found.append(("c", f"{entry}: fill {tag}: {e}"))
    if not relaxed:                                                     # (b), bitwise
        for fill, got in zip(fills[1:], runs[1:]):
            for k, v in got.items():
                if not same_bits(v, runs[0][k]):
                    n = int((bits(v) != bits(runs[0][k])).sum())
                    found.append(("b", f"{entry}: {k} depends on the bands: {n} words differ between fills {fills[0]:g} and {fill:g}"))
    if found:
        raise FootprintError(found)
    return runs[0]


# ------------------------------------------------------------------------------------------------------------------------
# host "kernels": pointer-style indexing into the flat allocation, a tile of 32 rows, one plausible bug each
# ------------------------------------------------------------------------------------------------------------------------
def host_conv3x3(t, N, H, W, Cin, Cout, mutation=None):
    """out[m][co] = sum_{tap, ci} x[n, y + dy, x + dx, ci] * w[co][tap][ci], zero outside the image; rows m = (n, y, x)."""
    x, w, o = t["x"], t["w"], t["out"]
    M = N * H * W
    Mt = (M + 31) // 32 * 32
    m = torch.arange(Mt)
    n, y, xx = m // (H * W), (m // W) % H, m % W
    wv = w.view.reshape(Cout, 9, Cin).double()
    acc = torch.zeros(Mt, Cout, dtype=torch.float64)
    for tap in range(9):
        iy, ix = y + tap // 3 - 1, xx + tap % 3 - 1
        col_ok = (ix >= 0) & (ix < W)
        ok = (m < M) & (iy >= 0) & (iy < H) & col_ok
        row = (n * H + iy) * W + ix
        if mutation == "halo_before":                     # the top halo of the FIRST sample is taken for rows of a sample before
            ok = ok | ((m < M) & (n == 0) & (iy == -1) & col_ok)
        if mutation == "tail_rows":                       # the bottom edge is tested against the tile-rounded row count
            ok = (m < M) & (iy >= 0) & col_ok & (row < Mt) & ((iy < H) | (n == N - 1))
        reach = ok if mutation != "mul_zero" else (m < M)
        addr = x.off + torch.where(reach, row, torch.zeros_like(row))[:, None] * x.ld + torch.arange(Cin)[None, :]
        v = x.buf[addr].double()
        v = v * ok[:, None].double() if mutation == "mul_zero" else torch.where(ok[:, None], v, torch.zeros_like(v))
        acc += v @ wv[:, tap].t()
    cols = Cout + 1 if mutation == "write_col_cout" else Cout
    res = torch.cat([acc, torch.zeros(Mt, 1, dtype=torch.float64)], 1)[:M, :cols].float()
    o.buf[(o.off + torch.arange(M)[:, None] * o.ld + torch.arange(cols)[None, :])] = res
    if mutation == "band_write":
        o.buf[o.off + o.op.rows * o.ld] = 0.0


def host_softmax(t, R, Wd, mutation=None):
    """Row softmax with a NaN-swallowing max (fmaxf / v_max) over the row's Wd columns."""
    x, o = t["x"], t["out"]
    span = Wd + 1 if mutation == "max_one_more" else Wd
    addr = x.off + torch.arange(R)[:, None] * x.ld + torch.arange(span)[None, :]
    v = x.buf[addr]
    mx = v[:, 0]
    for c in range(1, span):
        mx = torch.fmax(mx, v[:, c])
    e = torch.exp(v[:, :Wd] - mx[:, None])
    res = e / e.sum(1, keepdim=True)
    o.buf[o.off + torch.arange(R)[:, None] * o.ld + torch.arange(Wd)[None, :]] = res
    if mutation == "band_write":
        o.buf[o.off + o.op.rows * o.ld] = 0.0


# mutation -> the rules that reject it (exactly)
MUTATIONS = {
    ("conv", "halo_before"): {"b", "c"},          # reads one row before the first sample's top halo
    ("conv", "tail_rows"): {"b", "c"},            # reads one row past the last tile where M % 32 != 0
    ("conv", "write_col_cout"): {"a"},            # writes column Cout of an ldo > Cout row
    ("conv", "mul_zero"): {"b"},                  # multiplies an out-of-range load by 0 instead of selecting 0
    ("softmax", "max_one_more"): {"b"},           # row max over one column too many: only the 1e30 fill shows it
    ("conv", "band_write"): {"a"},                # writes the first float of the trailing band
    ("softmax", "band_write"): {"a"},
}
HOST_CONV = dict(N=3, H=5, W=5, Cin=8, Cout=6, ldx=8, ldo=8)       # M = 75: the last 32-row tile holds 11 rows
HOST_SOFTMAX = dict(R=7, Wd=13, ldx=16, ldo=16)


def close64(got, want, atol, rtol=1e-4):
    err = float((got.double() - want.double()).abs().max())
    assert torch.allclose(got.double(), want.double(), atol=atol, rtol=rtol), f"max|d| = {err:.3e}"


def _host_run(kind, mutation, fills=FILLS):
    if kind == "conv":
        c = HOST_CONV
        x, w = rnd("fp/host/x", c["N"], c["Cin"], c["H"], c["W"]), rnd("fp/host/w", c["Cout"], c["Cin"], 3, 3, scale=0.2)
        want = F.conv2d(x.double(), w.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, c["Cout"])
        ins = dict(x=inp(x.permute(0, 2, 3, 1).reshape(-1, c["Cin"]), ld=c["ldx"]), w=inp(w.permute(0, 2, 3, 1).reshape(c["Cout"], -1)))
        outs = dict(out=outp(c["N"] * c["H"] * c["W"], c["Cout"], ld=c["ldo"]))
        launch = lambda t: host_conv3x3(t, c["N"], c["H"], c["W"], c["Cin"], c["Cout"], mutation)
    else:
        c = HOST_SOFTMAX
        x = 3.0 * rnd("fp/host/s", c["R"], c["Wd"])
        want = torch.softmax(x.double(), -1)
        ins, outs = dict(x=inp(x, ld=c["ldx"])), dict(out=outp(c["R"], c["Wd"], ld=c["ldo"]))
        launch = lambda t: host_softmax(t, c["R"], c["Wd"], mutation)
    return footprint(f"host_{kind}", launch, ins, outs, lambda o, fill: close64(o["out"], want, 2e-5), fills=fills)


@pytest.mark.parametrize("kind", ["conv", "softmax"])
def test_the_unmutated_restatements_pass(kind):
    out = _host_run(kind, None)["out"]
    assert out.shape[1] == (HOST_CONV["Cout"] if kind == "conv" else HOST_SOFTMAX["Wd"]) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("kind,mutation", list(MUTATIONS), ids=lambda v: str(v))
def test_every_mutation_is_rejected_by_its_rule(kind, mutation):
    with pytest.raises(FootprintError) as e:
        _host_run(kind, mutation)
    assert e.value.rules == MUTATIONS[(kind, mutation)], str(e.value)


def test_the_fills_are_each_needed():
    """`v * 0` passes under the two finite fills, the over-wide max under the sentinel and under NaN."""
    _host_run("conv", "mul_zero", fills=(SENT, 1e30))
    _host_run("softmax", "max_one_more", fills=(SENT, NAN))
    assert HOST_CONV["N"] * HOST_CONV["H"] * HOST_CONV["W"] % 32 != 0 and HOST_CONV["ldo"] > HOST_CONV["Cout"]


def test_embed_keeps_alignment_and_two_row_tiles():
    for ld, width in ((8, 6), (96, 96), (128, 96), (384, 384), (4, 4)):
        band = band_floats(ld)
        assert band % 64 == 0 and band >= 1024 and band >= 2 * 64 * ld
        buf, view = embed(torch.zeros(5, width), NAN, band, ld=ld)
        assert (view.data_ptr() - buf.data_ptr()) % 256 == 0 and view.shape == (5, width) and view.stride(0) == ld
        assert int(torch.isnan(buf).sum()) == 2 * band + 5 * (ld - width)
    with pytest.raises(AssertionError):
        embed(16, NAN, 1000)


def test_a_relaxed_entry_still_has_to_be_right_under_every_fill():
    """Rule (c) per fill: a launch on the relaxed list whose result follows the band is rejected by (c), not waved through."""
    x = rnd("fp/host/r", 4, 8)

    def launch(t):
        e = t["out"]
        e.buf[e.off:e.off + 32] = (t["x"].view + (t["x"].buf[0] > 1e29).float()).reshape(-1)

    with pytest.raises(FootprintError) as e:
        footprint(RELAXED[1], launch, dict(x=inp(x)), dict(out=outp(4, 8)), lambda o, fill: close64(o["out"], x, 1e-6))
    assert e.value.rules == {"c"}
    with pytest.raises(FootprintError) as e:
        footprint("lfvdm_rowdot_bwd_det", launch, dict(x=inp(x)), dict(out=outp(4, 8)), lambda o, fill: close64(o["out"], x, 1e-6))
    assert e.value.rules == {"b"}


def test_the_relaxed_list_names_only_the_unordered_sums():
    """Exactly the five atomics launches; each of them AND its deterministic sibling is a GPU case, so the sibling runs under
    the bitwise rule; the GPU file hands `footprint` the case's own entry name (test_footprint_gpu.run)."""
    assert set(RELAXED) == {"lfvdm_gn_bwd/atomics", "lfvdm_rowdot_bwd", "lfvdm_rpe_nets_bwd", "lfvdm_gn_temporal_bwd",
                            "lfvdm_conv_wgrad/atomics"} and len(RELAXED) == 5
    assert set(SIBLING) == set(RELAXED) and not set(SIBLING.values()) & set(RELAXED)
    every = {c["entry"] for cases in GPU_CASES.values() for c in cases}
    for name, det in SIBLING.items():
        assert name in every, f"{name}: no GPU case"
        assert det in every, f"{det}: the deterministic sibling has no GPU case"


# ------------------------------------------------------------------------------------------------------------------------
# the GPU case lists (test_footprint_gpu runs them); a case qualifies only if some dimension overhangs a tile
# ------------------------------------------------------------------------------------------------------------------------
def _conv(name, N, H, Cin, Cout, k=3, stride=1, up=0, C1=0, **kw):
    Hs, Ws = (H, H) if isinstance(H, int) else H
    if up:
        Ho, Wo = 2 * Hs, 2 * Ws
    elif k == 1:
        Ho, Wo = Hs, Ws
    else:
        Ho, Wo = (Hs - 1) // stride + 1, (Ws - 1) // stride + 1
    return dict(entry="lfvdm_conv_igemm", name=name, N=N, Hs=Hs, Ws=Ws, Ho=Ho, Wo=Wo, C0=Cin - C1, C1=C1, Cout=Cout, k=k,
                stride=stride, up=up, **kw)


CONV_CASES = [
    _conv("3x3-ragged-M", 3, 5, 64, 96),
    _conv("head-Cout4", 3, 5, 64, 4),
    _conv("Cout48", 3, 5, 64, 48),
    _conv("stride2-odd-map", 3, 7, 64, 64, stride=2),
    _conv("up1", 1, 5, 64, 64, up=1),
    _conv("up2", 1, 5, 64, 64, up=2),
    _conv("up3", 1, 5, 64, 64, up=3),
    _conv("concat-64+32", 3, 5, 96, 64, C1=32),
    _conv("skip-segment", 3, 5, 64, 64, s2=(64, 32)),
    _conv("residual-ldr-resAB", 3, 5, 64, 96, res="ab", ldr=128),
    _conv("rows-ldo", 3, 5, 64, 96, ldo=128),
    _conv("nchw", 3, 5, 64, 4, nchw=True),
    _conv("gn-out-ld-film", 5, 2, 64, 64, gn=dict(film=True, skip_raw=0, gn_ld=96, film_pad=32)),
    _conv("gn-out-skip-raw", 5, 2, 64, 64, gn=dict(film=True, skip_raw=1, gn_ld=96, film_pad=32)),
    _conv("gn-out-general", 5, 2, 64, 64, gn=dict(film=False, skip_raw=0, gn_ld=96, film_pad=0, general=1)),
    _conv("linear-75x96x160", 3, (25, 1), 96, 160, k=1),
    _conv("split-k", 5, 2, 128, 128, splitk=True),
]


def conv_overhang(c):
    """The dimensions of a conv case that overhang a tile: rows (32), filters (32), K chunk (64 channels), padded strides."""
    M = c["N"] * c["Ho"] * c["Wo"]
    why = []
    if M % 32:
        why.append("M")
    if c["Cout"] % 32:
        why.append("Cout")
    if (c["C0"] + c["C1"]) % 64 or c["C0"] % 64:
        why.append("K")
    if c.get("ldo", c["Cout"]) > c["Cout"] or c.get("ldr", c["Cout"]) > c["Cout"] or c.get("gn", {}).get("gn_ld", 0) > c["Cout"]:
        why.append("ld")
    return why


# GroupNorm forward: (entry, N or B, P, C0, C1, extras).  A (sample, 8 groups) slice is walked in passes of 64 positions; the
# temporal kernels own 4 (b, pixel) columns per workgroup.
GN_CASES = ([dict(entry="lfvdm_gn_apply", N=2, P=P, C0=64, C1=32, film_pad=32, act=1) for P in (25, 1061)]
            + [dict(entry=e, N=2, P=25, C0=64, C1=32, film_pad=32) for e in ("lfvdm_gn_coef", "lfvdm_gn_coef_stats")]
            + [dict(entry="lfvdm_gn_apply_ws", N=2, P=1061, C0=64, C1=0, film_pad=32, act=1)]
            + [dict(entry="lfvdm_gn_apply_part", N=3, P=25, C0=32, C1=0, cg=4, ldo=96, act=1)]
            + [dict(entry="lfvdm_gn_temporal", N=2, T=T, P=3, C0=64, C1=0) for T in (1, 7, 33)])


def gn_overhang(c):
    why = [] if c["P"] % 64 == 0 else ["P"]
    if c.get("film_pad") or c.get("ldo", 0) > c["C0"]:
        why.append("ld")
    if c["entry"] == "lfvdm_gn_temporal" and (c["N"] * c["P"]) % 4:
        why.append("columns")
    return why


# attention: spatial (N, P, C, heads): query / key tiles of 32 / 64 tokens, head dim in fragments of 16; temporal (B, T, P, C, heads, mask, attn):
# T against the 32-frame window and the 8-frame groups of the long path, P against the pixel strip
ATTN_SPATIAL_CASES = ([dict(entry="lfvdm_attn_spatial", N=1, P=P, C=C, heads=4) for P, C in ((4, 64), (70, 64), (100, 64), (256, 96))]
                      + [dict(entry="lfvdm_attn_spatial_fused", N=2, P=P, C=64, heads=4) for P in (9, 36)])
ATTN_TEMPORAL_CASES = ([dict(entry="lfvdm_attn_temporal", B=2, T=T, P=P, C=64, heads=4, mask=mk, attn=at)
                        for T in (1, 3, 20, 27, 32, 33, 64) for P in (1, 3, 37) for mk in ("mixed", "ones") for at in (1, 0)]
                       + [dict(entry="lfvdm_attn_temporal", B=1, T=20, P=33, C=64, heads=4, mask="mixed", attn=1),       # second generation
                          dict(entry="lfvdm_attn_temporal", B=1, T=13, P=21, C=128, heads=2, mask="mixed", attn=1)]
                       + [dict(entry=e, B=2, T=T, P=P, C=64, heads=4, mask="mixed", attn=1)
                          for e in ("lfvdm_attn_temporal_sel", "lfvdm_attn_temporal_ring") for T in (3, 27, 33, 64) for P in (1, 37)])


def attn_overhang(c):
    why = []
    if c["P"] % 64 and c["entry"].startswith("lfvdm_attn_spatial"):
        why.append("P")
    if (c["C"] // c["heads"]) % 16:
        why.append("head dim")              # 24 floats per head: the last 16-float fragment of a head is half full
    if "T" in c:
        if c["T"] % 32:
            why.append("T")
        if c["P"] % 4:
            why.append("P")
        if c["T"] == 64 and (c["B"] * c["P"]) % 4:
            why.append("windows")           # T = 64, P = 1: the windows do not fill a workgroup's strip
    return why


# glue with tiles
GLUE_CASES = ([dict(entry="lfvdm_conv_in", B=1, T=3, C=4, H=H, Cout=Co) for H, Co in ((5, 48), (2, 32))]
              + [dict(entry="lfvdm_rowdot", M=3, K=256, O=96, ldin=320, ldout=128)]
              + [dict(entry="lfvdm_rpe_nets", B=2, T=5, widths=(64, 32, 128), tproj_pad=32, maxc=mc) for mc in (0, 128)])


def glue_overhang(c):
    if c["entry"] == "lfvdm_conv_in":
        return ["pixels"] if (c["B"] * c["T"] * c["H"] * c["H"]) % 64 else []
    if c["entry"] == "lfvdm_rowdot":
        return ["M"] * (c["M"] % 8 != 0) + ["ld"] * (c["ldin"] > c["K"] or c["ldout"] > c["O"])
    return ["rows"] * ((c["B"] * c["T"] * c["T"]) % 32 != 0) + ["ld"] * (c["tproj_pad"] > 0)


# backward launches: the temporal GroupNorm owns 4 (b, pixel) columns per workgroup, the row-dot backward 8 output rows per
# wave, the attention backwards the tiles of their forwards
BWD_CASES = ([dict(entry=e, B=1, T=7, P=3, C=64, accumulate=a) for e in ("lfvdm_gn_temporal_bwd", "lfvdm_gn_temporal_bwd_det") for a in (0, 1)]
             + [dict(entry="lfvdm_rowdot_bwd", M=3, K=256, O=(96, 44), lddout=48, lddin=320)]
             + [dict(entry="lfvdm_attn_spatial_bwd", N=1, P=70, C=64, heads=4)]
             + [dict(entry="lfvdm_attn_temporal_bwd", B=2, T=7, P=3, C=64, heads=4)])


def bwd_overhang(c):
    e = c["entry"]
    if e.startswith("lfvdm_gn_temporal_bwd"):
        return ["columns"] * ((c["B"] * c["P"]) % 4 != 0)
    if e == "lfvdm_rowdot_bwd":
        return ["O"] * any(o % 8 for o in c["O"]) + ["M"] * (c["M"] % 8 != 0) + ["ld"] * (c["lddin"] > c["K"])
    return attn_overhang(c)


# training launches.  Weight gradient: dW tiles of 32 filters x 32 channels per wave, M in 32-row chunks.  GroupNorm backward:
# _pl(C) positions per pass.  RPE backward: 32-row tiles of B*T*T rows.
WG = dict(N=3, H=5, C0=64, C1=0, Cout=96, k=3)                  # M = 75, Cout = 96: the last row chunk and filter tile are ragged
WGRAD_CASES = ([dict(entry=f"lfvdm_conv_wgrad/{m}", name=v, variant=v, **WG) for m in ("slab", "atomics") for v in ("dma3", "dma2", "regs")]
               + [dict(entry=f"lfvdm_conv_wgrad/{m}", name="codes", variant=None, codes=True, **WG) for m in ("slab", "atomics")]
               + [dict(entry="lfvdm_conv_wgrad/slab", name="oihw", variant=None, oihw=True, codes=True, **WG),
                  dict(entry="lfvdm_conv_wgrad/slab", name="coef-act", variant=None, coef=True, **WG),
                  dict(entry="lfvdm_conv_wgrad_grouped", name="grouped", M=75, widths=(64, 32))])
GN_BWD_SPLITS = [(32, 0), (64, 0), (96, 0), (128, 0), (64, 32), (128, 64), (100, 28), (192, 0), (256, 0), (256, 128), (256, 256),
                 (384, 0), (512, 256), (512, 512), (1024, 0)]   # test_norm_backward_gpu.SPLITS


def gn_pl(C):
    return 256 // (2 * C // 32)


GN_BWD_CASES = ([dict(entry=f"lfvdm_gn_bwd/{m}", C0=C0, C1=C1, N=4, T=2, P=gn_pl(C0 + C1) + 1, act=1, pad=32)
                 for m in ("atomics", "det") for C0, C1 in GN_BWD_SPLITS]
                + [dict(entry=f"lfvdm_gn_bwd/{m}", C0=64, C1=0, N=2, T=2, P=1061, act=1, pad=32) for m in ("atomics", "det")]
                + [dict(entry="lfvdm_gn_param_grads", N=6, T=3, C=96, pad=32)])
TRAIN_GLUE_CASES = [dict(entry="lfvdm_rowdot_bwd_det", M=3, K=256, O=(96, 44), lddout=48, lddin=320),
                    dict(entry="lfvdm_rpe_nets_bwd", B=3, T=6, widths=(64, 160, 32), pad=32),
                    dict(entry="lfvdm_rpe_nets_bwd_det", B=3, T=6, widths=(64, 160, 32), pad=32),
                    dict(entry="lfvdm_rpe_front", B=2, T=5, C=64, pad=32),
                    # B = 1 and T*T = 25 <= 32 rows: one workgroup per 64 channels, so every address of dtproj / dWd / dbd takes exactly
                    # one atomicAdd - an order-fixed sum, under the full bitwise rule
                    dict(entry="lfvdm_rpe_front_bwd", B=1, T=5, C=64, pad=32)]
FUSED_CASES = [dict(entry="lfvdm_gn_temporal_qkv", B=1, T=7, P=2, C=64),
               dict(entry="lfvdm_proj_gn", N=3, P=64, C=64),
               dict(entry="lfvdm_conv_igemm+lfvdm_gn_apply_part", N=5, H=2, Cin=64, C0=64, C1=64),
               dict(entry="lfvdm_conv_out_update_x0", B=1, T=3, H=8, W=12, C=128, Cout=3),
               dict(entry="lfvdm_conv_out_update_ms_x0", B=1, T=3, H=8, W=12, C=128, Cout=3),
               dict(entry="lfvdm_sampler_tick_fetch", B=3, row_floats=20, rows_ld=32),
               dict(entry="lfvdm_dyn_threshold", B=3, T=5, F=37, mask="subset", pct=0.995)]


def train_overhang(c):
    e = c["entry"]
    if e.startswith("lfvdm_conv_wgrad"):
        M = c.get("M") or c["N"] * c["H"] * c["H"]
        return ["M"] * (M % 32 != 0) + ["Cout"] * (c.get("Cout", 0) % 64 != 0)
    if e.startswith("lfvdm_gn_bwd"):
        return ["P"] * (c["P"] % gn_pl(c["C0"] + c["C1"]) != 0) + ["ld"] * (c["pad"] > 0)
    if e == "lfvdm_gn_param_grads":
        return ["ld"] * (c["pad"] > 0) + ["C"] * (c["C"] % 64 != 0)
    if e == "lfvdm_rowdot_bwd_det":
        return ["O"] * any(o % 8 for o in c["O"]) + ["M"] * (c["M"] % 8 != 0) + ["ld"] * (c["lddin"] > c["K"])
    if e.startswith("lfvdm_rpe"):
        return ["rows"] * ((c["B"] * c["T"] * c["T"]) % 32 != 0) + ["ld"] * (c["pad"] > 0)
    if e == "lfvdm_gn_temporal_qkv":
        return ["M"] * ((c["B"] * c["T"] * c["P"]) % 32 != 0)
    if e == "lfvdm_proj_gn":
        return ["N"] * (c["N"] % 2 != 0)                # frames against the pairs of frames a workgroup takes at P = 64
    if e == "lfvdm_conv_igemm+lfvdm_gn_apply_part":
        return ["M"] * ((c["N"] * c["H"] * c["H"]) % 32 != 0) + ["ld"]
    if e.startswith("lfvdm_conv_out_update"):
        return ["pixels"] * ((c["B"] * c["T"] * c["H"] * c["W"]) % 64 != 0) + ["Cout"] * (c["Cout"] % 4 != 0)
    if e == "lfvdm_dyn_threshold":
        return ["elements"] * ((c["T"] * c["F"]) % 4 != 0)      # 185 elements per row: the last float4 / the last pass is ragged
    return ["ld"] * (c["rows_ld"] > c["row_floats"])


# deterministic sibling of every relaxed launch: it must be in the case lists too, under the bitwise rule
SIBLING = {"lfvdm_gn_bwd/atomics": "lfvdm_gn_bwd/det", "lfvdm_rowdot_bwd": "lfvdm_rowdot_bwd_det", "lfvdm_rpe_nets_bwd": "lfvdm_rpe_nets_bwd_det",
           "lfvdm_gn_temporal_bwd": "lfvdm_gn_temporal_bwd_det", "lfvdm_conv_wgrad/atomics": "lfvdm_conv_wgrad/slab"}


# operands the header promises are never read: a NaN-filled buffer in place of NULL must change nothing and stay untouched
NEVER_READ_CASES = [dict(entry="lfvdm_update_x0", what="x0-hat tables under LFVDM_MEAN_X0"),
                    dict(entry="lfvdm_update_x0", what="noise under the deterministic DDIM rule"),
                    dict(entry="lfvdm_update_x0", what="noise rows with t[b] == 0"),
                    dict(entry="lfvdm_update_rng_x0", what="x0-hat tables under LFVDM_MEAN_X0"),
                    dict(entry="lfvdm_update_rng_x0", what="noise_out / seed under the deterministic DDIM rule"),
                    dict(entry="lfvdm_update_ms_x0", what="x0-hat tables under LFVDM_MEAN_X0"),
                    dict(entry="lfvdm_update_ms_x0", what="hist rows with k3[t] == 0"),
                    dict(entry="lfvdm_known_blend", what="seed / noise_out with eps given")]

GPU_CASES = {"conv": CONV_CASES, "gn": GN_CASES, "attn_spatial": ATTN_SPATIAL_CASES, "attn_temporal": ATTN_TEMPORAL_CASES,
             "glue": GLUE_CASES, "bwd": BWD_CASES, "wgrad": WGRAD_CASES, "gn_bwd": GN_BWD_CASES, "train_glue": TRAIN_GLUE_CASES,
             "fused": FUSED_CASES}
OVERHANG = {"conv": conv_overhang, "gn": gn_overhang, "attn_spatial": attn_overhang, "attn_temporal": attn_overhang,
            "glue": glue_overhang, "bwd": bwd_overhang, "wgrad": train_overhang, "gn_bwd": train_overhang, "train_glue": train_overhang,
            "fused": train_overhang}


@pytest.mark.parametrize("family", list(GPU_CASES))
def test_every_gpu_case_overhangs_a_tile(family):
    assert GPU_CASES[family]
    for c in GPU_CASES[family]:
        assert OVERHANG[family](c), f"{family}: {c} has no overhanging dimension"
    names = [repr(sorted(c.items(), key=str)) for c in GPU_CASES[family]]
    assert len(set(names)) == len(names)


def test_conv_cases_cover_the_listed_edges():
    by = {c["name"]: c for c in CONV_CASES}
    assert by["3x3-ragged-M"]["N"] * 25 == 75 and by["linear-75x96x160"]["N"] * 25 == 75
    assert (by["stride2-odd-map"]["Ho"], by["stride2-odd-map"]["Wo"]) == (4, 4)
    assert {c["up"] for c in CONV_CASES} == {0, 1, 2, 3} and {by[f"up{u}"]["Ho"] for u in (1, 2, 3)} == {10}
    assert (by["concat-64+32"]["C0"], by["concat-64+32"]["C1"]) == (64, 32)
    assert {c["gn"]["skip_raw"] for c in CONV_CASES if "gn" in c} == {0, 1}
