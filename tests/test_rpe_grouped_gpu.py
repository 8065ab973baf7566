"""Op-level fp64 parity of the three grouped launches that run every RPE network of a training step:

- lfvdm_rpe_nets_maxc with the hidden activations stored (lfvdm_rpe_job::act),
- lfvdm_rpe_nets_bwd and its deterministic form lfvdm_rpe_nets_bwd_det,
- lfvdm_conv_wgrad_grouped on the stored activations (the output layers' weight / bias gradients),

each alone and chained, through the C ABI, against ONE plain fp64 restatement of an RPENet (rpe.py:20-31) and its
autograd.  The shapes are the smallest at which the 32-row tile arithmetic of rpe_nets_bwd_kernel /
rpe_nets_bwd_reduce_kernel takes each of its paths (B, T -> M = B T^2 rows):

    1, 6   36 rows,  2 tiles   ragged last tile of 4 rows; `b_lo + 1 < B` is false
    2, 6   72 rows,  3 tiles   tile 1 straddles batch elements 0 / 1 at row 36; tile 2 ragged with b_lo = B - 1 (the clamp)
    3, 6  108 rows,  4 tiles   two consecutive straddling tiles (0 / 1, 1 / 2), then a ragged one
    2, 8  128 rows,  4 tiles   aligned (what the whole-model test has): the control
    2, 20 800 rows, 25 tiles   the production window: one straddling tile (rows 384..415), none ragged

and the widths C = 32 (only wave 0 works), 160 (wave 0 owns channel tiles 0 and 4), 512 (four tiles per wave, the LDS
maximum) at (2, 6), C = 128 at (2, 20), one width at each other shape, and one launch of three jobs of widths 64, 160, 32
at (3, 6) (the job lookup by tile0).  tproj differs by +1.5 b between batch elements, so a tile that uses the wrong
batch element's row is off by far more than any tolerance; tproj / dtproj are column views of wider buffers
(tproj_ld, dtproj_ld > C) whose other columns must stay bit-unchanged; R and act carry 32 guard rows behind row M.

Tolerances.  R and act: close(..., 2e-5), the bound of test_ops_gpu.py::test_rpe_nets.  Gradients: per case the same
RPENet also runs under torch autograd in float32 on the CPU; with e32 = max|g32 - g64| / max|g64| per gradient tensor,
the kernel must stay within 8 e32 (same normalisation, floor 1e-30 under the division).  The factor covers what the
float32 CPU run does not have (__expf and the reciprocal of the sigmoid, the k-ordered fp32 MFMA chain, the order of the
float atomics); it is a margin, not a measurement.  Every gradient check prints e32, the kernel's error and their ratio.

Measured on the MI355X: per launch and case the tensor with the largest ratio kernel error / e32 (both errors relative
to max|g64|), and the range of the ratio over the case's tensors.  No check needs more than 2.5 of the 8.

    launch          B, T   C            worst tensor    e32       kernel    ratio  (all tensors)
    bwd             1, 6   64           dtproj          1.35e-07  1.56e-07  1.15   (1.03..1.15)
    bwd             2, 6   32           dtproj          1.56e-07  2.42e-07  1.55   (0.53..1.55)
    bwd             2, 6   160          dWd             3.19e-07  4.55e-07  1.43   (1.06..1.43)
    bwd             2, 6   512          dbd             2.63e-07  5.35e-07  2.04   (1.70..2.04)
    bwd             3, 6   96           dbd             1.62e-07  2.40e-07  1.48   (0.85..1.48)
    bwd             2, 8   160          dtproj          2.62e-07  2.93e-07  1.11   (0.94..1.11)
    bwd             2, 20  128          dtproj          1.89e-07  1.77e-07  0.94   (0.54..0.94)
    bwd             3, 6   64+160+32    dWd / C64       2.75e-07  3.36e-07  1.22   (0.84..1.22)
    bwd_det         1, 6   64           dbd             1.35e-07  1.65e-07  1.22   (1.03..1.22)
    bwd_det         2, 6   32           dtproj          1.56e-07  2.42e-07  1.55   (0.55..1.55)
    bwd_det         2, 6   160          dWd             3.19e-07  4.55e-07  1.43   (1.06..1.43)
    bwd_det         2, 6   512          dbd             2.63e-07  5.35e-07  2.04   (1.70..2.04)
    bwd_det         3, 6   96           dbd             1.62e-07  2.41e-07  1.48   (0.88..1.48)
    bwd_det         2, 8   160          dtproj          2.62e-07  2.93e-07  1.11   (0.94..1.11)
    bwd_det         2, 20  128          dtproj          1.89e-07  1.92e-07  1.02   (0.64..1.02)
    bwd_det         3, 6   64+160+32    dWd / C160      2.76e-07  3.57e-07  1.29   (0.84..1.29)
    wgrad msplit 1  1, 6   64           dWout           1.42e-07  1.96e-07  1.38   (0.39..1.38)
    wgrad msplit 1  2, 6   32           dbout           7.38e-08  9.64e-08  1.31   (0.65..1.31)
    wgrad msplit 1  2, 6   160          dbout           9.32e-08  1.20e-07  1.28   (1.02..1.28)
    wgrad msplit 1  2, 6   512          dWout           2.27e-07  2.39e-07  1.05   (0.92..1.05)
    wgrad msplit 1  3, 6   96           dWout           2.49e-07  3.56e-07  1.43   (1.01..1.43)
    wgrad msplit 2  3, 6   96           dWout           2.49e-07  2.31e-07  0.93   (0.65..0.93)
    wgrad msplit 1  2, 8   160          dbout           1.66e-07  1.20e-07  0.72   (0.60..0.72)
    wgrad msplit 2  2, 8   160          dWout           5.87e-07  2.54e-07  0.43   (0.40..0.43)
    wgrad msplit 1  2, 20  128          dWout           3.76e-07  9.26e-07  2.46   (1.87..2.46)
    wgrad msplit 4  2, 20  128          dbout           1.04e-07  9.56e-08  0.92   (0.89..0.92)
    wgrad msplit 1  3, 6   64+160+32    dbout / C32     4.05e-08  6.37e-08  1.57   (0.98..1.57)
    wgrad msplit 2  3, 6   64+160+32    dbout / C64     4.53e-08  8.69e-08  1.92   (0.72..1.92)
    wgrad msplit 1  2, 6   64+160+32    dbout / C64     9.18e-08  1.12e-07  1.22   (0.60..1.22)
    chain           2, 20  128          dtproj          1.89e-07  2.39e-07  1.27   (0.62..1.27)
    chain           3, 6   64+160+32    dbout / C64     4.53e-08  8.69e-08  1.92   (0.82..1.92)

(The largest, 2.46, is the one launch in which a single wave adds all 25 row chunks of the production window in one
chain - msplit 1 - where the float32 CPU product sums blockwise.)

With `tp_hi` replaced by `tp_lo` in rpe_nets_bwd_kernel, and with the `s_hi` addition dropped from it and from the reduce
kernel (two arithmetic-only changes, tried on a copy), tests 2 and 3 fail at every width of (2, 6), at (3, 6) and at
(2, 20) with errors of 0.1 .. 1.3 of max|g64|, and pass at (1, 6) and at the aligned (2, 8).

lfvdm_conv_wgrad_grouped ACCUMULATES: conv_wgrad_grouped_kernel ends in det_add() with a null slab, i.e. atomicAdd into
`out` and `bias` - so its destinations are pre-filled with non-zero values like those of the backward entries.
GPU only."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import recipe
from test_ops_gpu import rnd, close

pytestmark = pytest.mark.gpu

E_SHAPE = 1             # LFVDM_E_SHAPE (include/lfvdm_hip.h)
TED = 64                # width of the time embedding that tproj is projected from
PAD = 4                 # columns between two networks' views in the wide tproj / dtproj buffers
GUARD = 32              # rows behind row M of R / act that no tile may write
DET_LD = 5 * 512        # floats of one tile's record in the deterministic workspace
MIXED = (64, 160, 32)

CASES = [(1, 6, (64,)), (2, 6, (32,)), (2, 6, (160,)), (2, 6, (512,)), (3, 6, (96,)), (2, 8, (160,)), (2, 20, (128,)),
         (3, 6, MIXED)]
CHAIN_CASES = [(2, 20, (128,)), (3, 6, MIXED)]
WGRAD_CASES = CASES + [(2, 6, MIXED)]


def _id(case):
    B, T, widths = case[:3]
    return f"B{B}-T{T}-C" + "+".join(str(c) for c in widths) + "".join(f"-msplit{m}" for m in case[3:])


def _build_msplit(B, T):
    """msplit as _RpeGroup._build computes it for the shape"""
    return max(1, min(4, ((B * T * T + 31) // 32) // 2))


WGRAD_PARAMS = [(B, T, w, m) for B, T, w in WGRAD_CASES for m in sorted({_build_msplit(B, T), 1})]


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from improved_diffusion import _native
    _native.lib()
    return _native


# ------------------------------------------------------------------------------------------------------------------------
# the reference: one RPENet in plain torch, any dtype, on the CPU
# ------------------------------------------------------------------------------------------------------------------------
def rpe_net(tproj, fi, Wd, bd, Wout, bout):
    """rpe.py:20-31 with the time projection given: R[b, t, s, :] and the hidden activations, in tproj's dtype."""
    d = (fi[:, :, None] - fi[:, None, :]).to(tproj.dtype)                                   # d = fi[b, t] - fi[b, s]
    feats = torch.stack([torch.log1p(d.clamp(min=0)), torch.log1p((-d).clamp(min=0)), (d == 0).to(tproj.dtype)], dim=-1)
    hid = tproj[:, None, None, :] + feats @ Wd.T + bd
    act = hid * torch.sigmoid(hid)
    return act @ Wout.T + bout, act


GRADS = ("dtproj", "dWd", "dbd", "dWout", "dbout")


def _autograd(net, fi, dtype):
    leaves = [net[k].to(dtype).requires_grad_(True) for k in ("tproj", "Wd", "bd", "Wout", "bout")]
    R, act = rpe_net(leaves[0], fi, *leaves[1:])
    (R.reshape(-1, R.shape[-1]) * net["dR"].to(dtype)).sum().backward()
    out = dict(zip(GRADS, (t.grad for t in leaves)))
    out.update(R=R.detach(), act=act.detach().reshape(-1, R.shape[-1]))
    return out


def _frame_indices(B, T):
    """Row 0: arange(T).  The others: sorted distinct draws from [0, 1000) with one gap above 900 (d == 0 on the diagonal only)."""
    gen = torch.Generator().manual_seed(1000 * B + T)
    rows = [torch.arange(T)]
    for b in range(1, B):
        lo = torch.randperm(90, generator=gen)[:T - 1].sort().values
        rows.append(torch.cat([lo, lo[-1:] + 901 + b]))
    fi = torch.stack(rows).to(torch.int64)
    assert int(fi.max()) < 1000 and bool((fi[:, 1:] > fi[:, :-1]).all())
    return fi


@functools.lru_cache(maxsize=None)
def _case(B, T, widths):
    """Inputs (float32, CPU) of every network of the launch, their fp64 results and gradients, and e32 per gradient tensor.
    Computed once per shape and shared by the tests; nothing in it is modified."""
    fi = _frame_indices(B, T)
    nets = []
    for i, C in enumerate(widths):
        tag = f"rg/{B}x{T}/{i}c{C}"
        shapes = {"Wd": ("embed_distances.weight", (C, 3)), "bd": ("embed_distances.bias", (C,)),
                  "Wt": ("embed_diffusion_time.weight", (C, TED)), "bt": ("embed_diffusion_time.bias", (C,)),
                  "Wout": ("out.weight", (C, C)), "bout": ("out.bias", (C,))}
        net = {k: torch.from_numpy(recipe.fill_param(f"{tag}.{name}", s)) for k, (name, s) in shapes.items()}
        net["tproj"] = (F.linear(rnd(tag + "/temb", B, TED), net["Wt"], net["bt"])
                        + 1.5 * torch.arange(B, dtype=torch.float32)[:, None]).contiguous()
        net["dR"] = rnd(tag + "/dR", B * T * T, C)
        net["C"] = C
        net["g64"] = _autograd(net, fi, torch.float64)
        g32 = _autograd(net, fi, torch.float32)
        net["e32"] = {k: float((g32[k].double() - net["g64"][k]).abs().max()) / max(float(net["g64"][k].abs().max()), 1e-30)
                      for k in GRADS}
        nets.append(net)
    return fi, nets


def tile_facts(B, T):
    """(tiles, straddling tiles, rows of the last tile) of the 32-row tiling of B * T * T rows"""
    TT, M = T * T, B * T * T
    tiles = (M + 31) // 32
    straddle = [t for t in range(tiles) if min(t * 32 + 31, M - 1) // TT != (t * 32) // TT]
    return tiles, straddle, M - (tiles - 1) * 32


def test_the_shapes_reach_what_they_are_meant_to():
    assert tile_facts(1, 6) == (2, [], 4)
    assert tile_facts(2, 6) == (3, [1], 8)
    assert tile_facts(3, 6) == (4, [1, 2], 12)
    assert tile_facts(2, 8) == (4, [], 32)
    assert tile_facts(2, 20) == (25, [12], 32)
    assert {c[:2] for c in CASES} == {(1, 6), (2, 6), (3, 6), (2, 8), (2, 20)}
    assert {w for B, T, w in CASES if (B, T) == (2, 6)} == {(32,), (160,), (512,)} and (2, 20, (128,)) in CASES
    assert {(B * T * T, w) for B, T, w in WGRAD_CASES if len(w) == 3} == {(72, MIXED), (108, MIXED)}
    assert {m for B, T, w, m in WGRAD_PARAMS if (B, T) == (2, 20)} == {1, 4}


# ------------------------------------------------------------------------------------------------------------------------
# one launch's device buffers and job tables
# ------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


class Launch:
    """Fresh device buffers for every network of a case: tproj / dtproj as column views of wide buffers (as _RpeGroup has
    them), R / act with GUARD rows behind row M and pre-filled with NaN, every gradient destination pre-filled with
    non-zero values, Wout_t packed by lfvdm_pack_conv_weight_t; and the three job tables."""

    def __init__(self, nat, B, T, widths, act_from_reference=False, msplit=None):
        self.nat, self.B, self.T, self.widths = nat, B, T, widths
        self.fi_cpu, self.nets = _case(B, T, widths)
        self.fi = self.fi_cpu.cuda()
        self.M = M = B * T * T
        self.tiles = (M + 31) // 32
        self.n = len(widths)
        self.total_tiles = self.n * self.tiles
        self.msplit = _build_msplit(B, T) if msplit is None else msplit
        wide = PAD + sum(c + PAD for c in widths)
        self.tproj_wide = torch.full((B, wide), 7.25, device="cuda")
        self.dtproj_pre = (0.25 * rnd(f"rg/{B}x{T}/dtproj_pre", B, wide)).cuda()
        self.dtproj_wide = self.dtproj_pre.clone()
        self.inside = torch.zeros(wide, dtype=torch.bool)
        self.dev, fj, bj, wj = [], [], [], []
        col, tile0, task0 = PAD, 0, 0
        for i, net in enumerate(self.nets):
            C = net["C"]
            d = {k: net[k].cuda() for k in ("Wd", "bd", "Wout", "bout", "dR")}
            d["tproj"], d["dtproj"] = self.tproj_wide[:, col:col + C], self.dtproj_wide[:, col:col + C]
            d["tproj"].copy_(net["tproj"])
            d["cols"] = (col, col + C)
            self.inside[col:col + C] = True
            d["R"] = torch.full((M + GUARD, C), float("nan"), device="cuda")
            d["act"] = torch.full((M + GUARD, C), float("nan"), device="cuda")
            if act_from_reference:
                d["act"][:M] = net["g64"]["act"].float().cuda()
            d["Wout_t"] = torch.empty(C, C, device="cuda")
            nat.pack_conv_weight_t(d["Wout"].view(C, C, 1, 1), d["Wout_t"])
            for k, shape in (("dWd", (C, 3)), ("dbd", (C,)), ("dWout", (C, C)), ("dbout", (C,))):
                d[k + "_pre"] = (0.25 * rnd(f"rg/{B}x{T}/{i}/{k}_pre", *shape)).cuda()
                d[k] = d[k + "_pre"].clone()
            fj.append(nat.RpeJob(d["tproj"].data_ptr(), d["Wd"].data_ptr(), d["bd"].data_ptr(), d["Wout"].data_ptr(),
                                 d["bout"].data_ptr(), d["R"].data_ptr(), C, tile0, self.tproj_wide.stride(0), 0,
                                 d["act"].data_ptr()))
            bj.append(nat.RpeBwdJob(d["tproj"].data_ptr(), d["Wd"].data_ptr(), d["bd"].data_ptr(), d["Wout_t"].data_ptr(),
                                    d["dR"].data_ptr(), d["dtproj"].data_ptr(), d["dWd"].data_ptr(), d["dbd"].data_ptr(), C, tile0,
                                    self.tproj_wide.stride(0), self.dtproj_wide.stride(0)))
            a = nat.fill_conv_args(src0=d["act"][:M], C0=C, N=M, Hs=1, Ws=1, Ho=1, Wo=1, ksize=1, res=d["dR"], ldr=C,
                                   out=d["dWout"], bias=d["dbout"], Cout=C)
            wj.append(nat.WgradJob(a, self.msplit, task0))
            self.dev.append(d)
            col += C + PAD
            tile0 += self.tiles
            task0 += (C // 32) * (C // 32) * self.msplit
        self.tasks = task0
        self.tproj_before = self.tproj_wide.clone()
        self.j_f, self.j_b, self.j_w = (nat.jobs_to_device(j, "cuda") for j in (fj, bj, wj))
        self.j_f_noact = nat.jobs_to_device([self._without_act(j) for j in fj], "cuda")

    def _without_act(self, j):
        return self.nat.RpeJob(j.tproj, j.Wd, j.bd, j.Wout, j.bout, j.R, j.C, j.tile0, j.tproj_ld, 0, None)

    # ---- the entries (return codes, not exceptions: the refusals are part of what is tested)
    def forward(self, max_channels, fi=None, T=None):
        fi = self.fi if fi is None else fi
        L = self.nat.lib()
        if max_channels is None:
            return L.lfvdm_rpe_nets(self.j_f.data_ptr(), self.n, self.total_tiles, fi.data_ptr(), self.B, T or self.T,
                                    self.nat.stream())
        return L.lfvdm_rpe_nets_maxc(self.j_f.data_ptr(), self.n, self.total_tiles, fi.data_ptr(), self.B, T or self.T,
                                     max_channels, self.nat.stream())

    def backward(self, fi=None, T=None):
        fi = self.fi if fi is None else fi
        return self.nat.lib().lfvdm_rpe_nets_bwd(self.j_b.data_ptr(), self.n, self.total_tiles, fi.data_ptr(), self.B,
                                                 T or self.T, self.nat.stream())

    def backward_det(self, ws, ws_floats=None, total_tiles=None, fi=None, T=None):
        fi = self.fi if fi is None else fi
        return self.nat.lib().lfvdm_rpe_nets_bwd_det(self.j_b.data_ptr(), self.n, total_tiles or self.total_tiles, fi.data_ptr(),
                                                     self.B, T or self.T, ws.data_ptr() if ws is not None else None,
                                                     (ws.numel() if ws is not None else 0) if ws_floats is None else ws_floats,
                                                     self.nat.stream())

    def wgrad(self):
        return self.nat.lib().lfvdm_conv_wgrad_grouped(self.j_w.data_ptr(), self.n, self.tasks, self.nat.stream())

    # ---- the checks
    def check_forward(self):
        torch.cuda.synchronize()
        for net, d in zip(self.nets, self.dev):
            for k in ("R", "act"):
                assert bool(torch.isnan(d[k][self.M:]).all()), f"{k}: a row behind M was written"
                close(d[k][:self.M], net["g64"][k].reshape(self.M, -1), 2e-5)
        self.check_views()

    def check_views(self):
        """the input is untouched, and so are the columns of the dtproj buffer that belong to no network"""
        torch.cuda.synchronize()
        assert torch.equal(_bits(self.tproj_wide), _bits(self.tproj_before))
        out = ~self.inside
        assert torch.equal(_bits(self.dtproj_wide.cpu()[:, out]), _bits(self.dtproj_pre.cpu()[:, out]))

    def check_grads(self, what, names):
        """prefill + fp64 gradient within 8 e32 of every named tensor of every network; prints every figure first"""
        torch.cuda.synchronize()
        bad = []
        for i, (net, d) in enumerate(zip(self.nets, self.dev)):
            for k in names:
                pre = self.dtproj_pre[:, d["cols"][0]:d["cols"][1]] if k == "dtproj" else d[k + "_pre"]
                g64 = self.want_grad(net, d, k)
                e32 = net["e32"][k]
                err = float((d[k].double().cpu() - (pre.double().cpu() + g64)).abs().max()) / max(float(g64.abs().max()), 1e-30)
                print(f"[rpe grouped] {what} B{self.B} T{self.T} job{i} C{net['C']} {k}: e32 {e32:.3e} kernel {err:.3e} "
                      f"ratio {err / max(e32, 1e-30):.2f}")
                if not err <= 8.0 * e32:
                    bad.append((i, k, err, e32))
        assert not bad, f"{what}: (job, tensor, kernel error, e32) beyond 8 e32: {bad}"

    def want_grad(self, net, d, k):
        return net["g64"][k]

    def untouched(self, names):
        """the named destinations still hold their prefill, bit for bit"""
        torch.cuda.synchronize()
        ok = "dtproj" not in names or torch.equal(_bits(self.dtproj_wide), _bits(self.dtproj_pre))
        return ok and all(torch.equal(_bits(d[k]), _bits(d[k + "_pre"])) for d in self.dev for k in names if k != "dtproj")

    def snapshot(self, names):
        torch.cuda.synchronize()
        return [_bits(self.dtproj_wide).clone()] + [_bits(d[k]).clone() for d in self.dev for k in names]


HIDDEN = ("dtproj", "dWd", "dbd")
OUTPUT = ("dWout", "dbout")


# ------------------------------------------------------------------------------------------------------------------------
# 1. forward with stored activations
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,widths", CASES, ids=[_id(c) for c in CASES])
def test_forward_with_stored_activations(nat, B, T, widths):
    """lfvdm_rpe_nets_maxc told the true maximum width, act and R pre-filled with NaN: both against fp64 at 2e-5; the same
    launch told 512, and plain lfvdm_rpe_nets, give bitwise the same R and act; max_channels 0 and 513 are refused."""
    a = Launch(nat, B, T, widths)
    assert a.forward(0) == E_SHAPE and a.forward(513) == E_SHAPE
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(d[k]).all()) for d in a.dev for k in ("R", "act")), "a refused launch wrote"
    assert a.forward(max(widths)) == 0
    a.check_forward()
    for mc in (512, None):
        b = Launch(nat, B, T, widths)
        assert b.forward(mc) == 0
        torch.cuda.synchronize()
        for da, db in zip(a.dev, b.dev):
            assert torch.equal(_bits(da["R"]), _bits(db["R"])) and torch.equal(_bits(da["act"]), _bits(db["act"])), mc
    # without `act` the launch computes the same R
    c = Launch(nat, B, T, widths)
    nat.check(nat.lib().lfvdm_rpe_nets_maxc(c.j_f_noact.data_ptr(), c.n, c.total_tiles, c.fi.data_ptr(), B, T, max(widths),
                                            nat.stream()), "lfvdm_rpe_nets_maxc")
    torch.cuda.synchronize()
    for da, dc in zip(a.dev, c.dev):
        assert torch.equal(_bits(da["R"]), _bits(dc["R"])) and bool(torch.isnan(dc["act"]).all())


# ------------------------------------------------------------------------------------------------------------------------
# 2. backward, atomics form
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,widths", CASES, ids=[_id(c) for c in CASES])
def test_backward_atomics(nat, B, T, widths):
    """lfvdm_rpe_nets_bwd accumulates into pre-filled dtproj / dWd / dbd: prefill + fp64 gradient within 8 e32."""
    a = Launch(nat, B, T, widths)
    assert a.backward() == 0
    a.check_grads("bwd", HIDDEN)
    a.check_views()
    assert a.untouched(OUTPUT)


# ------------------------------------------------------------------------------------------------------------------------
# 3. backward, deterministic form
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,widths", CASES, ids=[_id(c) for c in CASES])
def test_backward_deterministic(nat, B, T, widths):
    """lfvdm_rpe_nets_bwd_det with a workspace of exactly total_tiles * 5 * 512 floats, pre-filled with NaN (the reduce kernel
    must not read a word that no tile wrote): the comparison of the atomics form, and two runs bitwise equal."""
    runs = []
    for _ in range(2):
        a = Launch(nat, B, T, widths)
        ws = torch.full((a.total_tiles * DET_LD,), float("nan"), device="cuda")
        assert a.backward_det(ws) == 0
        runs.append(a.snapshot(HIDDEN))
    a.check_grads("bwd_det", HIDDEN)
    a.check_views()
    assert a.untouched(OUTPUT)
    assert all(torch.equal(x, y) for x, y in zip(*runs)), "two deterministic runs differ"


def test_backward_refusals(nat):
    """LFVDM_E_SHAPE, and no destination written: a workspace one float short, total_tiles no multiple of njobs, a null
    workspace, T * T < 32 (T = 5) in either form."""
    B, T = 3, 6
    a = Launch(nat, B, T, MIXED)
    full = a.total_tiles * DET_LD
    big = torch.full((full + DET_LD,), float("nan"), device="cuda")
    assert a.backward_det(big[:full - 1]) == E_SHAPE
    assert a.backward_det(big, ws_floats=full - 1) == E_SHAPE
    assert a.total_tiles % a.n == 0 and (a.total_tiles + 1) % a.n != 0
    assert a.backward_det(big, total_tiles=a.total_tiles + 1) == E_SHAPE
    assert a.backward_det(None) == E_SHAPE
    assert a.backward_det(None, ws_floats=full) == E_SHAPE
    fi5 = _frame_indices(B, 5).cuda()
    assert a.backward_det(big, fi=fi5, T=5) == E_SHAPE
    assert a.backward(fi=fi5, T=5) == E_SHAPE
    assert a.untouched(GRADS)
    assert bool(torch.isnan(big).all()), "a refused launch wrote its workspace"
    # the same tables are fine: the refusals above came from the arguments named
    assert a.backward_det(big[:full]) == 0
    a.check_grads("bwd_det after refusals", HIDDEN)


# ------------------------------------------------------------------------------------------------------------------------
# 4. grouped weight gradient of the output layers
# ------------------------------------------------------------------------------------------------------------------------
class WgradLaunch(Launch):
    """the stored activations are given (the fp64 ones rounded to fp32), so the expected values are exact in them"""

    def want_grad(self, net, d, k):
        act = d["act"][:self.M].double().cpu()
        return net["dR"].double().T @ act if k == "dWout" else net["dR"].double().sum(0)


@pytest.mark.parametrize("B,T,widths,msplit", WGRAD_PARAMS, ids=[_id(c) for c in WGRAD_PARAMS])
def test_grouped_weight_gradient(nat, B, T, widths, msplit):
    """lfvdm_conv_wgrad_grouped with jobs as _RpeGroup._build fills them (src0 = act, res = dR, ksize 1, Cout = C, task0 the
    prefix sum), at the msplit _build computes and at 1.  The kernel accumulates (float atomics into out / bias), so the
    destinations are pre-filled: prefill + fp64 dR^T act and dR.sum(0), within 8 e32."""
    a = WgradLaunch(nat, B, T, widths, act_from_reference=True, msplit=msplit)
    assert a.wgrad() == 0
    a.check_grads(f"wgrad msplit {msplit}", OUTPUT)
    assert a.untouched(HIDDEN)


# ------------------------------------------------------------------------------------------------------------------------
# 5. the three launches chained
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,widths", CHAIN_CASES, ids=[_id(c) for c in CHAIN_CASES])
def test_forward_backward_wgrad_chained(nat, B, T, widths):
    """Forward (storing act), backward on a random dR, weight gradient on the act the forward stored: R, act and the five
    gradients of an RPENet (time projection, both layers' weights and biases) against ONE fp64 autograd call - the
    op-level twin of test_backward_gpu.py::test_grouped_rpe_training_path_matches_per_network_path at shapes that straddle."""
    a = Launch(nat, B, T, widths)
    assert a.forward(max(widths)) == 0
    assert a.backward() == 0
    assert a.wgrad() == 0
    a.check_forward()
    a.check_grads("chain", GRADS)
