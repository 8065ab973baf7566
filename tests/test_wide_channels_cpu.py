"""The yardstick of test_wide_channels_gpu: the conv family at the widths of the pixel-space model (BASELINE.json configs[4],
``cfgE_T2`` of test_oracle_golden: 128 base channels, channel_mult (1, 1, 2, 3, 4)), checked here without a GPU.

The layer list is derived from ``oracle.unet_oracle.param_shapes`` of that configuration: every distinct 3x3 conv
(C0, C1, Cout) and every 1x1 skip (S0, S1, Cout) whose input or output is wider than 256 channels, the concat split of a
decoder block taken from the encoder's skip stack.  The case lists below are literals and must cover that set.

Every case is a ``test_backward_nodes_cpu.Case``: inputs in channels-last rows, the operation in plain NCHW torch
(``F.conv2d``, ``F.interpolate(mode="nearest")``, ``F.group_norm`` with 32 groups, FiLM ``(1 + scale) * h + shift``, SiLU),
fp64 the reference, float32 on the CPU the model, and the bound ``Case.bound``: 4 x float32-model error + ATOL[kind] x
(1 + |ref|max), kind "igemm" for outputs and data gradients, "wgrad" for weight and bias gradients.  Maps are tiny (4x4,
4x8, 3x5; N in 2, 3, 5): the width is under test.

Checked here: the literals cover the derived set; every bound is finite and non-zero; and the bounds cannot hide a wrong
kernel - for every concat case the reference with the concat boundary one 32-channel chunk off, and the one with the last
32-channel K chunk dropped, sit more than 10 x the bound away in the output and in the weight gradient; so does the H / W
swapped reference of every non-square case, and the fused-GroupNorm reference with groups of 8 or 16 channels at Cout = 384
(12 channels per group)."""
import functools
import re

import torch
import torch.nn.functional as F

from oracle import unet_oracle as uo
from test_ops_gpu import rnd
from test_oracle_golden import CONFIGS
from test_backward_nodes_cpu import ATOL, Case, _w, _affine, nchw, to_rows, linear_case, conv_case, res_case

WIDE = 256      # "wide": more channels than any direct op test reached before

# (N, C0, C1, Cout, H, W, stride, up, skip): 3x3 conv over the virtual concat (src0 | src1) + residual; skip: the 1x1 skip
# segment over the same raw sources rides in the launch.  H, W: the SOURCE map (up: nearest-2x in front of the conv)
SINGLE_CASES = [(2, 256, 0, 384, 4, 4, 1, 0, 0), (3, 384, 0, 384, 4, 8, 1, 0, 0), (5, 384, 0, 512, 3, 5, 1, 0, 0),
                (2, 512, 0, 512, 4, 4, 1, 0, 0),
                (3, 256, 0, 384, 3, 5, 1, 0, 1), (2, 384, 0, 512, 4, 4, 1, 0, 1)]         # the encoder's channel-changing blocks
CONCAT_CHANNELS = [(2, 256, 128, 256, 4, 4), (3, 384, 256, 384, 4, 8), (5, 384, 384, 384, 3, 5), (2, 512, 384, 512, 4, 8),
                   (3, 512, 512, 512, 4, 4),
                   # the rest of what the model holds
                   (2, 512, 384, 384, 3, 5), (5, 384, 256, 256, 4, 4), (3, 256, 256, 256, 3, 5), (2, 256, 128, 128, 4, 8)]
CONCAT_CASES = [c + (1, 0, skip) for c in CONCAT_CHANNELS for skip in (0, 1)]
RESAMPLE_CASES = [(3, 384, 0, 384, 4, 8, 2, 0, 0), (2, 512, 0, 512, 4, 8, 2, 0, 0),       # Downsample
                  (3, 384, 0, 384, 2, 4, 1, 1, 0), (2, 512, 0, 512, 2, 4, 1, 1, 0)]       # Upsample (up = 1, and up = 3 at 512)
UP_PARITY_CASE = RESAMPLE_CASES[3]
FORWARD_CASES = SINGLE_CASES + CONCAT_CASES + RESAMPLE_CASES
# weight gradient only: concat sources under stride 2 and under the nearest-2x upsample, at 512 + 384
WGRAD_RESAMPLED_CONCAT = [(2, 512, 384, 512, 4, 8, 2, 0, 0), (2, 512, 384, 512, 2, 4, 1, 1, 0)]
WGRAD_OIHW_CASE = (2, 512, 384, 512, 4, 8, 1, 0, 0)
# (M, K, O, res): the attention blocks' 1x1 GEMMs, qkv and proj (+ residual)
LINEAR_CASES = [(M, K, O, res) for M in (70, 257) for K, O, res in ((384, 1152, False), (512, 1536, False), (384, 384, True),
                                                                     (512, 512, True))]
# (N, Cin, Cout, H, W, film): conv3x3 with the next GroupNorm32 (+ FiLM) + SiLU in its epilogue; (.., skip_raw) on the GPU
GN_CASES = [(4, 256, 384, 2, 2, True), (6, 384, 384, 4, 4, False), (4, 384, 384, 2, 4, True), (6, 384, 512, 2, 2, True),
            (4, 512, 512, 4, 4, False), (6, 512, 512, 2, 4, True)]
GN_SKIP_RAW = [False, False, True, True, False, False]
GN_T = 2
# (N, Cin, C0, C1, H, W): GroupNorm32 + SiLU of concat(conv3x3(x), skip), half by half
CONCAT_GN_CASES = [(4, 384, 384, 384, 2, 4), (6, 512, 512, 512, 2, 2), (4, 512, 512, 512, 4, 4)]
# (C0, C1, Cout) of the node tests (ResBlockFn on the concat, ConvFn on C0 -> Cout), 4x8 map
NODE_CHANNELS = [(384, 256, 384), (512, 384, 512)]
NODE_MAP = (4, 8)
NODE_CONV_CASES = [(2, C0, Cout, 4, 8, stride, up) for C0, _, Cout in NODE_CHANNELS for stride, up in ((1, False), (2, False), (1, True))]

KINDS = dict(out="igemm", dx0="igemm", dx1="igemm", dres="igemm", dw="wgrad", db="wgrad", dws="wgrad", dbs="wgrad")


# ------------------------------------------------------------------------------------------------------------------------
# the layer list of the model
# ------------------------------------------------------------------------------------------------------------------------
def model_layers():
    """-> (set of 3x3 (C0, C1, Cout), set of 1x1 skip (S0, S1, Cout)) of cfgE_T2 that are wider than WIDE on either side.
    param_shapes lists the parameters in execution order: the encoder pushes the width of every block's output, a decoder
    ResBlock pops the skip half of its concat."""
    shapes = uo.param_shapes(uo.make_cfg(**CONFIGS["cfgE_T2"][0]))
    convs, skips, stack, last = set(), set(), [], None
    for name, shape in shapes.items():
        m = re.match(r"(input_blocks|middle_block|output_blocks)\.(.*)\.weight$", name)
        if not m or len(shape) != 4:
            continue
        side, rest = m.groups()
        Cout, Cin = shape[:2]
        if rest == "0.0":                                           # the input conv
            stack.append(Cout)
        elif rest.endswith("in_layers.2"):
            C1 = stack.pop() if side == "output_blocks" else 0
            last = (Cin - C1, C1, Cout)
            convs.add(last)
            if side == "input_blocks":
                stack.append(Cout)
        elif rest.endswith("out_layers.3"):
            convs.add((Cin, 0, Cout))
        elif rest.endswith("skip_connection"):
            assert shape == (last[2], last[0] + last[1], 1, 1)
            skips.add(last)
        elif rest.endswith(".op") or rest.endswith(".conv"):
            convs.add((Cin, 0, Cout))
            if side == "input_blocks":
                stack.append(Cout)
        else:
            raise AssertionError(f"a conv this test does not know: {name}")
    assert not stack, "every encoder output is consumed by a decoder block"
    wide = lambda s: {c for c in s if c[0] + c[1] > WIDE or c[2] > WIDE}
    return wide(convs), wide(skips)


def test_the_case_lists_cover_the_models_wide_layers():
    convs, skips = model_layers()
    print(f"[wide] 3x3 convs of cfgE_T2 wider than {WIDE}: {sorted(convs)}")
    print(f"[wide] 1x1 skips of cfgE_T2 wider than {WIDE}: {sorted(skips)}")
    assert len(convs) >= 10 and len(skips) >= 8, "a change of the reference defaults must not empty the test"
    have = {c[1:4] for c in FORWARD_CASES}
    have_skip = {c[1:4] for c in FORWARD_CASES if c[8]}
    assert convs <= have, sorted(convs - have)
    assert skips <= have_skip, sorted(skips - have_skip)
    # the widths this file is about, whatever the model says
    assert {(256, 0, 384), (384, 0, 384), (384, 0, 512), (512, 0, 512), (256, 128, 256), (384, 256, 384), (384, 384, 384),
            (512, 384, 512), (512, 512, 512)} <= have
    widths = {c[2] for c in shapes_of_attention()}
    assert widths <= {K for _, K, _, _ in LINEAR_CASES}, widths
    assert {(C0, C1, Cout) for C0, C1, Cout in NODE_CHANNELS} <= convs


def shapes_of_attention():
    shapes = uo.param_shapes(uo.make_cfg(**CONFIGS["cfgE_T2"][0]))
    return {(k, v[0], v[1]) for k, v in shapes.items() if k.endswith("attention.qkv.weight") and v[1] > WIDE}


# ------------------------------------------------------------------------------------------------------------------------
# restatements and cases
# ------------------------------------------------------------------------------------------------------------------------
def wide_conv(t, N, H, W, C0, stride, up, wrong=None):
    """conv3x3(src0 | src1) (+ conv1x1 of the same raw concat) (+ res), rows in, rows out.  wrong: "boundary" - the 32 channels
    left of the concat boundary are read from the first chunk of src1 (a boundary one chunk early); "drop" - the last
    32-channel K chunk (tap (2, 2) of the 3x3, or the tail of the 1x1 segment, which comes last in K) contributes nothing."""
    x = nchw(t["x0"], N, H, W)
    if "x1" in t:
        x1 = nchw(t["x1"], N, H, W)
        x = torch.cat([x[:, :C0 - 32], x1[:, :32], x1], 1) if wrong == "boundary" else torch.cat([x, x1], 1)
    w, ws = t["w"], t.get("ws")
    if wrong == "drop":
        keep = torch.ones_like(ws if ws is not None else w)
        if ws is not None:
            keep[:, -32:] = 0
            ws = ws * keep
        else:
            keep[:, -32:, 2, 2] = 0
            w = w * keep
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    y = F.conv2d(xin, w, t["b"], stride=stride, padding=1)
    if ws is not None:
        y = y + F.conv2d(x, ws, t["bs"])
    y = to_rows(y)
    return y + t["res"] if "res" in t else y


def out_map(H, W, stride, up):
    Hi, Wi = (2 * H, 2 * W) if up else (H, W)
    return (Hi - 1) // stride + 1, (Wi - 1) // stride + 1


@functools.lru_cache(maxsize=None)
def wide_case(N, C0, C1, Cout, H, W, stride, up, skip, wrong=None):
    """Inputs and probe depend on the tag only: the wrong references of a case share them."""
    tag = f"wide/conv/{N}/{C0}/{C1}/{Cout}/{H}x{W}/{stride}/{up}/{skip}"
    Cin = C0 + C1
    Ho, Wo = out_map(H, W, stride, up)
    inputs = dict(x0=rnd(tag + "/x0", N * H * W, C0), w=_w(tag + "/w", Cout, Cin, 3, 3), b=0.1 * rnd(tag + "/b", Cout))
    if C1:
        inputs["x1"] = 1.5 * rnd(tag + "/x1", N * H * W, C1)
    if skip:
        inputs.update(ws=_w(tag + "/ws", Cout, Cin, 1, 1), bs=0.1 * rnd(tag + "/bs", Cout))
    if C1 or skip:
        inputs["res"] = rnd(tag + "/res", N * Ho * Wo, Cout)
    # biases and the residual see the probe's rows only, the 1x1 skip's weight gradient is a sum of per-row products
    return Case(tag, inputs, lambda t, h, w: wide_conv(t, N, h, w, C0, stride, up, wrong), KINDS, (N * Ho * Wo, Cout), (H, W),
                geo_free=["db", "dbs", "dws", "dres"])


def gn_conv(t, N, H, W, T, groups, skip=None):
    """-> rows [M][Cn + Cout]: SiLU(FiLM(GroupNorm(conv3x3(x) | skip))) | conv3x3(x), Cn = Cout (+ the skip's channels)."""
    raw = F.conv2d(nchw(t["x"], N, H, W), t["w"], t["b"], padding=1)
    h = raw if skip is None else torch.cat([raw, nchw(skip.to(raw.dtype), N, H, W)], 1)
    h = F.group_norm(h, groups, t["g"], t["be"], 1e-5)
    if "film" in t:
        Cn = h.shape[1]
        f = t["film"].repeat_interleave(T, dim=0)[:, :, None, None]
        h = h * (1 + f[:, :Cn]) + f[:, Cn:]
    return torch.cat([to_rows(F.silu(h)), to_rows(raw)], 1)


@functools.lru_cache(maxsize=None)
def gn_case(N, Cin, Cout, H, W, film, gw=0):
    """gw: channels per group (0: Cout / 32, the GroupNorm32 of the model)."""
    tag = f"wide/gn/{N}/{Cin}/{Cout}/{H}x{W}/{int(film)}"
    g, be = _affine(tag + "/n", Cout)
    inputs = dict(x=rnd(tag + "/x", N * H * W, Cin), w=_w(tag + "/w", Cout, Cin, 3, 3), b=0.1 * rnd(tag + "/b", Cout), g=g, be=be)
    if film:
        inputs["film"] = 0.3 * rnd(tag + "/film", N // GN_T, 2 * Cout)
    groups = Cout // gw if gw else 32
    return Case(tag, inputs, lambda t, h, w: gn_conv(t, N, h, w, GN_T, groups), dict(out="igemm"), (N * H * W, 2 * Cout), (H, W))


@functools.lru_cache(maxsize=None)
def concat_gn_case(N, Cin, C0, C1, H, W):
    tag = f"wide/catgn/{N}/{Cin}/{C0}/{C1}/{H}x{W}"
    g, be = _affine(tag + "/n", C0 + C1)
    inputs = dict(x=rnd(tag + "/x", N * H * W, Cin), w=_w(tag + "/w", C0, Cin, 3, 3), b=0.1 * rnd(tag + "/b", C0), g=g, be=be)
    skip = 1.5 * rnd(tag + "/skip", N * H * W, C1)
    c = Case(tag, inputs, lambda t, h, w: gn_conv(t, N, h, w, 1, 32, skip), dict(out="igemm"), (N * H * W, C0 + C1 + C0), (H, W))
    c.skip = skip
    return c


def part_bound(case, lo, hi):
    """Case.bound for the columns [lo, hi) of the output, as a tensor of its own."""
    ref = case.ref["out"][:, lo:hi]
    model = float((case.evaluate(torch.float32)["out"][:, lo:hi].double() - ref).abs().max())
    return 4 * model + ATOL["igemm"] * (1.0 + float(ref.abs().max())), model


def conv_cases():
    return [wide_case(*c) for c in FORWARD_CASES + WGRAD_RESAMPLED_CONCAT]


def all_cases():
    out = conv_cases() + [linear_case(M, K, O, res, True) for M, K, O, res in LINEAR_CASES]
    out += [gn_case(*c) for c in GN_CASES] + [concat_gn_case(*c) for c in CONCAT_GN_CASES]
    out += [conv_case(*c) for c in NODE_CONV_CASES] + [res_case(*c, *NODE_MAP) for c in NODE_CHANNELS]
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the bounds
# ------------------------------------------------------------------------------------------------------------------------
def test_every_case_uses_the_maps_and_batches_of_the_plan():
    for N, C0, C1, Cout, H, W, stride, up, skip in FORWARD_CASES + WGRAD_RESAMPLED_CONCAT:
        assert N in (2, 3, 5) and (H, W) in ((4, 4), (4, 8), (3, 5), (2, 4)), (N, H, W)
        assert (H, W) != (2, 4) or up, "2x4 is the source of an upsample"
        assert C0 % 32 == 0 and C1 % 32 == 0 and max(C0 + C1, Cout) > WIDE
    assert {c[4:6] for c in FORWARD_CASES} >= {(4, 4), (4, 8), (3, 5)} and {c[0] for c in FORWARD_CASES} == {2, 3, 5}
    assert WGRAD_OIHW_CASE in FORWARD_CASES and UP_PARITY_CASE[1:4] == (512, 0, 512)
    for (N, Cin, Cout, H, W, film) in GN_CASES:
        assert N in (4, 6) and (H, W) in ((2, 2), (4, 4), (2, 4)) and Cout in (384, 512)
    assert {(c[2], c[5], s) for c, s in zip(GN_CASES, GN_SKIP_RAW)} >= {(Cout, f, s) for Cout in (384, 512) for f, s in
                                                                       ((True, True), (False, False))}


def test_every_bound_is_finite_and_non_zero():
    n = 0
    for c in all_cases():
        for name in c.kinds:
            if name not in c.ref:
                continue
            b, m = c.bound(name), c.model_error(name)
            assert 0.0 < b < float("inf") and b == b, (c.tag, name, b)
            assert m <= 1e-3 * (1.0 + float(c.ref[name].abs().max())), (c.tag, name, m)      # the float32 model is a float32 model
            n += 1
    for c in [gn_case(*g) for g in GN_CASES] + [concat_gn_case(*g) for g in CONCAT_GN_CASES]:
        Cn = c.ref["out"].shape[1] - c.inputs["w"].shape[0]
        for lo, hi in ((0, Cn), (Cn, c.ref["out"].shape[1])):
            b, _ = part_bound(c, lo, hi)
            assert 0.0 < b < float("inf") and b == b, (c.tag, lo, hi, b)
            n += 1
    print(f"[wide] {n} bounds")


def _far(tag, name, wrong, ref, bound):
    d = float((wrong.reshape(-1) - ref.reshape(-1)).abs().max())
    print(f"[wide] {tag} {name}: wrong reference off by {d:.3e}, bound {bound:.3e}")
    assert d > 10 * bound, (tag, name, d, bound)


def test_a_misplaced_concat_boundary_or_a_dropped_chunk_cannot_hide_inside_a_bound():
    cases = [c for c in FORWARD_CASES + WGRAD_RESAMPLED_CONCAT if c[2]]
    assert len(cases) >= 10
    for args in cases:
        c = wide_case(*args)
        for wrong in ("boundary", "drop"):
            got = wide_case(*args, wrong=wrong).ref
            names = ["out", "dw"] + (["dws"] if args[8] else [])
            if wrong == "drop" and args[8]:
                names.remove("dw")          # the dropped chunk is the 1x1 segment's: the 3x3 weight gradient does not see it
            for name in names:
                _far(f"{c.tag} {wrong}", name, got[name], c.ref[name], c.bound(name))


def test_a_swapped_geometry_cannot_hide_inside_a_bound():
    cases = [c for c in conv_cases() + [gn_case(*g) for g in GN_CASES] + [concat_gn_case(*g) for g in CONCAT_GN_CASES]
             if c.geometry[0] != c.geometry[1]]
    assert len(cases) >= 15
    for c in cases:
        ref, swapped = c.ref, c.evaluate(torch.float64, transposed=True)
        for name in [k for k in c.kinds if k in ref]:
            d = float((swapped[name].reshape(-1) - ref[name].reshape(-1)).abs().max())
            if name in c.geo_free:
                assert d <= 1e-9 * (1 + float(ref[name].abs().max())), (c.tag, name, d)
                continue
            print(f"[wide] {c.tag} {name}: swapped geometry {d:.3e}, bound {c.bound(name):.3e}")
            assert d > 10 * c.bound(name), (c.tag, name, d, c.bound(name))


def test_a_wrong_group_width_cannot_hide_inside_a_bound():
    """Cout = 384: 12 channels per group.  Groups of 8 or 16 channels (what a tile of 64 or 128 columns would hold whole) must
    not pass for it."""
    cases = [g for g in GN_CASES if g[2] == 384]
    assert len(cases) >= 3
    for g in cases:
        c = gn_case(*g)
        bound, _ = part_bound(c, 0, 384)
        for gw in (8, 16):
            _far(c.tag, f"groups of {gw}", gn_case(*g, gw=gw).ref["out"][:, :384], c.ref["out"][:, :384], bound)
