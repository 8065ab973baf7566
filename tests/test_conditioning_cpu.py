"""The case lists of test_conditioning_gpu do what they are for, shown without a GPU: on every GroupNorm case a one-pass
E[x^2] - mean^2 variance in float32 misses the bound the kernel is held to (by >= 10 x in regime "b"), the softmax cases
reach the logit ranges they claim and are not one-hot everywhere, and the inputs of test_gn_apply_large_maps could not
have told a one-pass kernel from a two-pass one."""
import pytest
import torch

import test_conditioning_gpu as cg


def _condition(tag, one, bound, two, regime, shape_has_b):
    sep = one / bound
    print(f"[cond-cpu] {tag}: two-pass model {two:.3e}, one-pass model {one:.3e}, bound {bound:.3e}, one-pass / bound = {sep:.1f}")
    if regime == "b":
        assert sep >= 10, f"{tag}: the one-pass model misses the bound by only {sep:.2f} x"
    else:
        # regime a: |mean| / std = 64; float32 squares of 64 +- 1 carry 2.4e-4 of rounding against a variance of 1, so a
        # one-pass kernel errs by a few 1e-4 - above the two-pass model, not 10 x above the bound.  The shape's regime-b
        # case (the larger offset in units of the spread) carries the condition.
        assert shape_has_b, f"{tag}: no regime-b case for this shape"
        assert one > two


def _has_b(cases, case):
    return case[:-1] + ("b",) in cases


@pytest.mark.parametrize("case", cg.GN_APPLY_CASES)
def test_gn_apply_cases_separate(case):
    b = cg.gn_apply_case(*case)["bud"]
    _condition(f"gn_apply {case}", b["one"], b["bound"], b["two"], case[-1], _has_b(cg.GN_APPLY_CASES, case))


@pytest.mark.parametrize("case", cg.GN_WS_CASES)
def test_gn_apply_ws_cases_separate(case):
    b = cg.gn_ws_case(*case)["bud"]
    if case[6]:
        # the drifting mean (32 -> 96 over the pixels) gives the group a variance of about 340: a one-pass variance is fine
        # there; what this case must catch is a chunk merge that loses the between-chunk term
        sep = b["no_between"] / b["bound"]
        print(f"[cond-cpu] gn_apply_ws drift {case}: two-pass {b['two']:.3e}, merge without the between-chunk term "
              f"{b['no_between']:.3e}, bound {b['bound']:.3e}: {sep:.1f} x")
        assert sep >= 10
        return
    _condition(f"gn_apply_ws {case}", b["one"], b["bound"], b["two"], case[-1], _has_b(cg.GN_WS_CASES, case))


@pytest.mark.parametrize("case", cg.GN_COEF_CASES)
def test_gn_coef_cases_separate(case):
    b = cg.gn_coef_case(*case)["bud"]
    _condition(f"gn_coef {case}", b["one"], b["bound"], b["two"], case[-1], _has_b(cg.GN_COEF_CASES, case))


@pytest.mark.parametrize("case", cg.GNT_CASES)
def test_gn_temporal_cases_separate(case):
    b = cg.gnt_case(*case)["bud"]
    _condition(f"gn_temporal {case}", b["one"], b["bound"], b["two"], case[-1], _has_b(cg.GNT_CASES, case))


def test_gn_temporal_cases_reach_every_kernel():
    assert {cg._gnt_target(c[1], c[3]) for c in cg.GNT_CASES} == {"reg8", "reg16", "reg32", "general"}
    assert {cg._gnt_target(c[1], c[3]) for c in cg.GNT_BWD_CASES} >= {"general"} and len({c[:4] for c in cg.GNT_BWD_CASES}) == 2


@pytest.mark.parametrize("case", cg.GNT_QKV_CASES)
def test_gn_temporal_qkv_cases_separate(case):
    c = cg.gnt_qkv_case(*case)
    for which, b in (("xn", c["bud"]), ("qkv", c["bud_q"])):
        _condition(f"gn_temporal_qkv {which} {case}", b["one"], b["bound"], b["two"], case[-1], _has_b(cg.GNT_QKV_CASES, case))


@pytest.mark.parametrize("case", cg.PROJ_GN_CASES)
def test_proj_gn_cases_separate(case):
    b = cg.proj_gn_case(*case)["bud"]
    _condition(f"proj_gn {case}", b["one"], b["bound"], b["two"], case[-1], _has_b(cg.PROJ_GN_CASES, case))


@pytest.mark.parametrize("case", cg.CONV_GN_CASES)
def test_conv_fused_groupnorm_cases_separate(case):
    c = cg.conv_gn_case(*case)
    b = c["bud"]
    _condition(f"conv fused GroupNorm {case}", b["one"], b["bound"], b["two"], case[-1], _has_b(cg.CONV_GN_CASES, case))


@pytest.mark.parametrize("case", cg.CONCAT_GN_CASES)
def test_concat_groupnorm_cases_separate(case):
    b = cg.concat_gn_case(*case)["bud"]
    _condition(f"concat GroupNorm {case}", b["one"], b["bound"], b["two"], case[-1], _has_b(cg.CONCAT_GN_CASES, case))


def _bwd_condition(tag, b, regime):
    for i, name in enumerate(("dx", "dgamma", "dbeta")):
        sep = b["one"][i] / b["bound"][i]
        print(f"[cond-cpu] {tag} {name}: two-pass {b['two'][i]:.3e}, one-pass {b['one'][i]:.3e}, bound {b['bound'][i]:.3e}: {sep:.1f} x")
    # dx and dgamma carry the condition (dbeta does not depend on the statistics at all without an activation)
    if regime == "b":
        assert b["one"][0] / b["bound"][0] >= 10 and b["one"][1] / b["bound"][1] >= 10, tag
    else:
        assert b["one"][0] > b["two"][0] and b["one"][1] > b["two"][1]


@pytest.mark.parametrize("case", cg.GN_BWD_SMALL_CASES)
def test_gn_backward_small_cases_separate(case):
    C0, C1, pcls, N, T, act, film, regime = case
    assert regime == "b" or case[:-1] + ("b",) in cg.GN_BWD_SMALL_CASES
    P = cg._p_of(pcls, C0 + C1, 16 * cg._pl(C0 + C1))
    _bwd_condition(f"gn_bwd {case} P={P}", cg.gn_bwd_case(C0, C1, N, P, T, act, film, regime)["bud"], regime)


def test_gn_backward_small_cases_cover_every_split():
    from test_norm_backward_gpu import SPLITS
    assert {(c[0], c[1]) for c in cg.GN_BWD_SMALL_CASES} == set(SPLITS)


@pytest.mark.parametrize("case", cg.GN_BWD_WS_CASES)
def test_gn_backward_ws_cases_separate(case):
    N, P, C0, C1, film, act, regime = case
    _bwd_condition(f"gn_bwd_ws {case}", cg.gn_bwd_case(C0, C1, N, P, 2, act, film, regime)["bud"], regime)


@pytest.mark.parametrize("case", cg.GNT_BWD_CASES)
def test_gn_temporal_backward_cases_separate(case):
    _bwd_condition(f"gn_temporal_bwd {case}", cg.gnt_bwd_case(*case)["bud"], case[-1])


@pytest.mark.parametrize("case", cg.LARGE_MAPS_CASES)
def test_existing_large_maps_inputs_could_not_tell(case):
    """On the inputs of test_gn_apply_large_maps (* 1.3 + 0.7) the one-pass model passes that test's tolerance (3e-5): those
    inputs never pinned the two-pass statistics.  All six cases of that test."""
    b = cg.large_maps_inputs_one_pass_error(*case)
    print(f"[cond-cpu] test_gn_apply_large_maps inputs {case}: one-pass model {b['one']:.3e}, two-pass {b['two']:.3e} (tolerance 3e-5)")
    assert b["one"] < 3e-5


# ---- softmax -----------------------------------------------------------------------------------------------------------
def _logit_checks(tag, logits, attn, s):
    fin = logits[torch.isfinite(logits)]
    std, top = float(fin.std()), float(fin.max())
    frac = float((attn.max(-1).values < 0.99).float().mean())
    print(f"[cond-cpu] {tag} s={s:g}: logit std {std:.1f}, max {top:.1f}, rows with largest probability < 0.99: {100 * frac:.0f} %")
    return std, top, frac


@pytest.mark.parametrize("s", cg.SCALES)
@pytest.mark.parametrize("case", cg.ATTN_SPATIAL_CASES)
def test_attn_spatial_cases_reach_their_logits(case, s):
    N, P, Cc, heads, constructed = case
    c = cg.attn_spatial_case(*case, s)
    logits, attn = c["ref"]["logits"], c["ref"]["attn"]
    std, top, frac = _logit_checks(f"attn_spatial {case}", logits, attn, s)
    if constructed:
        last = (P - 1) // cg.KEY_BLOCK * cg.KEY_BLOCK
        assert bool((logits.argmax(-1) >= last).all()), "every query's largest logit lies in the last key block"
        gap = logits.max(-1).values - logits[..., :cg.KEY_BLOCK].max(-1).values
        print(f"[cond-cpu] attn_spatial constructed s={s:g}: the first block's maximum is {float(gap.min()):.1f} .. {float(gap.max()):.1f} below")
        assert float(gap.min()) >= 40
    else:
        assert 0.75 * s * s <= std <= 1.25 * s * s, std
        if s == 3.0:
            assert frac >= 0.25
    if s == 6.0:
        assert top > 88
    for k, v in c["model"].items():
        print(f"[cond-cpu]   {k}: float32 model {v:.3e}, bound {c['bound'][k]:.3e}")


@pytest.mark.parametrize("s", cg.SCALES)
@pytest.mark.parametrize("case", cg.ATTN_FUSED_CASES)
def test_attn_fused_cases_reach_their_logits(case, s):
    c = cg.attn_fused_case(*case, s)
    std, top, frac = _logit_checks(f"attn_spatial_fused {case}", c["logits"], c["attn"], s)
    assert 0.75 * s * s <= std <= 1.25 * s * s, std
    if s == 6.0:
        assert top > 88
    else:
        assert frac >= 0.25


@pytest.mark.parametrize("s", cg.SCALES)
@pytest.mark.parametrize("case", cg.ATTN_TEMPORAL_CASES)
def test_attn_temporal_cases_reach_their_logits(case, s):
    c = cg.attn_temporal_case(*case, s)
    std, top, frac = _logit_checks(f"attn_temporal {case}", c["logits"], c["attn"], s)
    assert 0.75 * s * s <= std <= 1.25 * s * s, std
    if s == 6.0:
        assert top > 88
    else:
        assert frac >= 0.25
    for k, v in c["model"].items():
        print(f"[cond-cpu]   {k}: float32 model {v:.3e}, bound {c['bound'][k]:.3e}")


@pytest.mark.parametrize("pattern", cg.MASK_PATTERNS)
def test_mask_patterns_are_what_they_say(pattern):
    B, T = 2, 7
    m = cg.mask_pattern(pattern, B, T)
    t = cg.lone_frame(pattern, T)
    ones = m.sum(1)
    if pattern == "zeros":
        assert float(ones.max()) == 0
    elif pattern.startswith("one_obs"):
        assert bool((ones == 1).all()) and bool((m[:, t] == 1).all())
    elif pattern == "one_latent":
        assert bool((ones == T - 1).all()) and bool((m[:, t] == 0).all())
    else:
        assert bool((m[:, ::2] == 1).all()) and bool((m[:, 1::2] == 0).all())
    if t is not None:       # the fp64 core itself: one-hot row, no gradient into q / k of the lone frame
        c = cg.attn_temporal_case(*cg.MASK_SHAPES[0], 3.0, pattern)
        row = c["attn"][:, :, :, t, :]
        assert float(row[..., t].min()) == 1.0 and float(row.sum(-1).max()) == 1.0
        d = c["ref"]["dqkv"].view(B, T, 5, 3, 64)[:, t]
        assert float(d[:, :, :2].abs().max()) == 0.0


def test_off_centre_local_stage_case_separates():
    """The off-centre case of test_chain_gpu.LOCAL_CASES (through the bias): condition and spread of the conv output."""
    import test_chain_gpu as tc
    for name in tc.OFF_CENTRE_LOCAL:
        assert name in tc.LOCAL_CASES
        raw, _, b = tc.local_stage_budget(name)
        _condition(f"local stage {name}", b["one"], b["bound"], b["two"], "b", True)
        gw = 128 // 32
        spread = float(raw.view(-1, 32, gw).std(-1).mean())
        assert float(raw.abs().mean()) > 60 and spread < 0.1, (float(raw.abs().mean()), spread)


def test_attn_temporal_cases_reach_every_kernel():
    """The dispatch restated (cg.temporal_kernels: T > 32 -> long window; B P F < 16384 and F in {16, 32, 64} -> second
    generation; else the first generation's <32> / <16> / <8>; backward rows: second generation for F in {16, 32, 64}, else
    the first generation): the saturated cases reach every forward and every backward kernel, and the mask patterns run on
    a second-generation and on a first-generation shape."""
    got = [cg.temporal_kernels(*c) for c in cg.ATTN_TEMPORAL_CASES]
    assert {f for f, _ in got} == {"gen2", "long", "gen1<32>", "gen1<16>", "gen1<8>"}
    assert {b for _, b in got} == {"gen2", "long", "gen1<16>", "gen1<8>"}
    assert [cg.temporal_kernels(*c) for c in cg.MASK_SHAPES] == [("gen2", "gen2"), ("gen1<8>", "gen1<8>")]
    B, T, P, Cc, heads = cg.ATTN_TEMPORAL_CASES[5]
    assert B * P * (Cc // heads) >= 16384 and Cc // heads == 32 and T <= 24
    for B, T, P, Cc, heads in cg.ATTN_TEMPORAL_CASES[:2] + cg.MASK_SHAPES[:1]:
        assert B * P * (Cc // heads) < 16384 and Cc // heads in (16, 32, 64) and T <= 32
