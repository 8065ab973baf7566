"""Persistent level chain (csrc/level_chain.hip) on the MI355X: ONE launch for a run of low-resolution stages must give
BITWISE the per-launch plan (same tile codes: every stage keeps its K-slice order and epilogue), replay after replay."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_oracle_golden import load_case
from test_forward_gpu import build_native
from test_sampler_gpu import make_diffusion

pytestmark = pytest.mark.gpu


def _sampler(model, shape, steps="", inject=False):
    from improved_diffusion.gaussian_diffusion import GraphSampler
    return GraphSampler(make_diffusion(1000, steps), model, shape, True, inject_noise=inject)


@pytest.mark.parametrize("local", [False, True])
def test_level_chain_is_bitwise_the_per_launch_plan(local, monkeypatch):
    """cfg B (BASELINE.json configs[1]): 40 steps through the replayed graphs (five 8-step launches), once with the 4x4 / 2x2
    levels as persistent chains and once with the same plan taken apart again.  Samples, x0 predictions and the noise of the
    last step must be equal bit for bit - a stale byte anywhere in a hand-off between two stages of a chain would show here -
    and no chain wait may have timed out.
    local = False (LFVDM_CHAIN_LOCAL=0): the split-K tile body in every stage; taken apart = ``disable_chains``, one
    lfvdm_conv_igemm / lfvdm_gn_apply launch per stage with the same tune codes.
    local = True (default): sample-local stages; taken apart = ``split_chains``, every stage a chain of its own (the same
    body and work items, ordered by launch boundaries instead of flags).  The per-launch TILE plan sums K in another order:
    it must agree within the forward tolerance, not bitwise."""
    monkeypatch.setenv("LFVDM_CHAIN_LOCAL", "1" if local else "0")
    from improved_diffusion import _native as nat
    cfg, sd, inp = load_case("cfgB")
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    shape = tuple(inp["x"].shape)
    outs, launches = [], []
    for mode in ("chained", "apart") + (("tiles",) if local else ()):
        s = _sampler(model, shape)
        s.begin(d["x"].clone(), mk)
        assert getattr(s.plan, "tuned", False)
        assert len(s.plan.chains) >= 2, "the encoder and decoder halves of the low-resolution levels"
        kinds = [k for c in s.plan.chains for k in c["kinds"]]
        assert (nat.CHAIN_LOCAL in kinds) == local
        if mode != "chained":
            if local and mode == "apart":
                s.plan.split_chains()
            else:
                s.plan.disable_chains()
            s.graph = s.graph_k = None
            s.begin(d["x"].clone(), mk)
            assert not s.plan.chains
        s.seed.fill_(4242)
        out = s.run(999, 40)
        torch.cuda.synchronize()
        assert not s.plan.chains_aborted()
        outs.append((out["sample"].clone(), out["pred_xstart"].clone(), s.noise.clone()))
        launches.append(len(s.plan.steps) + s.extra_launches)
        if mode == "chained":
            print("[chain] stages per chain:", [c["n"] for c in s.plan.chains], "kinds:", [c["kinds"] for c in s.plan.chains],
                  "work items:", [c["items"] for c in s.plan.chains], "grids:", [c["grid"] for c in s.plan.chains])
        del s
    print(f"[chain] launches per step: {launches[0]} chained, {launches[1]} per launch")
    assert launches[0] <= launches[1] - 15
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][0]).all())
    if local:       # 40 free-running steps against the tile plan: rounding only (same noise stream: bitwise equal draws)
        assert torch.equal(outs[0][2], outs[2][2])
        dev = float((outs[0][0] - outs[2][0]).abs().max())
        print(f"[chain] sample-local chains vs per-launch tile plan after 40 steps: max |d| = {dev:.3g}")
        assert dev <= 1e-4          # (observed 2.4e-7; a wrong GroupNorm half in one decoder stage gave ~1e-3 here)


def test_level_chain_eager_launches_repeat_bitwise():
    """The chain outside a graph: 30 eager forward launches on the same inputs (generation counter advancing every launch,
    flags never reset) give the same output every time, equal to the per-launch plan's."""
    cfg, sd, inp = load_case("cfgB")
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    from improved_diffusion._engine import Plan
    B, T, _, H, W = inp["x"].shape
    pl = Plan(model.native_engine(), B, T, H, W, False)
    pl.refresh_weights()
    pl.set_inputs(d["x"], d["x0"], torch.tensor([500.0, 20.0], device="cuda"), d["frame_indices"], d["obs_mask"], d["latent_mask"])
    pl.launch()
    pl.autotune()
    assert pl.chains
    ref = None
    for i in range(30):
        pl.launch()
        torch.cuda.synchronize()
        o = pl.out.clone()
        if ref is None:
            ref = o
        assert torch.equal(ref, o), i
    epoch = [int(c["ctl"][0].item()) for c in pl.chains]
    assert min(epoch) >= 30
    assert pl.split_chains() >= 20        # every stage a launch of its own: the same bodies, ordered by launch boundaries
    pl.launch()
    torch.cuda.synchronize()
    assert torch.equal(ref, pl.out)
    tile = Plan(model.native_engine(), B, T, H, W, False)       # and the plan without chains: rounding only
    tile.refresh_weights()
    tile.set_inputs(d["x"], d["x0"], torch.tensor([500.0, 20.0], device="cuda"), d["frame_indices"], d["obs_mask"], d["latent_mask"])
    tile.launch()
    torch.cuda.synchronize()
    assert float((tile.out - ref).abs().max()) <= 2e-4 + 1e-3 * float(ref.abs().max())


@pytest.mark.parametrize("name", ["cfgB_16x32", "cfgB_32x16", "cfgB_8x24"])
def test_chained_plan_at_nonsquare_latents_matches_the_fp64_fixture(name):
    """The bench model on non-square latents, planned as the sampler plans it: Plan -> autotune() (which builds the level
    chains) -> launch().  16x32 / 32x16: the bottom level is 2x4 / 4x2, so the chains hold sample-local stages of P = 8
    (two samples per 16-row tile).  8x24: no level's pixel count is a power of two - no sample-local stage may be chosen.
    The output must meet the fp64 fixture at the contract tolerance; ``split_chains`` (same bodies, one launch per
    stage) must be bitwise equal, the plan without chains (per-launch tile kernels) equal to rounding."""
    from improved_diffusion import _native as nat
    from improved_diffusion._engine import Plan
    from test_oracle_golden import compare_to_fixture, load_nonsquare
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"forward_{name}.npz"))
    cfg, sd, inp = load_nonsquare(name)
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    B, T, _, H, W = inp["x"].shape
    pl = Plan(model.native_engine(), B, T, H, W, False)
    pl.refresh_weights()
    pl.set_inputs(d["x"], d["x0"], d["t"].float(), d["frame_indices"], d["obs_mask"], d["latent_mask"])
    pl.launch()
    pl.autotune()
    pl.launch()
    torch.cuda.synchronize()
    kinds = [(st.kind, st.conv.Ho * st.conv.Wo if st.kind == nat.CHAIN_LOCAL else 0) for c in pl.chains for _, st in c["run"]]
    names = {nat.CHAIN_LOCAL: "local", nat.CHAIN_CONV: "tile", nat.CHAIN_GN: "gn"}
    print(f"[{name}] chains: {len(pl.chains)}, stages:", sorted({(names.get(k, k), P) for k, P in kinds}))
    if name == "cfgB_8x24":
        assert not any(k == nat.CHAIN_LOCAL for k, _ in kinds)
    else:
        assert pl.chains and any(k == nat.CHAIN_LOCAL and P == 8 for k, P in kinds)
        assert not any(c["ctl"][nat.CHAIN_CTL_ABORT].item() for c in pl.chains)
    ref = pl.out.clone()
    err = compare_to_fixture(ref, g, atol=1e-4, rtol=1e-3)
    print(f"[{name}] chained plan max|hip - fp64| = {err:.3e}")
    assert pl.split_chains() >= 1
    pl.launch()
    torch.cuda.synchronize()
    assert torch.equal(ref, pl.out)
    tile = Plan(model.native_engine(), B, T, H, W, False)           # no autotune: no chains
    tile.refresh_weights()
    tile.set_inputs(d["x"], d["x0"], d["t"].float(), d["frame_indices"], d["obs_mask"], d["latent_mask"])
    tile.launch()
    torch.cuda.synchronize()
    assert not tile.chains
    dev = float((tile.out - ref).abs().max())
    print(f"[{name}] per-launch tile plan vs chained: max|d| = {dev:.3g}")
    assert dev <= 1e-4 + 1e-3 * float(ref.abs().max())
    compare_to_fixture(tile.out, g, atol=1e-4, rtol=1e-3)


def test_a_raised_abort_word_makes_the_sampler_fall_back(capfd):
    """Every wait inside a chain is bounded: a poller that times out raises the chain's abort word, every other poller sees
    it and leaves.  The host side of that contract: ``p_sample_loop`` finds the word raised after the chain, says so on
    stderr, takes the plan apart into one launch per stage and runs the chain again - the caller gets valid samples."""
    from improved_diffusion import _native as nat
    cfg, sd, inp = load_case("cfgB")
    model = build_native(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    shape = tuple(inp["x"].shape)
    diff = make_diffusion(1000, "25")
    torch.manual_seed(11)
    a, _ = diff.p_sample_loop(model, shape, clip_denoised=True, model_kwargs=mk, return_decoded=False)
    s = diff._graph_sampler(model, shape, True)
    assert s.plan.chains and not s.chain_timed_out()
    s.plan.chains[0]["ctl"][nat.CHAIN_CTL_ABORT] = 1            # what a timed-out poller does
    b, _ = diff.p_sample_loop(model, shape, clip_denoised=True, model_kwargs=mk, return_decoded=False)
    err = capfd.readouterr().err
    assert "persistent level chain timed out" in err
    assert not s.plan.chains and s.chain_timeouts == 1 and bool(torch.isfinite(b).all())
    n_steps = len(s.plan.steps)
    c, _ = diff.p_sample_loop(model, shape, clip_denoised=True, model_kwargs=mk, return_decoded=False)      # stays per launch
    assert len(s.plan.steps) == n_steps and not s.plan.chains and bool(torch.isfinite(c).all())


# ------------------------------------------------------------------------------------------- sample-local stages (round 6)
def _launch_chain(stage_list, timeout_s=2.0):
    """Plan and launch a chain of ChainStage objects once (tensors the stages point at are the caller's)."""
    import ctypes as C
    from improved_diffusion import _native as nat
    L = nat.lib()
    n = len(stage_list)
    stages = (nat.ChainStage * n)(*stage_list)
    cap = 1 << 18
    deps = (C.c_int32 * cap)()
    used, ws_f, cnt_i = C.c_int64(), C.c_int64(), C.c_int64()
    n_flags, grid, lds = C.c_int32(), C.c_int32(), C.c_int32()
    rc = L.lfvdm_chain_plan(stages, n, deps, cap, C.byref(used), C.byref(n_flags), C.byref(ws_f), C.byref(cnt_i), C.byref(grid),
                            C.byref(lds))
    assert rc == 0, rc
    assert grid.value <= L.lfvdm_chain_capacity(lds.value)
    ws = torch.empty(max(1, ws_f.value), device="cuda")
    cnt = torch.zeros(max(1, cnt_i.value), dtype=torch.int32, device="cuda")
    for i in range(n):
        cv = stages[i].conv
        cv.splitk_ws, cv.splitk_cnt = ws.data_ptr() + 4 * stages[i].ws_off, cnt.data_ptr() + 4 * stages[i].cnt_off
        cv.splitk_ws_floats, cv.splitk_cnt_ints = ws.numel() - stages[i].ws_off, cnt.numel() - stages[i].cnt_off
    stages_dev = torch.frombuffer(bytearray(bytes(memoryview(stages))), dtype=torch.uint8).cuda()
    deps_dev = torch.frombuffer(bytearray(bytes(memoryview(deps))[:4 * max(1, used.value)]), dtype=torch.int32).cuda()
    flags = torch.zeros(max(1, n_flags.value), dtype=torch.int32, device="cuda")
    ctl = torch.zeros(nat.CHAIN_CTL_INTS, dtype=torch.int32, device="cuda")
    for _ in range(2):          # twice: the generation counter advances, nothing is reset
        nat.check(L.lfvdm_level_chain(stages_dev.data_ptr(), n, deps_dev.data_ptr(), flags.data_ptr(), ctl.data_ptr(), grid.value,
                                      lds.value, timeout_s, nat.stream()), "lfvdm_level_chain")
    torch.cuda.synchronize()
    assert int(ctl[nat.CHAIN_CTL_ABORT].item()) == 0
    return [s.n_items for s in stages], grid.value


LOCAL_CASES = {
    # name: (N, Hs, Ws, Ho, Wo, ksize, stride, up, C0, C1, s2C0, s2C1, Cout, res, gn (None | (film, skip_raw, gw, ld)), rt)
    "res2x2_gn_film": (40, 2, 2, 2, 2, 3, 1, 0, 128, 0, 0, 0, 128, False, (True, 1, 0, 0), 1),
    "res2x2_residual_raw": (40, 2, 2, 2, 2, 3, 1, 0, 128, 0, 0, 0, 128, True, None, 1),
    "res2x2_residual_gn_both": (40, 2, 2, 2, 2, 3, 1, 0, 128, 0, 0, 0, 128, True, (False, 0, 0, 0), 1),
    "down8to4": (40, 8, 8, 4, 4, 3, 2, 0, 128, 0, 0, 0, 128, False, (False, 0, 0, 0), 2),
    "down8to4_rt1": (40, 8, 8, 4, 4, 3, 2, 0, 128, 0, 0, 0, 128, False, (False, 0, 0, 0), 1),
    "down4to2": (40, 4, 4, 2, 2, 3, 2, 0, 128, 0, 0, 0, 128, False, (False, 0, 0, 0), 1),
    "up2to4_cat_half": (40, 2, 2, 4, 4, 3, 1, 1, 128, 0, 0, 0, 128, False, (False, 0, 8, 256), 2),
    "skip_segment_cat_half": (40, 2, 2, 2, 2, 3, 1, 0, 128, 0, 128, 128, 128, False, (False, 0, 8, 256), 1),
    "skip_segment_4x4_rt2": (40, 4, 4, 4, 4, 3, 1, 0, 128, 0, 128, 64, 128, False, None, 2),
    "proj1x1_residual_gn": (40, 2, 2, 2, 2, 1, 1, 0, 128, 0, 0, 0, 128, True, (False, 0, 0, 0), 1),
    "res4x4_rt1": (40, 4, 4, 4, 4, 3, 1, 0, 128, 0, 0, 0, 128, False, (True, 1, 0, 0), 1),
    "res4x4_rt2": (40, 4, 4, 4, 4, 3, 1, 0, 128, 0, 0, 0, 128, True, (True, 0, 0, 0), 2),
    "batch1_ragged_rows": (6, 2, 2, 2, 2, 3, 1, 0, 128, 0, 0, 0, 128, True, (True, 0, 0, 0), 1),
    "ragged_rt2": (5, 4, 4, 4, 4, 3, 1, 0, 64, 0, 0, 0, 64, True, (True, 0, 0, 0), 2),
    "wide_256_gw8": (20, 2, 2, 2, 2, 3, 1, 0, 64, 0, 0, 0, 256, False, (True, 1, 0, 0), 1),
    "narrow_64_gw2": (20, 2, 2, 2, 2, 3, 1, 0, 64, 0, 0, 0, 64, True, (True, 0, 0, 0), 1),
    "wide_512_gw16_concat_source": (8, 2, 2, 2, 2, 3, 1, 0, 64, 64, 0, 0, 512, False, (False, 0, 0, 0), 1),
    "map4x1": (12, 4, 1, 4, 1, 1, 1, 0, 192, 0, 0, 0, 64, False, None, 1),
    "cin192_3x3_runtime_loop": (8, 2, 2, 2, 2, 3, 1, 0, 192, 0, 0, 0, 64, True, (True, 0, 0, 0), 1),      # 3 units per tap and wave: no instance
    "cin256_1x1": (12, 4, 4, 4, 4, 1, 1, 0, 256, 0, 0, 0, 128, True, (False, 0, 0, 0), 2),
    "cin512_1x1_runtime_loop": (6, 2, 2, 2, 2, 1, 1, 0, 256, 256, 0, 0, 64, False, None, 1),
    "cin64_3x3_rt2": (10, 4, 4, 4, 4, 3, 1, 0, 64, 0, 64, 0, 64, False, (True, 1, 0, 0), 2),
    # P = 8: two samples per 16-row tile (the bottom level of a 16x32 / 32x16 latent with channel_mult (1, 2, 2, 2))
    "map2x4_gn_film": (40, 2, 4, 2, 4, 3, 1, 0, 128, 0, 0, 0, 128, False, (True, 0, 0, 0), 1),
    "map4x2_residual_gn_rt2": (40, 4, 2, 4, 2, 3, 1, 0, 128, 0, 0, 0, 128, True, (False, 0, 0, 0), 2),
    "map8x1_gw2_skip_raw": (20, 8, 1, 8, 1, 3, 1, 0, 64, 0, 0, 0, 64, True, (True, 1, 0, 0), 1),
    "map1x8_gw8_ragged_rt2": (10, 1, 8, 1, 8, 3, 1, 0, 64, 0, 0, 0, 256, False, (True, 0, 0, 0), 2),
    "map2x4_gw16_concat_source": (6, 2, 4, 2, 4, 3, 1, 0, 64, 64, 0, 0, 512, True, (False, 0, 0, 0), 1),
    "down4x8_to_2x4_rt2": (40, 4, 8, 2, 4, 3, 2, 0, 128, 0, 0, 0, 128, False, (True, 1, 0, 0), 2),
    "down4x8_to_2x4_ragged": (13, 4, 8, 2, 4, 3, 2, 0, 64, 0, 0, 0, 64, True, (True, 0, 0, 0), 1),
    "up1x2_to_2x4_cat_half": (40, 1, 2, 2, 4, 3, 1, 1, 128, 0, 0, 0, 128, False, (False, 0, 8, 256), 2),
    "skip_segment_concat_2x4": (40, 2, 4, 2, 4, 3, 1, 0, 128, 0, 128, 64, 128, True, (True, 0, 0, 0), 1),
    "cat_half_4x2": (40, 4, 2, 4, 2, 3, 1, 0, 128, 0, 0, 0, 128, False, (False, 0, 8, 256), 2),
    # P = 2 and P = 1: eight / sixteen samples per tile (the bottom levels of 8x16 and 4x8 latents)
    "map1x2_gn_film": (40, 1, 2, 1, 2, 3, 1, 0, 128, 0, 0, 0, 128, True, (True, 0, 0, 0), 1),
    "map2x1_gw2_ragged_rt2": (21, 2, 1, 2, 1, 3, 1, 0, 64, 0, 0, 0, 64, False, (True, 1, 0, 0), 2),
    "down2x4_to_1x2": (40, 2, 4, 1, 2, 3, 2, 0, 128, 0, 0, 0, 128, True, (False, 0, 0, 0), 1),
    "map1x1_gw8": (40, 1, 1, 1, 1, 3, 1, 0, 64, 0, 0, 0, 256, True, (True, 0, 0, 0), 1),
    "down2x2_to_1x1_rt2_ragged": (23, 2, 2, 1, 1, 3, 2, 0, 128, 0, 0, 0, 128, False, (True, 1, 0, 0), 2),
    # off centre through the bias (+-64 alternating per group, conv output std about 0.05): the GroupNorm statistics of the
    # stage see |mean| / std of about 1280 while the conv itself stays well conditioned (test_conditioning_*)
    "off_centre_bias_4x4": (40, 4, 4, 4, 4, 3, 1, 0, 128, 0, 0, 0, 128, False, (True, 1, 0, 0), 1),
}
OFF_CENTRE_LOCAL = {"off_centre_bias_4x4": (64.0, 0.05)}


def _local_stage_f64(N, Hs, Ws, Ho, Wo, k, stride, up, src0, src1, W, b, s2a, s2b, W2, b2, resid, gn, gamma, beta, film, T):
    """fp64 restatement of one stage (include/lfvdm_hip.h, lfvdm_conv_args): conv over the (upsampled) concat source, 1x1
    skip segment, residual -> raw rows; GroupNorm of gw-channel groups per sample, affine, FiLM, SiLU -> normalised rows."""
    d = lambda t: t.double().cpu()      # noqa: E731
    Cout = W.shape[0]
    x = d(src0) if src1 is None else torch.cat([d(src0), d(src1)], 1)
    x = x.view(N, Hs, Ws, -1).permute(0, 3, 1, 2)
    if up:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    w = d(W).view(Cout, k, k, -1).permute(0, 3, 1, 2)
    y = F.conv2d(x, w, d(b), stride=stride, padding=k // 2)
    assert y.shape[2:] == (Ho, Wo)
    y = y.permute(0, 2, 3, 1).reshape(N * Ho * Wo, Cout)
    if s2a is not None:
        s = d(s2a) if s2b is None else torch.cat([d(s2a), d(s2b)], 1)
        y = y + s @ d(W2).t() + d(b2)
    if resid is not None:
        y = y + d(resid)
    if not gn:
        return y, None
    use_film, _, gw, _ = gn
    gw = gw or Cout // 32
    g = F.group_norm(y.view(N, Ho * Wo, Cout).transpose(1, 2), Cout // gw, d(gamma), d(beta), eps=1e-5).transpose(1, 2)
    if use_film:
        f = d(film).repeat_interleave(T, dim=0)[:, None]
        g = g * (1 + f[..., :Cout]) + f[..., Cout:]
    return y, F.silu(g).reshape(N * Ho * Wo, Cout)


def _local_inputs(name, dev):
    """The operands of one LOCAL_CASES stage (seeded by the case's name) on ``dev``."""
    import zlib
    N, Hs, Ws, Ho, Wo, k, stride, up, C0, C1, s2C0, s2C1, Cout, res, gn, rt = LOCAL_CASES[name]
    T = 2 if N % 2 == 0 else 1
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 1000)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)      # noqa: E731
    Cin, C2, taps = C0 + C1, s2C0 + s2C1, k * k
    M, Min = N * Ho * Wo, N * Hs * Ws
    src0, src1 = rn(Min, C0), (rn(Min, C1) if C1 else None)
    W, b = rn(Cout, taps, Cin) / (taps * Cin) ** 0.5, 0.1 * rn(Cout)
    s2a, s2b = (rn(M, s2C0) if s2C0 else None), (rn(M, s2C1) if s2C1 else None)
    W2, b2 = (rn(Cout, C2) / C2 ** 0.5 if C2 else None), (0.1 * rn(Cout) if C2 else None)
    resid = rn(M, Cout) if res else None
    gamma, beta, film = 1.0 + 0.1 * rn(Cout), 0.1 * rn(Cout), 0.3 * rn(N // T, 2 * Cout)
    if name in OFF_CENTRE_LOCAL:
        mean, std = OFF_CENTRE_LOCAL[name]
        gw = (gn[2] or Cout // 32)
        sign = (1.0 - 2.0 * ((torch.arange(Cout) // gw) % 2).float()).to(dev)
        W, b = (W * std).contiguous(), mean * sign + std * b
    return src0, src1, W, b, s2a, s2b, W2, b2, resid, gamma, beta, film


def local_stage_budget(name):
    """(fp64 raw rows, fp64 normalised rows, budget) of an OFF_CENTRE_LOCAL case: the bound of test_conditioning_gpu (4 x the
    float32 two-pass model + this test's 1e-4) in place of the fixed tolerance.  CPU only."""
    from test_conditioning_gpu import computed_budget, _affine
    N, Hs, Ws, Ho, Wo, k, stride, up, C0, C1, s2C0, s2C1, Cout, res, gn, rt = LOCAL_CASES[name]
    T = 2 if N % 2 == 0 else 1
    src0, src1, W, b, s2a, s2b, W2, b2, resid, gamma, beta, film = _local_inputs(name, "cpu")
    raw, ref = _local_stage_f64(N, Hs, Ws, Ho, Wo, k, stride, up, src0, src1, W, b, s2a, s2b, W2, b2, resid, gn, gamma, beta, film, T)
    post = lambda r: _affine(r, N, Ho * Wo, Cout, gamma, beta, film if gn[0] else None, T, 1)      # noqa: E731
    return raw, ref, computed_budget(raw, N, Ho * Wo, Cout, gn[2] or Cout // 32, post, ref, 1e-4)


@pytest.mark.parametrize("name", sorted(LOCAL_CASES))
def test_sample_local_stage_matches_the_tile_kernel(name):
    """One LFVDM_CHAIN_LOCAL stage (csrc/conv_local_body.h: whole samples x 16 filters x all of K per work item, MFMA
    16x16x4, GroupNorm by lane butterflies) against the stand-alone implicit-GEMM launch on the same lfvdm_conv_args and
    against an fp64 restatement: every operand form the low-resolution levels use (unet.py:194-207 ResBlocks with FiLM,
    :91-114 / :60-88 resampling, the 1x1 skip segment on a raw concat, residuals, the concat-half normalisation gn_gw /
    gn_ld, ragged last items) on every map the stage accepts - P = Ho*Wo of 1, 2, 4, 8 and 16, square or not.  fp32,
    different K order: local vs tile |d| <= 2e-5 * (1 + |ref|max); both vs fp64 1e-4 (normalised) / 5e-5 (raw)."""
    import ctypes as C
    from improved_diffusion import _native as nat
    N, Hs, Ws, Ho, Wo, k, stride, up, C0, C1, s2C0, s2C1, Cout, res, gn, rt = LOCAL_CASES[name]
    T = 2 if N % 2 == 0 else 1
    Cin, C2, M = C0 + C1, s2C0 + s2C1, N * Ho * Wo
    src0, src1, W, b, s2a, s2b, W2, b2, resid, gamma, beta, film = _local_inputs(name, "cuda")
    ref_raw, ref_gn = _local_stage_f64(N, Hs, Ws, Ho, Wo, k, stride, up, src0, src1, W, b, s2a, s2b, W2, b2, resid, gn, gamma,
                                       beta, film, T)
    outs = []
    for local in (False, True):
        a = nat.ConvArgs()
        a.src0, a.src1, a.C0, a.C1, a.N, a.Hs, a.Ws, a.Ho, a.Wo = src0.data_ptr(), src1.data_ptr() if C1 else None, C0, C1, N, Hs, Ws, Ho, Wo
        a.up, a.stride, a.ksize, a.W, a.bias, a.Cout = up, stride, k, W.data_ptr(), b.data_ptr(), Cout
        if C2:
            a.s2src0, a.s2src1, a.s2C0, a.s2C1 = s2a.data_ptr(), s2b.data_ptr() if s2C1 else None, s2C0, s2C1
            a.W2, a.bias2 = W2.data_ptr(), b2.data_ptr()
        if res:
            a.res, a.ldr = resid.data_ptr(), Cout
        raw = torch.full((M, Cout), 7.0, device="cuda")
        a.out, a.ldo, a.out_mode = raw.data_ptr(), Cout, nat.OUT_ROWS
        gout = None
        if gn:
            use_film, skip_raw, gw, ld = gn
            gout = torch.full((M, ld or Cout), 7.0, device="cuda")
            a.gn_gamma, a.gn_beta, a.gn_out = gamma.data_ptr(), beta.data_ptr(), gout.data_ptr()
            if use_film:
                a.gn_film, a.gn_film_ld, a.gn_film_div = film.data_ptr(), 2 * Cout, T
            else:
                a.gn_film_div = 1
            a.gn_act, a.gn_skip_raw, a.gn_eps, a.gn_gw, a.gn_ld = nat.ACT_SILU, skip_raw, 1e-5, gw, ld
        if local:
            assert nat.lib().lfvdm_chain_local_ok(C.byref(a), rt) == 0
            st = nat.ChainStage()
            st.kind, st.cfg = nat.CHAIN_LOCAL, rt
            C.memmove(C.byref(st.conv), C.byref(a), C.sizeof(nat.ConvArgs))
            items, grid = _launch_chain([st])
            assert items[0] == -(-M // (16 * rt)) * (Cout // 16) and grid % 8 == 0
        else:
            ws, cnt = nat.splitk_workspace(torch.device("cuda", torch.cuda.current_device()))
            a.splitk_ws, a.splitk_cnt, a.splitk_ws_floats, a.splitk_cnt_ints = ws.data_ptr(), cnt.data_ptr(), ws.numel(), cnt.numel()
            a.tune = 0
            nat.check(nat.lib().lfvdm_conv_igemm(C.byref(a), nat.stream()), "lfvdm_conv_igemm")
            torch.cuda.synchronize()
        outs.append((raw, gout))
    (r0, g0), (r1, g1) = outs
    if not (gn and gn[1]):
        tol = 2e-5 * (1.0 + float(r0.abs().max()))
        assert float((r0 - r1).abs().max()) <= tol, (name, float((r0 - r1).abs().max()))
        for which, r in (("tile", r0), ("local", r1)):
            dev = float((r.double().cpu() - ref_raw).abs().max())
            assert dev <= 5e-5, (name, which, "raw vs fp64", dev)
    else:
        assert bool((r1 == 7.0).all()), "gn_skip_raw: the raw tensor is not written"
    if gn:
        limit = 1e-4
        tol = 2e-5 * (1.0 + float(g0.abs().max()))
        if name in OFF_CENTRE_LOCAL:        # each form within the conditioning bound of fp64, so within twice that of each other
            bud = local_stage_budget(name)[2]
            limit, tol = bud["bound"], 2 * bud["bound"]
            print(f"[cond] local stage {name}: two-pass model {bud['two']:.3e}, one-pass model {bud['one']:.3e}, bound {limit:.3e}")
        devs = {"local-tile": float((g0[:, :Cout] - g1[:, :Cout]).abs().max())}
        for which, gg in (("tile", g0), ("local", g1)):
            devs[which] = float((gg[:, :Cout].double().cpu() - ref_gn).abs().max())
        print(f"[local] {name}: P = {Ho * Wo}, normalised max|d| " + ", ".join(f"{k_} {v:.3g}" for k_, v in devs.items()))
        assert float((g0 - g1).abs().max()) <= tol, (name, devs)
        assert devs["tile"] <= limit and devs["local"] <= limit, (name, devs)
        if gn[3]:
            assert bool((g1[:, Cout:] == 7.0).all()), "the other half of the concat operand is someone else's"
