"""The in-kernel Philox noise on the MI355X against the counter-exact host reference (oracle/philox_ref.py, pinned on the
CPU by tests/test_noise_exact_cpu.py): every launch that draws - lfvdm_update_rng_x0, lfvdm_conv_out_update_x0,
lfvdm_known_blend, lfvdm_renoise, lfvdm_search_noise_fill, lfvdm_search_noise_qsample - and the samplers' key handling,
element by element, under seeds whose high word is set.  GPU only.

What fails under which fault (each on essentially every element):
  a dropped high key word      every seed-parametrised case (1 << 32 draws seed 0's noise) and test_both_key_words_count
                               of each launch; the repeat keys in test_known_region_chain_repeat_keys (the stride's high word)
  wrong constants or rounds    every case of every launch (the reference itself is pinned by the known-answer vectors)
  counter words misplaced      rows with t != row index (test_update_rng, test_conv_out_update, test_known_blend,
                               test_renoise), test_streams_at_one_key (the stream word), test_search_noise_fill_and_qsample
                               (j above the video, the step above the stream id, frame 299)
  geometry-dependent quads     test_update_rng_long_rows, test_known_blend_second_pass, test_renoise_second_pass (the head and
                               the search launches have no capped grid: one quad per wave, one workgroup per slot)
  an off-by-one head quad      test_conv_out_update, both shapes (Cout = 3 and 4, W = 4 and 12)

Tolerance.  The integer part is exact; what separates a kernel from the reference is the device's logf, sqrtf, sincosf and
one fp32 product.  The deviation is counted in units of 2^-23 * max(1, m), m the reference radius of the element's
Box-Muller pair.  Unrelated draws differ by O(1), about 10^6 units, so a wrong counter word, key word, round or constant
fails on essentially every element.

Measured on the MI355X (largest deviation over all cases of this module, printed by every run): 1.776 units, in the
second-pass blend case of 1048596 elements (re-noise 1.759 and update 1.680 at that size; at most 1.41 in the small cases,
the samplers' included).  The assertion stands at four times that value, 7.104 units (libm differences between ROCm
releases), and never above 16."""
import numpy as np
import pytest
import torch

from oracle import philox_ref as pr
from test_oracle_golden import load_case
from test_forward_gpu import build_native
from test_ops_gpu import cl, packed, rnd
from test_sampler_gpu import make_diffusion

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -23
MEASURED_UNITS = 1.776      # module docstring
TOL_UNITS = min(4.0 * MEASURED_UNITS, 16.0)
assert TOL_UNITS <= 16.0

SEEDS = [0, 1 << 32, 0x0123456789ABCDEF, 2 ** 63 - 1, -1]
S = 0x0123456789ABCDEF      # the seed of the single-seed cases: both words set, and different
SECOND_PASS_INNER = 4 * (1024 * 256 + 5)      # quads past 1024 workgroups x 256 threads: the second grid-stride pass
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if WORST:
        name = max(WORST, key=WORST.get)
        print(f"\n[noise exact] largest deviation over all cases: {WORST[name]:.3f} units of 2^-23 max(1, m) ({name}); "
              f"asserted at {TOL_UNITS:g}")


@pytest.fixture(scope="module")
def nat():
    from improved_diffusion import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def diff():
    return make_diffusion(1000, "")


def i64(seed):
    """Any Python int -> the int64 with the bits of seed modulo 2^64 (what a device seed tensor holds)."""
    return ((int(seed) + 2 ** 63) % 2 ** 64) - 2 ** 63


def seed_tensor(seed):
    return torch.tensor([i64(seed)], dtype=torch.int64, device="cuda")


def nan_like(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def check(name, got, ref):
    """Every element of ``got`` (a device tensor) within TOL_UNITS of the reference (z, m); -> the float32 array."""
    z, m = ref
    g = got.detach().cpu().numpy()
    assert g.dtype == np.float32 and g.size == z.size, (name, g.shape, z.shape)
    g = g.reshape(z.shape)
    assert np.all(np.isfinite(g)), f"{name}: {int((~np.isfinite(g)).sum())} elements not written or not finite"
    dev = np.abs(g.astype(np.float64) - z) / (UNIT * np.maximum(1.0, m))
    worst = float(dev.max())
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print(f"[noise exact] {name}: max deviation {worst:.3f} units over {g.size} elements")
    assert worst <= TOL_UNITS, (name, worst, int((dev > TOL_UNITS).sum()), g.size)
    return g


# ------------------------------------------------------------------------------------------------ the launches
def draw_update(nat, diff, seed, t, inner, rule=("ancestral",)):
    """lfvdm_update_rng_x0 on (B, inner) rows -> noise_out"""
    B = len(t)
    recip, recipm1, c1, c2, sg, R, M = diff._update_args(torch.device("cuda"), rule)
    assert sg is not None
    g = torch.Generator().manual_seed(1)
    x, eps = torch.randn(B, inner, generator=g).cuda(), torch.randn(B, inner, generator=g).cuda()
    nz, out = nan_like(B, inner), nan_like(B, inner)
    nat.update_rng_x0(x, eps, nz, torch.tensor(t, dtype=torch.int64, device="cuda"), recip, recipm1, c1, c2, sg, R, M, True, out,
                      seed_tensor(seed))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    return nz


def draw_head(nat, diff, seed, t, dims):
    """lfvdm_conv_out_update_x0 -> noise_out (B, T, Cout, H, W)"""
    B, T, H, W, C, Cout = dims
    assert nat.lib().lfvdm_conv_out_psample_ok(B * T, H, W, C, Cout) == 0
    a = rnd("nx/a", B * T, C, H, W)
    w, bias = rnd("nx/w", Cout, C, 3, 3, scale=0.05), rnd("nx/b", Cout)
    x = rnd("nx/x", B, T, Cout, H, W).cuda()
    recip, recipm1, c1, c2, sg, R, M = diff._update_args(torch.device("cuda"))
    nz, out = nan_like(*x.shape), nan_like(*x.shape)
    nat.conv_out_update_x0(cl(a), packed(nat, w), bias.cuda(), None, x, None, nz, torch.tensor(t, dtype=torch.int64, device="cuda"),
                           recip, recipm1, c1, c2, sg, R, M, True, out, seed_tensor(seed))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    return nz


def fractional_mask(B, T, H, W, seed=3):
    """values strictly inside (0, 1) with some exact 0 and 1 among them"""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(B, T, H, W, generator=g) * 0.98 + 0.01
    pick = torch.randint(0, 4, (B, T, H, W), generator=g)
    return torch.where(pick == 0, torch.zeros(()), torch.where(pick == 1, torch.ones(()), m)).cuda()


def draw_blend(nat, diff, seed, t, shape, mask=None):
    """lfvdm_known_blend with fresh noise -> noise_out"""
    B, T, C, H, W = shape
    tb = diff.known_region_tables("cuda")
    g = torch.Generator().manual_seed(2)
    x, known = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    mask = fractional_mask(B, T, H, W) if mask is None else mask
    nz = nan_like(*shape)
    nat.known_blend(x, known, mask, torch.tensor(t, dtype=torch.int64, device="cuda"), tb["a"], tb["s"], seed=seed_tensor(seed),
                    noise_out=nz)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all())
    return nz


def draw_renoise(nat, diff, seed, t, inner):
    B = len(t)
    tb = diff.known_region_tables("cuda")
    x = torch.randn(B, inner, generator=torch.Generator().manual_seed(4)).cuda()
    nz = nan_like(B, inner)
    nat.renoise(x, torch.tensor(t, dtype=torch.int64, device="cuda"), tb["sqrt_1mbeta"], tb["sqrt_beta"], seed_tensor(seed),
                noise_out=nz)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all())
    return nz


# the search: V = 2 videos, W = 4 windows of K = 3 slots, frames of (4, 4, 4).  A padding slot, frame 299, and the same
# (video, frame) in two different slots of two windows: (video 0, frame 5) in [0, 0] and [2, 1], (video 1, frame 5) in
# [1, 0] and [3, 2], (video 0, frame 1) in [0, 1] and [2, 2], (video 1, frame 2) in [1, 2] and [3, 0]
SEARCH_V, SEARCH_CHW = 2, (4, 4, 4)
SEARCH_TABLE = np.array([[5, 1, -1], [5, 299, 2], [0, 5, 1], [2, 0, 5]], dtype=np.int32)
SEARCH_T_LIST = [999, 400, 0]


def draw_fill(nat, seed, step, j):
    table = torch.from_numpy(SEARCH_TABLE).cuda()
    noise = nan_like(*SEARCH_TABLE.shape, *SEARCH_CHW)
    nat.search_noise_fill(table, seed, step, j, noise, SEARCH_V)
    torch.cuda.synchronize()
    return noise


def draw_qsample(nat, diff, seed, step, j):
    """lfvdm_search_noise_qsample with ctl = (position, ticket, list length, unused) and key = (seed, window step)"""
    tb = diff.tables(torch.device("cuda"))
    sa, sb = tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"]
    table = torch.from_numpy(SEARCH_TABLE).cuda()
    Wn = SEARCH_TABLE.shape[0]
    x_start = torch.randn(*SEARCH_TABLE.shape, *SEARCH_CHW, generator=torch.Generator().manual_seed(5)).cuda()
    noise, x_t = nan_like(*x_start.shape), nan_like(*x_start.shape)
    t_buf = torch.full((Wn,), -5, dtype=torch.int64, device="cuda")
    ctl = torch.tensor([j, 0, len(SEARCH_T_LIST), 0], dtype=torch.int32, device="cuda")
    key = torch.tensor([i64(seed), step], dtype=torch.int64, device="cuda")
    nat.search_noise_qsample(x_start, table, torch.tensor(SEARCH_T_LIST, dtype=torch.int64, device="cuda"), ctl, key, sa, sb,
                             noise, x_t, t_buf, SEARCH_V)
    torch.cuda.synchronize()
    assert ctl.tolist() == [j + 1, 0, len(SEARCH_T_LIST), 0] and t_buf.tolist() == [SEARCH_T_LIST[j] + 1] * Wn
    return noise


def search_ref(seed, step, j):
    z, m = pr.search_noise(seed, step, j, SEARCH_TABLE, SEARCH_V, int(np.prod(SEARCH_CHW)))
    return z.reshape(SEARCH_TABLE.shape + SEARCH_CHW), m.reshape(SEARCH_TABLE.shape + SEARCH_CHW)


def check_search(name, noise, seed, step, j):
    g = check(name, noise, search_ref(seed, step, j))
    pad = SEARCH_TABLE < 0
    assert pad.any() and np.array_equal(g[pad].view(np.uint32), np.zeros(g[pad].shape, dtype=np.uint32)), "padding: +0 bitwise"
    assert np.array_equal(g[0, 0], g[2, 1]) and np.array_equal(g[1, 0], g[3, 2]), "one (video, frame), two slots and windows"


HEAD_DIMS = [(2, 2, 4, 4, 256, 4), (1, 3, 8, 12, 128, 3)]      # (B, T, H, W, C, Cout)
BLEND_SHAPES = [(2, 3, 4, 4, 4), (2, 3, 4, 3, 3)]               # H*W % 4 == 0: the vector-mask instance; != 0: the scalar one
UPDATE_T, HEAD_T, ROW_T = [999, 1, 0], [700, 0], [500, 3]


def one_draw(nat, diff, launch, seed):
    """One small case of ``launch`` under ``seed`` -> (noise tensor, reference)"""
    if launch == "update":
        return draw_update(nat, diff, seed, UPDATE_T, 1027), pr.row_stream_noise(seed, pr.STREAM_UPDATE, UPDATE_T, 1027)
    if launch == "head":
        B, T, H, W, _, Cout = HEAD_DIMS[0]
        return draw_head(nat, diff, seed, HEAD_T, HEAD_DIMS[0]), pr.row_stream_noise(seed, pr.STREAM_UPDATE, HEAD_T, T * Cout * H * W)
    if launch == "blend":
        return (draw_blend(nat, diff, seed, ROW_T, BLEND_SHAPES[0]),
                pr.row_stream_noise(seed, pr.STREAM_BLEND, ROW_T, int(np.prod(BLEND_SHAPES[0][1:]))))
    if launch == "renoise":
        return draw_renoise(nat, diff, seed, ROW_T, 1028), pr.row_stream_noise(seed, pr.STREAM_RENOISE, ROW_T, 1028)
    if launch == "fill":
        return draw_fill(nat, seed, 1, 1), search_ref(seed, 1, 1)
    assert launch == "qsample"
    return draw_qsample(nat, diff, seed, 1, 1), search_ref(seed, 1, 1)


LAUNCHES = ["update", "head", "blend", "renoise", "fill", "qsample"]


# ------------------------------------------------------------------------------------------------ the update launches
@pytest.mark.parametrize("seed", SEEDS)
def test_update_rng(nat, diff, seed):
    """B = 3 rows of 1027 elements: two workgroups and a three-element tail; t = 999, 1 and 0 (the t = 0 row still reports
    its draw).  The stochastic DDIM rule reports the same noise as the ancestral rule."""
    ref = pr.row_stream_noise(seed, pr.STREAM_UPDATE, UPDATE_T, 1027)
    anc = draw_update(nat, diff, seed, UPDATE_T, 1027)
    check(f"update_rng_x0 ancestral seed {seed:#x}", anc, ref)
    ddim = draw_update(nat, diff, seed, UPDATE_T, 1027, rule=("ddim", 1.0))
    check(f"update_rng_x0 ddim seed {seed:#x}", ddim, ref)
    assert torch.equal(anc, ddim)


# launch_update_rng caps the grid at 1024 workgroups of 256 threads, one quad per thread: 262144 quads per pass.
# inner = 262147 is 65537 quads, 257 workgroups: that case does NOT reach a second pass (it crosses 2^16 quads and ends in
# a three-element tail).  The second size, the blend's, is 262149 quads and does.
@pytest.mark.parametrize("inner", [262147, SECOND_PASS_INNER + 3])
def test_update_rng_long_rows(nat, diff, inner):
    t = [431]
    check(f"update_rng_x0 inner {inner}", draw_update(nat, diff, S, t, inner), pr.row_stream_noise(S, pr.STREAM_UPDATE, t, inner))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("dims", HEAD_DIMS)
def test_conv_out_update(nat, diff, dims, seed):
    """The fused head's noise is the row stream of the (T, Cout, H, W) frame stack: element i = ((tt * Cout + co) * H + y)
    * W + x, quad i >> 2, value i & 3."""
    B, T, H, W, _, Cout = dims
    t = HEAD_T[:B]
    z, m = pr.row_stream_noise(seed, pr.STREAM_UPDATE, t, T * Cout * H * W)
    shape = (B, T, Cout, H, W)
    check(f"conv_out_update_x0 {dims} seed {seed:#x}", draw_head(nat, diff, seed, t, dims), (z.reshape(shape), m.reshape(shape)))


# ------------------------------------------------------------------------------------------------ blend and re-noise
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shape", BLEND_SHAPES)
def test_known_blend(nat, diff, shape, seed):
    B, T, C, H, W = shape
    z, m = pr.row_stream_noise(seed, pr.STREAM_BLEND, ROW_T, T * C * H * W)
    got = draw_blend(nat, diff, seed, ROW_T, shape)
    check(f"known_blend {shape} seed {seed:#x}", got, (z.reshape(shape), m.reshape(shape)))
    for other in (fractional_mask(B, T, H, W, seed=9), torch.zeros(B, T, H, W, device="cuda"), torch.ones(B, T, H, W, device="cuda")):
        assert torch.equal(draw_blend(nat, diff, seed, ROW_T, shape, mask=other), got), "the reported noise does not depend on the mask"


def test_known_blend_second_pass(nat, diff):
    """B = 1, 262149 quads: five quads past the capped grid of 1024 x 256, in both mask instances (one reference)."""
    t = [250]
    ref = pr.row_stream_noise(S, pr.STREAM_BLEND, t, SECOND_PASS_INNER)
    assert SECOND_PASS_INNER == 3 * 4 * 87383
    for shape in [(1, 3, 4, 1, 87383), (1, 3, 1, 4, 87383)]:      # H*W = 87383: scalar mask; 4 * 87383: vector mask
        check(f"known_blend second pass {shape}", draw_blend(nat, diff, S, t, shape), ref)


@pytest.mark.parametrize("seed", SEEDS)
def test_renoise(nat, diff, seed):
    check(f"renoise seed {seed:#x}", draw_renoise(nat, diff, seed, ROW_T, 1028), pr.row_stream_noise(seed, pr.STREAM_RENOISE, ROW_T, 1028))


def test_renoise_second_pass(nat, diff):
    t = [250]
    check("renoise second pass", draw_renoise(nat, diff, S, t, SECOND_PASS_INNER),
          pr.row_stream_noise(S, pr.STREAM_RENOISE, t, SECOND_PASS_INNER))


def test_streams_at_one_key(nat, diff):
    """Update, blend and re-noise at one (seed, t, shape): the reference with stream word 0, 1 and 2."""
    shape = BLEND_SHAPES[0]
    inner = int(np.prod(shape[1:]))
    up = check("streams: update", draw_update(nat, diff, S, ROW_T, inner), pr.row_stream_noise(S, pr.STREAM_UPDATE, ROW_T, inner))
    bl = check("streams: blend", draw_blend(nat, diff, S, ROW_T, shape).view(shape[0], inner), pr.row_stream_noise(S, pr.STREAM_BLEND, ROW_T, inner))
    rn = check("streams: renoise", draw_renoise(nat, diff, S, ROW_T, inner), pr.row_stream_noise(S, pr.STREAM_RENOISE, ROW_T, inner))
    assert not np.any(up == bl) and not np.any(up == rn) and not np.any(bl == rn)


# ------------------------------------------------------------------------------------------------ the key
@pytest.mark.parametrize("launch", LAUNCHES)
def test_both_key_words_count(nat, diff, launch):
    """Seed s against s + 2^32 (only the high word differs) and against s with its halves swapped: different tensors, each
    the reference's."""
    swapped = ((S & 0xFFFFFFFF) << 32) | (S >> 32)
    base = check(f"{launch} seed s", *one_draw(nat, diff, launch, S))
    for name, seed in (("s + 2^32", S + 2 ** 32), ("halves swapped", swapped)):
        other = check(f"{launch} seed {name}", *one_draw(nat, diff, launch, seed))
        assert not np.array_equal(other, base), name
        live = base != 0                                              # (the search's padding slots are zero under every seed)
        assert np.mean(other[live] == base[live]) < 1e-3, name


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("launch", ["fill", "qsample"])
def test_search_noise_seeds(nat, diff, launch, seed):
    noise = draw_fill(nat, seed, 1, 1) if launch == "fill" else draw_qsample(nat, diff, seed, 1, 1)
    check_search(f"search {launch} seed {seed:#x}", noise, seed, 1, 1)


# ------------------------------------------------------------------------------------------------ the search
def test_search_noise_fill_and_qsample(nat, diff):
    """Positions, window steps up to the last the counter word holds, a seed >= 2^63 given to the fill as it is and to the
    head launch as the negative int64 of the same bits in key[0]: both report the reference's tensor, hence each other's."""
    seed = 2 ** 63 + 0x0123456789ABCDEF
    assert seed >= 2 ** 63 and i64(seed) < 0
    fills, heads = {}, {}
    for step in (0, 1, 2 ** 24 - 1):
        for j in (0, 1, 65534):
            fills[step, j] = draw_fill(nat, seed, step, j)
            check_search(f"search fill step {step} j {j}", fills[step, j], seed, step, j)
        for j in (0, 1, 2):
            heads[step, j] = draw_qsample(nat, diff, seed, step, j)
            check_search(f"search qsample step {step} j {j}", heads[step, j], seed, step, j)
        for j in (0, 1):
            assert torch.equal(fills[step, j], heads[step, j]), (step, j)
    live = torch.from_numpy(SEARCH_TABLE >= 0).cuda()
    keys = list(fills)
    for a in range(len(keys)):
        for b in range(a + 1, len(keys)):
            assert not bool((fills[keys[a]][live] == fills[keys[b]][live]).any()), (keys[a], keys[b])


# ------------------------------------------------------------------------------------------------ the samplers
@pytest.fixture(scope="module")
def micro():
    cfg, sd, inp = load_case("micro")
    model = build_native(cfg, sd).eval()
    d = {k: v.cuda() for k, v in inp.items()}
    mk = dict(frame_indices=d["frame_indices"], obs_mask=d["obs_mask"], latent_mask=d["latent_mask"], x0=d["x0"])
    return model, d, mk, tuple(inp["x"].shape)


def test_graph_sampler_chain(micro):
    """Two replayed steps: after each, the sampler's noise is the update stream under its own seed at the t it consumed."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    model, d, mk, shape = micro
    diff = make_diffusion(1000, "10")
    inner = int(np.prod(shape[1:]))
    torch.manual_seed(21)
    s = GraphSampler(diff, model, shape, True)
    s.begin(d["x"].clone(), mk)
    nt = diff.num_timesteps
    for i in (nt - 1, nt - 2):
        s.step(i)
        torch.cuda.synchronize()
        assert s.t_buf.tolist() == [i] * shape[0]
        seed = int(s.seed)
        check(f"GraphSampler step t = {i} (head fused: {bool(s.plan.head_fused)})", s.noise.view(shape[0], inner),
              pr.row_stream_noise(seed, pr.STREAM_UPDATE, [i] * shape[0], inner))
    assert seed >> 32, "the chain's key comes from random_(): 63 bits"


def test_known_region_chain_repeat_keys(micro, monkeypatch):
    """A known-region chain with two resample repeats through the public loop, on a sampler that records its noise: the
    update and blend noise of repeat r are the reference's under the key seed0 + _repeat_seed_offset(r) modulo 2^64."""
    from improved_diffusion.gaussian_diffusion import GraphSampler
    model, d, mk, shape = micro
    B, T, _, H, W = shape
    diff = make_diffusion(1000, "3")
    inner = int(np.prod(shape[1:]))
    s = GraphSampler(diff, model, shape, True)
    s.enable_known_region(False, record_noise=True)
    monkeypatch.setattr(diff, "_known_region_sampler", lambda *a, **k: s)
    records, renoised = [], []
    step, renoise = s.step, s.renoise

    def recording_step(i):
        out = step(i)
        torch.cuda.synchronize()
        records.append((i, int(s.seed), s.noise.clone(), s.known_noise.clone()))
        return out
    monkeypatch.setattr(s, "step", recording_step)
    monkeypatch.setattr(s, "renoise", lambda: (renoised.append(len(records)), renoise())[1])
    g = torch.Generator().manual_seed(17)
    known = torch.randn(shape, generator=g).cuda()
    torch.manual_seed(22)
    out = diff.known_region_sample_loop(model, shape, known, fractional_mask(B, T, H, W), resample_steps=2, model_kwargs=mk,
                                        latent_mask=d["latent_mask"], return_decoded=False)
    assert bool(torch.isfinite(out).all())
    assert [rec[0] for rec in records] == [2, 2, 1, 1, 0], "two repeats of every timestep above 0"
    assert renoised == [1, 3], "one re-noise between the two repeats of a timestep above 0"
    seed0 = records[0][1] % 2 ** 64
    assert seed0 >> 32
    for (i, seed, up, bl), r in zip(records, [0, 1, 0, 1, 0]):
        key = (seed0 + diff._repeat_seed_offset(r)) % 2 ** 64
        assert seed % 2 ** 64 == key, (i, r)
        check(f"known-region chain t = {i} repeat {r}: update", up.view(B, inner), pr.row_stream_noise(key, pr.STREAM_UPDATE, [i] * B, inner))
        check(f"known-region chain t = {i} repeat {r}: blend", bl.view(B, inner), pr.row_stream_noise(key, pr.STREAM_BLEND, [i] * B, inner))
    assert diff._repeat_seed_offset(1) % 2 ** 64 == 0x1E3779B97F4A7C15 and diff._repeat_seed_offset(0) == 0
