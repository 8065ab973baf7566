"""The yardstick of test_train_glue_gpu: case lists, host restatements and mutated restatements of the kernels that move and
fold data around a training step - lfvdm_prepare_batch, lfvdm_det_reduce, lfvdm_pack_conv_weights and
lfvdm_unpack_conv_grads - checked here without a GPU.

None of these kernels rounds more than once per element: each is a copy, a permutation or a fixed-order chain of fp32
additions, so the GPU file compares bits.  A bitwise comparison only proves something if the inputs can tell a wrong kernel
from a right one, and that is what this file establishes: for every case it builds the restatement and a set of MUTATED
restatements (one plausible kernel bug each) and asserts that every mutation that applies to the case changes at least one
output word.  A mutation "applies" where the bug it models changes the arithmetic at all:

- batch gather: the omitted clamp needs Tp > 1 (with one pool row every index is row 0), the truncated copy needs
  frame_elems % 1024 != 0; the others always apply.  A case is a shape with BOTH its tables (ordinary, adversarial).
- reduce: another order needs parts >= 2 (reversed) and a pairwise tree that is not the chain needs parts >= 2 as well;
  (8, 1, 0, 0) has a single order.  The first-trip-only mutation needs an element past the capped grid: the two large cases.
- pack: un-flipped taps need the transposed layout with 9 taps; an ignored ld needs ld > natural; swapped tile origins
  need a tile grid that is not square ((b / tci, b % tci) swapped on a square grid is the same set of tiles in another
  order); the leaking filter clamp needs Cout % 32 != 0.
- unpack: an ignored ldp / un-zeroed padding need ldp > Cin; swapped (t, ci) needs taps > 1 and Cin > 1; the job boundary
  needs a job in front.

Tables of the batch gather: the ordinary table of a shape reads pool row (7 s + 3) % Tp in slot s = b F + f, which reaches
min(Tp, B F) different row indices - every one where the shape has the slots for it ((1, 2, 3, 8196) has two slots for
three rows) - and leaves a pool row unused wherever the pool has more than one row ((1, 1, 1, 4) has one).  The adversarial
table spends its first five slots on -1, Tp, -2^31, 2^31 - 1 and Tp + 7, which clamp onto the two end rows, so it may
reach up to five row indices fewer."""
import numpy as np
import pytest
import torch

from test_ops_gpu import rnd

NAN = float("nan")
SENT = -724531.25               # exactly representable; no kernel under test produces it
GUARD = 64                      # floats of guard band


def bits(t):
    """The raw words of a float32 tensor / array (NaN-safe equality)."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------
# 1. batch gather
# ------------------------------------------------------------------------------------------------------------------------
GATHER_CASES = [(1, 1, 1, 4), (2, 3, 5, 180), (3, 7, 9, 1028), (2, 20, 40, 3 * 10 * 12), (1, 2, 3, 4 * 2049), (5, 1, 2, 1024)]
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
ADV_FLAGS = [0, 1, 2, -1, I32_MAX, I32_MIN]
ADV_INDEX = [I32_MAX, I32_MIN, -1, 0]


def adv_rows(Tp):
    return [-1, Tp, I32_MIN, I32_MAX, Tp + 7]


def gather_pool(B, F, Tp, fe):
    """Every element distinct: a frame from the wrong row, or shifted by one float4, cannot compare equal."""
    assert B * Tp * fe < 2 ** 24
    return (torch.arange(B * Tp * fe, dtype=torch.float32) + 1.0).view(B, Tp, fe)


def gather_tables(B, F, Tp, fe):
    """-> {"ordinary", "adversarial"}: int32 (B, F, 4) tables of (pool row, frame index, observed, latent)."""
    S = B * F
    s = np.arange(S)
    u = rnd(f"tg/gather/{B}/{F}/{Tp}/{fe}", S, 3).numpy()
    rows = (7 * s + 3) % Tp
    ordinary = np.stack([rows, 1 + np.floor(np.abs(u[:, 0]) * 400).astype(np.int64), (u[:, 1] > 0), (u[:, 2] > 0.3)], 1)
    adv = ordinary.copy()
    ar = adv_rows(Tp)
    adv[:min(S, len(ar)), 0] = ar[:S]
    adv[:, 1] = [ADV_INDEX[i % 4] for i in s]
    adv[:, 2] = [ADV_FLAGS[(i + 2) % 6] for i in s]
    adv[:, 3] = [ADV_FLAGS[(5 * i) % 6] for i in s]
    return {k: torch.from_numpy(v.astype(np.int64)).to(torch.int32).view(B, F, 4) for k, v in (("ordinary", ordinary), ("adversarial", adv))}


def gather_ref(pool, table, mutation=None):
    """-> (batch, frame_indices int64, obs, latent).  Elements a mutated kernel never writes keep the NaN pre-fill."""
    B, Tp, fe = pool.shape
    t = table.long()
    row = t[..., 0] % Tp if mutation == "no_clamp" else t[..., 0].clamp(0, Tp - 1)
    batch = pool[torch.arange(B)[:, None], row].clone()
    if mutation == "whole_passes":
        batch[..., (fe // 1024) * 1024:] = NAN
    fi = t[..., 0 if mutation == "index_col0" else 1].clone()
    flag = (lambda c: t[..., c].float()) if mutation == "flag_value" else (lambda c: (t[..., c] != 0).float())
    obs, lat = flag(2), flag(3)
    if mutation == "flags_swapped":
        obs, lat = lat, obs
    return batch, fi, obs, lat


GATHER_MUTATIONS = ["no_clamp", "flag_value", "index_col0", "flags_swapped", "whole_passes"]


def gather_applies(mutation, B, F, Tp, fe):
    return {"no_clamp": Tp > 1, "whole_passes": fe % 1024 != 0}.get(mutation, True)


def _gather_differs(a, b):
    return any(not same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("B,F,Tp,fe", GATHER_CASES)
def test_gather_tables_cover_the_pool_and_the_edges(B, F, Tp, fe):
    tabs = gather_tables(B, F, Tp, fe)
    S = B * F
    for name, tab in tabs.items():
        t = tab.long()
        hit = t[..., 0].clamp(0, Tp - 1)
        used = {(b, int(r)) for b in range(B) for r in hit[b]}
        lost = 0 if name == "ordinary" else 5       # the five edge slots clamp onto the two end rows
        assert len({r for _, r in used}) >= max(1, min(Tp, S) - lost), name
        if name == "ordinary":
            assert len({r for _, r in used}) == min(Tp, S)
        assert len(used) < B * Tp or B * Tp == 1, "a pool row must stay unused"
    adv = tabs["adversarial"].long().view(S, 4)
    assert adv[:, 0].tolist()[:5] == adv_rows(Tp)[:S]
    if S >= 6:
        assert set(adv[:, 2].tolist()) == set(ADV_FLAGS) and set(adv[:, 3].tolist()) == set(ADV_FLAGS)
    if S >= 4:
        assert set(adv[:, 1].tolist()) == set(ADV_INDEX)
    assert set(tabs["ordinary"][..., 2:].unique().tolist()) <= {0, 1}
    # the int32 -> int64 widening: the reference keeps the sign
    assert gather_ref(gather_pool(B, F, Tp, fe), tabs["adversarial"])[1].view(-1)[0] == I32_MAX


@pytest.mark.parametrize("B,F,Tp,fe", GATHER_CASES)
def test_gather_cases_tell_a_wrong_kernel_from_a_right_one(B, F, Tp, fe):
    pool = gather_pool(B, F, Tp, fe)
    tabs = gather_tables(B, F, Tp, fe)
    assert pool.unique().numel() == pool.numel()
    for m in GATHER_MUTATIONS:
        if gather_applies(m, B, F, Tp, fe):
            assert any(_gather_differs(gather_ref(pool, t), gather_ref(pool, t, m)) for t in tabs.values()), m


def test_every_gather_mutation_applies_somewhere():
    for m in GATHER_MUTATIONS:
        assert sum(gather_applies(m, *c) for c in GATHER_CASES) >= 4, m


# ------------------------------------------------------------------------------------------------------------------------
# 2. ordered slab reduction
# ------------------------------------------------------------------------------------------------------------------------
GRID_CAP = 4096 * 256           # threads of the capped grid: one float4 (aligned body) or one float (scalar body) each
REDUCE_SMALL = ([(8, parts, 0, 0) for parts in range(1, 10)]
                + [(1024, 4, 0, 0), (1024, 6, 0, 0), (1024, 5, 1, 0), (1024, 5, 0, 1), (1024, 5, 1, 1), (1023, 5, 0, 0)])
REDUCE_LARGE = [(4 * (GRID_CAP + 100), 3, 0, 0), (GRID_CAP + 101, 3, 0, 0)]
ROW_SCALE = [1e-4, 1e3, 1.0]    # of slab row p: ROW_SCALE[p % 3] - a sum in another order differs in the low bits


def reduce_is_aligned(n, parts, off_dst, off_slab):
    """Which kernel the launcher picks when the base allocations are 16-byte aligned."""
    return n % 4 == 0 and off_dst % 4 == 0 and off_slab % 4 == 0


def reduce_inputs(n, parts, off_dst=0, off_slab=0):
    tag = f"tg/reduce/{n}/{parts}"
    scale = torch.tensor([ROW_SCALE[p % 3] for p in range(parts)])[:, None]
    return rnd(tag + "/dst", n), rnd(tag + "/slab", parts, n) * scale


def reduce_ref(dst0, slab, mutation=None, first_trip=None):
    parts = slab.shape[0]
    want = dst0.clone()
    if mutation == "pairwise":
        level = [slab[p] for p in range(parts)]
        while len(level) > 1:
            level = [level[i] + level[i + 1] if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
        return want + level[0]
    order = range(parts - 1, -1, -1) if mutation == "reversed" else range(parts - 1 if mutation == "last_dropped" else parts)
    for p in order:
        want += slab[p]
    if mutation == "first_trip":
        want[first_trip:] = dst0[first_trip:]
    return want


@pytest.mark.parametrize("n,parts,od,os_", REDUCE_SMALL)
def test_reduce_cases_tell_another_order_from_the_sequential_one(n, parts, od, os_):
    dst0, slab = reduce_inputs(n, parts)
    want = reduce_ref(dst0, slab)
    assert not same_bits(want, reduce_ref(dst0, slab, "last_dropped"))
    if parts >= 2:
        assert not same_bits(want, reduce_ref(dst0, slab, "reversed")), "reversed order"
        assert not same_bits(want, reduce_ref(dst0, slab, "pairwise")), "pairwise tree"
    else:
        assert same_bits(want, reduce_ref(dst0, slab, "reversed")) and same_bits(want, reduce_ref(dst0, slab, "pairwise"))


def test_reduce_cases_reach_every_path():
    assert {p % 4 for _, p, _, _ in REDUCE_SMALL if p >= 4} == {0, 1, 2, 3} and {p for _, p, _, _ in REDUCE_SMALL} >= {1, 2, 3}
    scalar = [c for c in REDUCE_SMALL if not reduce_is_aligned(*c)]
    assert {(c[0] % 4 == 0, c[2], c[3]) for c in scalar} == {(True, 1, 0), (True, 0, 1), (True, 1, 1), (False, 0, 0)}
    (n4, _, _, _), (n1, _, _, _) = REDUCE_LARGE
    assert reduce_is_aligned(*REDUCE_LARGE[0]) and not reduce_is_aligned(*REDUCE_LARGE[1])
    # the grid is capped at 4096 workgroups: 100 float4 threads / 101 scalar threads take a second trip
    assert (n4 // 4 + 255) // 256 > 4096 and n4 // 4 - GRID_CAP == 100
    assert (n1 + 255) // 256 > 4096 and n1 - GRID_CAP == 101
    assert reduce_first_trip(*REDUCE_LARGE[0]) == 4 * GRID_CAP and reduce_first_trip(*REDUCE_LARGE[1]) == GRID_CAP


def reduce_first_trip(n, parts, od, os_):
    """Elements the first trip of the grid-stride loop covers (the GPU file asserts that every later element moved)."""
    return GRID_CAP * (4 if reduce_is_aligned(n, parts, od, os_) else 1)


def test_first_trip_mutation_is_visible_on_a_scaled_down_model():
    """The same mutation at a cap of 8 threads: elements past the first trip keep dst0 and differ."""
    dst0, slab = reduce_inputs(4 * 8 + 12, 3)
    assert not same_bits(reduce_ref(dst0, slab), reduce_ref(dst0, slab, "first_trip", 32))


# ------------------------------------------------------------------------------------------------------------------------
# 4. grouped pack / unpack
# ------------------------------------------------------------------------------------------------------------------------
# (Cout, Cin, k, transposed, ld); the first job has one tile
PACK_JOBS = ([(1, 1, 3, 0, 0), (1, 1, 3, 1, 0)]
             + [(co, ci, k, tr, 0) for co, ci, k in ((33, 31, 3), (65, 5, 1), (4, 40, 3)) for tr in (0, 1)]
             + [(33, 5, 3, 0, 32), (7, 40, 1, 0, 64), (4, 64, 3, 1, 32), (3, 33, 3, 1, 4)]
             + [(512, 384, 3, 0, 0), (512, 384, 3, 1, 0)])
PACK_SINGLE = (33, 31, 3, 1, 0)
PACK_MUTATIONS = ["no_flip", "ld_ignored", "origins_swapped", "clamp_leaks"]


def pack_tiles(Cout, Cin):
    return ((Cout + 31) // 32) * ((Cin + 31) // 32)


def pack_weight(job):
    Cout, Cin, k, tr, ld = job
    return rnd(f"tg/pack/{Cout}/{Cin}/{k}", Cout, Cin, k, k)


def pack_geometry(job):
    """-> (rows, taps, natural width, row stride) of the destination."""
    Cout, Cin, k, tr, ld = job
    nat = Cout if tr else Cin
    return (Cin if tr else Cout), k * k, nat, (ld or nat)


def pack_prefill(job):
    """Flat destination + guard: NaN where the kernel must write, the sentinel in the padding columns and the guard."""
    rows, taps, nat, ldd = pack_geometry(job)
    buf = torch.full((rows * taps, ldd), SENT)
    buf[:, :nat] = NAN
    return torch.cat([buf.view(-1), torch.full((GUARD,), SENT)])


def pack_expected(job, w):
    """The host permutation placed in the pre-filled destination."""
    Cout, Cin, k, tr, ld = job
    rows, taps, nat, ldd = pack_geometry(job)
    perm = w.flip(2, 3).permute(1, 2, 3, 0) if tr else w.permute(0, 2, 3, 1)
    buf = pack_prefill(job)
    buf[:rows * taps * ldd].view(rows * taps, ldd)[:, :nat] = perm.reshape(rows * taps, nat)
    return buf


def pack_model(job, w, mutation=None):
    """The kernel's tile walk on the host (32 filters x 32 channels x all taps per workgroup), with one bug."""
    Cout, Cin, k, tr, ld = job
    rows, taps, nat, ldd = pack_geometry(job)
    if mutation == "ld_ignored":
        ldd = nat
    buf = pack_prefill(job).numpy()
    wn = w.reshape(Cout, Cin, taps).numpy()
    tci = (Cin + 31) // 32
    for b in range(pack_tiles(Cout, Cin)):
        co0, ci0 = (b // tci) * 32, (b % tci) * 32
        if mutation == "origins_swapped":
            co0, ci0 = ci0, co0
        nco, nci = min(32, Cout - co0), min(32, Cin - ci0)
        if nco <= 0 or nci <= 0:
            continue
        # filters past the ragged edge (clamp_leaks: they carry the last filter's values) first, the real ones over them
        for cs in ((np.arange(nco, 32), np.arange(nco)) if mutation == "clamp_leaks" else (np.arange(nco),)):
            if cs.size == 0:
                continue
            c, ii, t = np.meshgrid(cs, np.arange(nci), np.arange(taps), indexing="ij")
            src_t = (taps - 1 - t) if (tr and mutation != "no_flip") else t
            val = wn[co0 + np.minimum(c, nco - 1), ci0 + ii, src_t]
            idx = (((ci0 + ii) * taps + t) * ldd + co0 + c) if tr else (((co0 + c) * taps + t) * ldd + ci0 + ii)
            ok = idx < buf.size
            buf[idx[ok]] = val[ok]
    return torch.from_numpy(buf)


def pack_applies(mutation, job):
    Cout, Cin, k, tr, ld = job
    return {"no_flip": tr == 1 and k == 3, "ld_ignored": ld > (Cout if tr else Cin),
            "origins_swapped": (Cout + 31) // 32 != (Cin + 31) // 32, "clamp_leaks": Cout % 32 != 0}[mutation]


@pytest.mark.parametrize("job", PACK_JOBS + [PACK_SINGLE], ids=lambda j: "-".join(map(str, j)))
def test_pack_jobs_tell_a_wrong_kernel_from_a_right_one(job):
    w = pack_weight(job)
    want = pack_expected(job, w)
    rows, taps, nat, ldd = pack_geometry(job)
    assert not torch.isnan(want.view(-1)[:rows * taps * ldd].view(-1, ldd)[:, :nat]).any()
    assert same_bits(pack_model(job, w), want), "the tile walk is the permutation"
    for m in PACK_MUTATIONS:
        if pack_applies(m, job):
            assert not same_bits(pack_model(job, w, m), want), m


def test_pack_job_list_reaches_every_edge():
    assert pack_tiles(*PACK_JOBS[0][:2]) == 1 and len(PACK_JOBS) >= 12
    for m in PACK_MUTATIONS:
        assert sum(pack_applies(m, j) for j in PACK_JOBS) >= 3, m
    assert {(j[3], j[1] if not j[3] else j[0], j[4]) for j in PACK_JOBS if j[4]} == {(0, 5, 32), (0, 40, 64), (1, 4, 32), (1, 3, 4)}
    assert pack_tiles(512, 384) == 16 * 12


# (Cout, Cin, taps, ldp)
UNPACK_JOBS = [(64, 32, 9, 0), (7, 5, 9, 32), (33, 100, 1, 0), (3, 40, 1, 64), (2, 1024, 9, 0), (1, 1, 9, 0)]
UNPACK_MAX_ROW = max(t * max(ci, ldp) for _, ci, t, ldp in UNPACK_JOBS)
UNPACK_MUTATIONS = ["ldp_ignored", "t_ci_swapped", "padding_kept", "boundary"]


def unpack_inputs(j, job):
    """-> (g0 [Cout][Cin][taps], gp0 [Cout][taps][ldp or Cin]); the padding columns of gp0 are NOT zero, so that a kernel
    that reads them, or leaves them, shows."""
    Cout, Cin, taps, ldp = job
    return rnd(f"tg/unpack/{j}/g", Cout, Cin, taps), rnd(f"tg/unpack/{j}/gp", Cout, taps, ldp or Cin)


def unpack_ref(j, job, g0, gp0, mutation=None):
    """-> (g, gp afterwards)."""
    Cout, Cin, taps, ldp = job
    real = gp0[:, :, :Cin]
    if mutation == "ldp_ignored":
        real = gp0.reshape(-1)[:Cout * taps * Cin].reshape(Cout, taps, Cin)     # rows of taps * Cin floats
    add = real.reshape(Cout, Cin, taps) if mutation == "t_ci_swapped" else real.permute(0, 2, 1)
    g, gp = g0 + add, torch.zeros_like(gp0)
    if mutation == "padding_kept":
        gp[:, :, Cin:] = gp0[:, :, Cin:]
    if mutation == "boundary" and j > 0:         # the first row of the job is taken for a row of the job in front
        g[0], gp[0] = g0[0], gp0[0]
    return g, gp


def unpack_applies(mutation, j, job):
    Cout, Cin, taps, ldp = job
    return {"ldp_ignored": ldp > Cin, "padding_kept": ldp > Cin, "t_ci_swapped": taps > 1 and Cin > 1, "boundary": j > 0}[mutation]


@pytest.mark.parametrize("j", range(len(UNPACK_JOBS)))
def test_unpack_jobs_tell_a_wrong_kernel_from_a_right_one(j):
    job = UNPACK_JOBS[j]
    g0, gp0 = unpack_inputs(j, job)
    want = unpack_ref(j, job, g0, gp0)
    assert float(want[1].abs().max()) == 0.0 and float(gp0.abs().min()) > 0.0
    for m in UNPACK_MUTATIONS:
        if unpack_applies(m, j, job):
            got = unpack_ref(j, job, g0, gp0, m)
            assert not (same_bits(got[0], want[0]) and same_bits(got[1], want[1])), m


def test_unpack_job_list_reaches_every_edge():
    assert UNPACK_MAX_ROW == 9216 == max(t * max(ci, ldp) for _, ci, t, ldp in UNPACK_JOBS) and len(UNPACK_JOBS) >= 6
    for m in UNPACK_MUTATIONS:
        assert sum(unpack_applies(m, j, job) for j, job in enumerate(UNPACK_JOBS)) >= 2, m
    assert {t for _, _, t, _ in UNPACK_JOBS} == {1, 9}
    assert any(t == 9 and t * ci > 256 for _, ci, t, _ in UNPACK_JOBS), "a row longer than one 256-thread pass"


def test_multiply_shift_is_division_by_nine_for_every_row_index():
    """unpack_conv_grads_kernel: ci = (i * 58255) >> 19 in 32-bit unsigned arithmetic, for rows of at most 16384 floats
    (64 KB of LDS)."""
    i = np.arange(16384, dtype=np.uint64)
    assert int((i * 58255).max()) < 2 ** 32
    assert np.array_equal((i * 58255) >> 19, i // 9)
    assert 16384 * 4 == 64 * 1024 and 16385 * 4 > 64 * 1024
