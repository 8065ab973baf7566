"""Global-norm gradient clipping and the non-finite step skip on the MI355X (csrc/grad_clip.hip): the norm launches against
numpy fp64, the clip coefficient and the clipped fused AdamW/EMA launch against torch in fp64, the skip on an inf / NaN
gradient, every EMA-count instance and both loop shapes of the capped grid of the fused kernel (plain and clipping entry,
``grad_sqsum`` included) against fp64, ``TrainLoop`` with ``max_grad_norm`` (on: against the loop's host-memory arithmetic; off: bitwise the loop
without the keyword and none of the new entries called) and two ranks agreeing bitwise.  GPU only."""
import argparse
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import PKG, ROOT
from test_oracle_golden import load_case
from test_forward_gpu import build_native
from test_dist_gpu import _data, _free_port

pytestmark = pytest.mark.gpu

NEW_ENTRIES = ("lfvdm_grad_norm_partials", "lfvdm_grad_norm_finalize", "lfvdm_adamw_ema_clip")


@pytest.fixture(autouse=True)
def _leave_the_logger_clean():
    """``TrainLoop`` logs running means into the process-wide logger; a loop that is never dumped would leave its losses in
    the means the next test's loop reports (tests/test_train_gpu.py compares them)."""
    yield
    from improved_diffusion.logger import logger
    logger.dumpkvs()


def _stat(g, grad_scale, max_norm, stat=None):
    from improved_diffusion import _native as nat
    stat = torch.zeros(4, device="cuda") if stat is None else stat
    partials = torch.empty(nat.grad_norm_nparts(g.numel()), device="cuda")
    nat.grad_clip_stat(g, grad_scale, max_norm, partials, stat)
    torch.cuda.synchronize()
    return stat


def _ints(stat):
    return stat.view(torch.int32)[2:].tolist()


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset_one_float"])
@pytest.mark.parametrize("n", [1, 3, 1023, 262147])
def test_norm_matches_fp64(n, offset):
    """stat[0] against numpy fp64 on an arena of n floats, on a 16-byte aligned base pointer and on one moved by a float
    (the scalar head).  A thread adds at most ``chain`` products in a row: 16 per grid-stride pass (4 float4 loads of 4)
    and one head / tail element; behind it come 6 shuffle steps, 3 additions across the waves, the double sum (exact at this
    scale), one rounding to fp32, and two roundings per element (scale, square): relative error <= (chain + 16) * 2^-24."""
    from improved_diffusion import _native as nat
    base = torch.randn(n + 1, generator=torch.Generator().manual_seed(n)).cuda()
    g = base[offset:offset + n]
    assert g.data_ptr() % 16 == 4 * offset
    scale = 0.75
    nparts = nat.grad_norm_nparts(n)
    passes = math.ceil((n // 4) / (4 * 256 * nparts))
    chain = 16 * passes + 1
    if n == 262147:
        assert nparts > 1 and passes > 1 and n % 4 != 0, "the case is meant to cover several workgroups, passes and a tail"
    want = float(((g.cpu().numpy().astype(np.float64) * scale) ** 2).sum())
    a, b = _stat(g, scale, 1.0), _stat(g, scale, 1.0)
    got = float(a[0])
    rel = abs(got - want) / want
    print(f"[grad norm] n={n} offset={offset} nparts={nparts} chain={chain} rel.err={rel:.3e} bound={(chain + 16) * 2.0 ** -24:.3e}")
    assert rel <= (chain + 16) * 2.0 ** -24
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two runs must give identical bits"
    assert _ints(a) == [0, 0]


class _Opt:
    """p / g / m / v and n_ema (two unless told) EMA copies of n floats on the device + the launch arguments of one optimizer step."""

    def __init__(self, n, seed=0, n_ema=2):
        gen = torch.Generator().manual_seed(seed)
        self.n = n
        self.p = torch.randn(n, generator=gen).cuda()
        self.g = (torch.randn(n, generator=gen) * 0.1).cuda()
        self.m = torch.zeros(n, device="cuda")
        self.v = torch.zeros(n, device="cuda")
        self.rates = [0.9, 0.999, 0.99, 0.9999][:n_ema]
        self.ema = [self.p.clone() for _ in self.rates]
        self.lr, self.betas, self.eps, self.wd, self.scale = 1e-3, (0.9, 0.999), 1e-8, 0.01, 0.5

    def clone(self):
        o = _Opt.__new__(_Opt)
        o.__dict__.update(self.__dict__)
        o.p, o.g, o.m, o.v = self.p.clone(), self.g.clone(), self.m.clone(), self.v.clone()
        o.ema = [e.clone() for e in self.ema]
        return o

    def state(self):
        return [self.p, self.m, self.v] + self.ema

    def args(self, step):
        from improved_diffusion import _native as nat
        a = nat.AdamWArgs()
        a.p, a.g, a.m, a.v = self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr()
        for i, (e, r) in enumerate(zip(self.ema, self.rates)):
            a.ema[i], a.ema_rate[i] = e.data_ptr(), r
        a.n_ema, a.n = len(self.ema), self.n
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = self.lr, self.betas[0], self.betas[1], self.eps, self.wd
        a.bias_corr1 = 1.0 - self.betas[0] ** step
        a.bias_corr2_sqrt = math.sqrt(1.0 - self.betas[1] ** step)
        a.grad_scale = self.scale
        return a

    def step_plain(self, step):
        from improved_diffusion import _native as nat
        nat.check(nat.lib().lfvdm_adamw_ema(ctypes.byref(self.args(step)), nat.stream()), "lfvdm_adamw_ema")
        torch.cuda.synchronize()

    def step_clip(self, step, max_norm, stat):
        from improved_diffusion import _native as nat
        _stat(self.g, self.scale, max_norm, stat)
        nat.adamw_ema_clip(self.args(step), stat)
        torch.cuda.synchronize()
        return stat


N_OPT = 5003        # five workgroups of the optimizer launch and a three-element tail


def test_coef_one_below_the_threshold_and_clip_entry_equals_plain_entry():
    o = _Opt(N_OPT)
    norm = float((o.g.double() * o.scale).norm())
    a, b = o.clone(), o.clone()
    stat = a.step_clip(1, 10.0 * norm, torch.zeros(4, device="cuda"))
    b.step_plain(1)
    assert float(stat[1]) == 1.0 and _ints(stat) == [0, 0]
    for x, y in zip(a.state(), b.state()):
        assert torch.equal(x, y)
    assert not torch.equal(a.p, o.p)
    # max_norm = 0: no clipping whatever the norm
    stat0 = _stat(o.g * 1e6, o.scale, 0.0)
    assert float(stat0[1]) == 1.0 and _ints(stat0) == [0, 0]


def test_clipped_step_matches_fp64_torch():
    """Norm above max_norm, two steps (the second on non-zero moments): fp64 clip_grad_norm_ + AdamW + EMA on the scaled
    gradient; atol 1e-6 / rtol 1e-5 as tests/test_train_gpu.py::test_fused_adamw_ema_matches_torch."""
    o = _Opt(N_OPT, seed=1)
    ref = torch.nn.Parameter(o.p.double().cpu())
    ref_ema = [ref.detach().clone() for _ in o.rates]
    opt = torch.optim.AdamW([ref], lr=o.lr, betas=o.betas, eps=o.eps, weight_decay=o.wd)
    stat = torch.zeros(4, device="cuda")
    gen = torch.Generator().manual_seed(2)
    for step in (1, 2):
        o.g.copy_(torch.randn(o.n, generator=gen) * (0.1 * step))
        norm = float((o.g.double() * o.scale).norm())
        max_norm = 0.1 * norm
        ref.grad = o.g.double().cpu() * o.scale
        total = torch.nn.utils.clip_grad_norm_([ref], max_norm, error_if_nonfinite=False)
        opt.step()
        for e, r in zip(ref_ema, o.rates):
            e.mul_(r).add_(ref.detach(), alpha=1.0 - r)
        o.step_clip(step, max_norm, stat)
        assert abs(float(stat[0]) - float(total) ** 2) <= 1e-5 * float(total) ** 2
        assert abs(float(stat[1]) - max_norm / (float(total) + 1e-6)) <= 1e-6 and float(stat[1]) < 1.0
        assert torch.allclose(o.p.cpu(), ref.detach().float(), atol=1e-6, rtol=1e-5)
        assert torch.allclose(o.m.cpu(), opt.state[ref]["exp_avg"].float(), atol=1e-6, rtol=1e-5)
        assert torch.allclose(o.v.cpu(), opt.state[ref]["exp_avg_sq"].float(), atol=1e-6, rtol=1e-5)
        for e, re_ in zip(o.ema, ref_ema):
            assert torch.allclose(e.cpu(), re_.float(), atol=1e-6, rtol=1e-5)


def test_nonfinite_gradient_skips_the_step():
    """One inf, then one NaN, in the last element (which the scalar tail handles): flag up, count incremented, nothing
    written; the clean step after them updates exactly as the plain entry does."""
    o = _Opt(N_OPT, seed=3)
    o.m.normal_(); o.v.uniform_(0.0, 1.0)
    before = [t.clone() for t in o.state()]
    stat = torch.zeros(4, device="cuda")
    clean = o.g.clone()
    for k, poison in enumerate((float("inf"), float("nan"))):
        o.g.copy_(clean)
        o.g[-1] = poison
        o.step_clip(3, 1.0, stat)
        assert _ints(stat) == [1, k + 1]
        for x, y in zip(before, o.state()):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    o.g.copy_(clean)
    ref = o.clone()
    ref.step_plain(3)
    o.step_clip(3, 1e9, stat)
    assert _ints(stat) == [0, 2] and float(stat[1]) == 1.0
    for x, y in zip(ref.state(), o.state()):
        assert torch.equal(x, y)
    assert not torch.equal(o.p, before[0])


# ------------------------------------------------------------------------------------------------------------------------
# every instance and every grid shape of adamw_ema_kernel (csrc/adamw_ema_body.h)
# ------------------------------------------------------------------------------------------------------------------------
GRID_CAP = 2048 * 256                       # float4 slots of one pass of the capped grid
N_SECOND_SLOT = 4 * (GRID_CAP + 100) + 2    # one loop pass; the u = 1 slot is valid for 100 threads only; a 2-element tail
N_SECOND_PASS = 4 * (2 * GRID_CAP + 257) + 1  # a second loop pass (257 threads) whose u = 1 slot is invalid everywhere; 1-element tail


def _sqsum_adds(n):
    """Additions along the longest path of the plain entry's grad_sqsum: 8 per loop pass of a thread (two float4 slots of
    four squares), 1 for the tail element, 6 shuffle steps, 3 across the waves, one float atomic per workgroup."""
    blocks = min(2048, max(1, (n // 4 + 255) // 256))
    passes = max(1, math.ceil((n // 4) / (2 * 256 * blocks)))
    return 8 * passes + 1 + 6 + 3 + blocks, blocks, passes


def _steps_against_fp64(o, entry):
    """Two steps of the plain or the clipping entry (the second on non-zero moments) against fp64 torch.optim.AdamW (+
    clip_grad_norm_) + EMA, vectorised on the CPU: atol 1e-6 / rtol 1e-5 as test_clipped_step_matches_fp64_torch.  Plain
    entry: grad_sqsum against fp64 as well.  Its terms are non-negative, so its relative error is at most (additions
    along the longest path) * 2^-24, counted by _sqsum_adds from n."""
    from improved_diffusion import _native as nat
    ref = torch.nn.Parameter(o.p.double().cpu())
    ref_ema = [ref.detach().clone() for _ in o.rates]
    opt = torch.optim.AdamW([ref], lr=o.lr, betas=o.betas, eps=o.eps, weight_decay=o.wd)
    stat, sqsum = torch.zeros(4, device="cuda"), torch.zeros(1, device="cuda")
    gen = torch.Generator().manual_seed(o.n % 9973)
    for step in (1, 2):
        o.g.copy_(torch.randn(o.n, generator=gen) * (0.1 * step))
        ref.grad = o.g.double().cpu() * o.scale
        if entry == "clip":
            max_norm = 0.1 * float(ref.grad.norm())
            torch.nn.utils.clip_grad_norm_([ref], max_norm, error_if_nonfinite=False)
            o.step_clip(step, max_norm, stat)
            assert 0.0 < float(stat[1]) < 1.0 and _ints(stat) == [0, 0]
        else:
            want = float((ref.grad * ref.grad).sum())
            a = o.args(step)
            sqsum.zero_()
            a.grad_sqsum = sqsum.data_ptr()
            nat.check(nat.lib().lfvdm_adamw_ema(ctypes.byref(a), nat.stream()), "lfvdm_adamw_ema")
            torch.cuda.synchronize()
            adds, blocks, passes = _sqsum_adds(o.n)
            rel = abs(float(sqsum[0]) - want) / want
            print(f"[adamw sqsum] n={o.n} n_ema={len(o.rates)} step={step} blocks={blocks} passes={passes} rel.err={rel:.3e} "
                  f"bound={adds * 2.0 ** -24:.3e}")
            assert rel <= adds * 2.0 ** -24
        opt.step()
        for e, r in zip(ref_ema, o.rates):
            e.mul_(r).add_(ref.detach(), alpha=1.0 - r)
        pairs = [("p", o.p, ref.detach()), ("m", o.m, opt.state[ref]["exp_avg"]), ("v", o.v, opt.state[ref]["exp_avg_sq"])]
        pairs += [(f"ema{k}", e, re_) for k, (e, re_) in enumerate(zip(o.ema, ref_ema))]
        for name, got, want_t in pairs:
            assert torch.allclose(got.cpu(), want_t.float(), atol=1e-6, rtol=1e-5), (name, step)


@pytest.mark.parametrize("n_ema", [0, 1, 2, 3, 4])
def test_every_ema_count_matches_fp64_torch(n_ema):
    """The five NE instances of the plain entry (0..4 EMA copies, each with its own rate) at n = 5003."""
    o = _Opt(N_OPT, seed=10 + n_ema, n_ema=n_ema)
    assert len(o.ema) == n_ema and len(set(o.rates)) == n_ema
    _steps_against_fp64(o, "plain")


@pytest.mark.parametrize("entry", ["plain", "clip"])
@pytest.mark.parametrize("n", [N_SECOND_SLOT, N_SECOND_PASS], ids=["second_slot_100_threads", "second_pass_257_threads"])
def test_capped_grid_passes_match_fp64_torch(n, entry):
    """n beyond one float4 per thread of the capped 2048 x 256 grid: the clamped duplicate loads of the u = 1 slot (valid
    for 100 threads, or for none in a second loop pass of 257 threads) and the scalar tail, in both entries, one EMA copy."""
    n4 = n // 4
    _, blocks, passes = _sqsum_adds(n)
    assert blocks == 2048 and n % 4 != 0
    if n == N_SECOND_SLOT:
        assert passes == 1 and n4 - GRID_CAP == 100
    else:
        assert passes == 2 and n4 - 2 * GRID_CAP == 257
    _steps_against_fp64(_Opt(n, seed=20, n_ema=1), entry)


def _device_loop(cfg, sd, data_seed=0, **kw):
    """``TrainLoop`` at the micro config (ch32, 16 x 16, 4 frames, batch 2) on the device; ``kw``: max_grad_norm or nothing."""
    from improved_diffusion import script_util as su
    from improved_diffusion.train_util import TrainLoop
    diffusion = su.create_gaussian_diffusion(steps=1000, rescale_timesteps=True, rescale_learned_sigmas=True)
    return TrainLoop(model=build_native(cfg, sd).train(), diffusion=diffusion, data=_data(2, 12, 4, 16, data_seed), batch_size=2,
                     microbatch=-1, lr=1e-3, ema_rate="0.9", log_interval=1000, save_interval=10 ** 9, resume_checkpoint="",
                     use_fp16=False, diffusion_space_kwargs={}, fp16_scale_growth=1e-3, schedule_sampler=None, weight_decay=0.01,
                     lr_anneal_steps=0, sample_interval=None, pad_with_random_frames=True, max_frames=4, enc_dec_chunk_size=20,
                     args=argparse.Namespace(resume_id=""), **kw)


def _count_new_entries(monkeypatch):
    from improved_diffusion import _native as nat
    L = nat.lib()
    calls = {k: 0 for k in NEW_ENTRIES}
    for name in NEW_ENTRIES:
        orig = getattr(L, name)

        def counted(*a, _orig=orig, _name=name):
            calls[_name] += 1
            return _orig(*a)
        monkeypatch.setattr(L, name, counted)
    return calls


def test_trainloop_clips_every_step_and_matches_the_host_memory_arithmetic(monkeypatch):
    """Three optimizer steps at the micro config with max_grad_norm = 1e-3 (every step clips).  A second ``TrainLoop`` whose
    arenas live in host memory (``_optimize_host``: clip_grad_norm_ + AdamW + EMA in torch) receives the same gradients -
    same seed, same batch, the U-Net itself runs on the device only - and must end with the same parameters and EMA:
    atol 1e-6 / rtol 1e-5, the tolerance of tests/test_train_gpu.py::test_fused_adamw_ema_matches_torch."""
    monkeypatch.delenv("LFVDM_MAX_GRAD_NORM", raising=False)
    from test_grad_clip_cpu import make_host_loop
    cfg, sd, _ = load_case("micro")
    calls = _count_new_entries(monkeypatch)
    loop = _device_loop(cfg, sd, max_grad_norm=1e-3)
    host = make_host_loop(sd, cfg, max_grad_norm=1e-3)
    assert loop.arena.offsets == host.arena.offsets and loop.arena.numel == host.arena.numel
    torch.manual_seed(0); np.random.seed(0)
    for step in range(3):
        loop.forward_backward()
        torch.cuda.synchronize()
        host.arena.g.copy_(loop.arena.g.cpu())
        loop.optimize_normal()
        host.optimize_normal()
        loop.step += 1; host.step += 1
        torch.cuda.synchronize()
        st, hst = loop.clip_stat.cpu(), host.clip_stat
        print(f"[trainloop clip] step {step}: norm {float(st[0]) ** 0.5:.4e} coef {float(st[1]):.4e} (host {float(hst[1]):.4e})")
        assert 0.0 < float(st[1]) < 1.0 and _ints(st) == [0, 0]
        assert abs(float(st[1]) - float(hst[1])) <= 1e-5 * float(hst[1])
    assert calls == {k: 3 for k in NEW_ENTRIES}
    assert torch.allclose(loop.arena.p.cpu(), host.arena.p, atol=1e-6, rtol=1e-5)
    assert torch.allclose(loop.ema_flat[0].cpu(), host.ema_flat[0], atol=1e-6, rtol=1e-5)
    assert float((loop.arena.p.cpu() - host.arena.p).abs().max()) < 1e-5 and float((loop.arena.p - loop.ema_flat[0]).abs().max()) > 1e-4


def _three_steps(**kw):
    cfg, sd, _ = load_case("micro")
    loop = _device_loop(cfg, sd, **kw)
    torch.manual_seed(17); np.random.seed(17)
    for _ in range(3):
        loop.forward_backward()
        loop.optimize_normal()
        loop.step += 1
    torch.cuda.synchronize()
    return [loop.arena.p.clone(), loop.exp_avg.clone(), loop.exp_avg_sq.clone(), loop.ema_flat[0].clone()]


def test_trainloop_with_clipping_off_is_the_loop_without_the_keyword(monkeypatch):
    """max_grad_norm = 0 against a loop constructed without the keyword (LFVDM_DETERMINISTIC=1, so that the gradients of two
    runs are comparable bit for bit): parameters, moments and EMA bitwise equal after three steps, and not one call of the
    three new entries."""
    monkeypatch.delenv("LFVDM_MAX_GRAD_NORM", raising=False)
    monkeypatch.setenv("LFVDM_DETERMINISTIC", "1")
    calls = _count_new_entries(monkeypatch)
    without, off = _three_steps(), _three_steps(max_grad_norm=0)
    for x, y in zip(without, off):
        assert torch.equal(x, y)
    assert calls == {k: 0 for k in NEW_ENTRIES}


def _rank_worker(rank, world, port, q):
    try:
        for p in (PKG, ROOT, os.path.join(ROOT, "tests")):
            if p not in sys.path:
                sys.path.insert(0, p)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank), LFVDM_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
        os.environ.pop("LFVDM_MAX_GRAD_NORM", None)
        import torch.distributed as dist
        from improved_diffusion import dist_util
        dist_util.setup_dist()
        cfg, sd, _ = load_case("micro")
        loop = _device_loop(cfg, sd, data_seed=50 + rank, max_grad_norm=1e-3)
        assert loop.world == world and loop.use_ddp
        torch.manual_seed(100 + rank); np.random.seed(100 + rank)
        loop.forward_backward()
        local = loop.arena.g.clone()
        loop.optimize_normal()
        loop.step += 1
        torch.cuda.synchronize()

        def gathered(t):
            out = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(out, t.contiguous())
            return out

        grads = gathered(local)
        assert not torch.equal(grads[0], grads[1]), "ranks must see different data"
        stats = gathered(loop.clip_stat.view(torch.int32))
        assert torch.equal(stats[0], stats[1]), "the clip record is that of the averaged gradient on every rank"
        assert 0.0 < float(loop.clip_stat[1]) < 1.0 and loop.clip_stat.view(torch.int32)[2:].tolist() == [0, 0]
        mean_norm = float(((grads[0].double() + grads[1].double()) / world).norm())
        assert abs(float(loop.clip_stat[0]) ** 0.5 - mean_norm) <= 1e-4 * mean_norm
        for t in (loop.arena.p, loop.exp_avg, loop.ema_flat[0]):
            both = gathered(t)
            assert torch.equal(both[0], both[1])
        dist.barrier()
        q.put((rank, "ok", float(loop.clip_stat[1])))
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, "fail", traceback.format_exc()))
        raise


def test_two_ranks_agree_on_the_clipped_step():
    """Two fresh processes on one card (gloo, as tests/test_dist_gpu.py): after one clipped step the clip record, parameters,
    moments and EMA are bitwise equal across the ranks, without a collective beyond the gradient exchange."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=420) for _ in range(world)]
    for p in procs:
        p.join(60)
    for r in sorted(res):
        print(r)
    assert all(r[1] == "ok" for r in res), [r[2] for r in res if r[1] != "ok"]
    assert all(p.exitcode == 0 for p in procs)
    assert res[0][2] == res[1][2]
