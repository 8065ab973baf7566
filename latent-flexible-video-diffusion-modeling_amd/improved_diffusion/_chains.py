"""Host side of the persistent level chains (csrc/level_chain.hip): which launches of an ``_engine.Plan`` can be stages of
a chain, planning a run of them into ONE lfvdm_level_chain launch, tuning codes inside a chain, taking chains apart again.
Functions of the plan; of its state they use ``steps``, ``chains``, ``chains_off``, ``skip_side``, ``part_bases``, ``keep``,
``head`` and ``dev``."""
import ctypes as C
import os
from itertools import groupby

import torch as th

from . import _native as nat


# LFVDM_LEVEL_CHAIN=0: every launch of the low-resolution levels stays its own launch (A/B aid; the persistent level chain
# is bitwise the per-launch plan with the same tile codes).  LFVDM_CHAIN_MAX_M: launches with at most this many output rows
# (N * Ho * Wo) are candidates (640 = the 4x4 and 2x2 levels of the 20-frame, batch-2 headline configuration)
def level_chain_enabled():
    """Read when a plan is built / tuned (not at import): a process that learns late that it SHARES its GPU with another
    process - bench.py's N-ranks-on-fewer-cards rehearsal - switches the chains off for the plans it builds afterwards.  A
    chain needs all its workgroups co-resident; two processes' chains on one card can each get part of the CUs and wait for
    workgroups that cannot start (every wait is bounded: the timeout raises the abort word and the sampler falls back, but
    that costs LFVDM_CHAIN_TIMEOUT_S seconds)."""
    return os.environ.get("LFVDM_LEVEL_CHAIN", "1") != "0"


def chain_local_enabled():
    """LFVDM_CHAIN_LOCAL=0: the chains keep the split-K tile body of round 5 for every stage (A/B aid).  Default: stages on
    maps of <= 16 pixels run SAMPLE-LOCAL (csrc/conv_local_body.h: whole samples x 16 filters x all of K per work item, filter
    slice resident in LDS before the item's flags arrive, no split-K seam, GroupNorm inside one wave)."""
    return os.environ.get("LFVDM_CHAIN_LOCAL", "1") != "0"


CHAIN_MAX_M = int(os.environ.get("LFVDM_CHAIN_MAX_M", "640"))
CHAIN_TIMEOUT_S = float(os.environ.get("LFVDM_CHAIN_TIMEOUT_S", "2.0"))
_p = th.Tensor.data_ptr


# ---------------------------------------------------------------------- step -> stage
def local_tiles(a):
    """Row tiles per work item (1 | 2) if this launch runs as a SAMPLE-LOCAL chain stage, else 0.  One tile of 16 rows
    per item while the stage then fits one round of 256 workgroups, else two."""
    L = nat.lib()
    if not (chain_local_enabled() and level_chain_enabled()) or a.N * a.Ho * a.Wo > CHAIN_MAX_M or a.out_mode != nat.OUT_ROWS:
        return 0
    forced = int(os.environ.get("LFVDM_CHAIN_LOCAL_RT", "0")) or int(nat.tune_cache().get(nat.tune_key(a) + (nat.TUNE_LOCAL_RT,), 0))
    M, NS = a.N * a.Ho * a.Wo, a.Cout // 16
    order = (1, 2) if -(-M // 16) * NS <= 256 else (2, 1)
    for rt in ((forced,) if forced else order):
        if L.lfvdm_chain_local_ok(C.byref(a), rt) == 0:
            return rt
    return 0


def tile_stage_candidate(a):
    """Is this implicit-GEMM launch a candidate TILE stage of a chain (``Plan.autotune`` then picks its code among the
    variants the chain kernel holds)?  A low-resolution launch that does not run sample-local."""
    return level_chain_enabled() and a.N * a.Ho * a.Wo <= CHAIN_MAX_M and a.out_mode == nat.OUT_ROWS and local_tiles(a) == 0


def chain_stage(step, part_bases):
    """-> ChainStage for a step that can run inside a persistent level chain, else None.  ``part_bases``: output pointer of
    a lfvdm_gn_apply_part launch -> (base, first column) of the concat operand it writes one half of."""
    L = nat.lib()
    fn, args = step
    st = nat.ChainStage()
    if fn is L.lfvdm_conv_igemm:
        a = args[0]._obj
        st.cfg = local_tiles(a)
        if not st.cfg and (a.N * a.Ho * a.Wo > CHAIN_MAX_M or L.lfvdm_chain_conv_ok(C.byref(a)) != 0):
            return None
        st.kind = nat.CHAIN_LOCAL if st.cfg else nat.CHAIN_CONV
        C.memmove(C.byref(st.conv), C.byref(a), C.sizeof(nat.ConvArgs))
        return st
    g = st.gn
    if fn is L.lfvdm_gn_apply_part:
        kw = dict(zip(nat.GN_APPLY_PART_ARGS, args), film_div=1)
        g.out_base, g.out_col = part_bases[kw["out"]]
    elif fn is L.lfvdm_gn_apply:
        kw = dict(zip(nat.GN_APPLY_ARGS, args))
        if any([kw.pop(k) for k in ("coefA", "coefB", "stats")]):      # (a stage writes the activated tensor only)
            return None
    else:
        return None
    for name, v in kw.items():
        setattr(g, name, v)
    if g.N * g.P > CHAIN_MAX_M or L.lfvdm_chain_gn_ok(g.C0, g.C1, g.N, g.P) != 0:
        return None
    st.kind = nat.CHAIN_GN
    return st


# ---------------------------------------------------------------------- a run of stages -> one chain
def _free_first(run):
    """Stages that read nothing the chain produces (the skip half of a concat GroupNorm) first: the planner puts them on
    idle workgroups, and a workgroup walks the stages in list order - at the front they run at once."""
    def outs_of(st):
        return ({st.conv.out, st.conv.gn_out} if st.kind != nat.CHAIN_GN else {st.gn.out_base or st.gn.out}) - {None}

    def srcs_of(st):
        if st.kind == nat.CHAIN_GN:
            return {st.gn.src0, st.gn.src1} - {None}
        cv = st.conv
        return {cv.src0, cv.src1, cv.s2src0, cv.s2src1, cv.res} - {None}

    # free-standing stages: GroupNorms of tensors from earlier launches (the skip half of a concat normalisation) and
    # sample-local convolutions that read nothing else (the skip half of a split concat convolution)
    produced = set().union(*(outs_of(st) for _, st in run))
    free_gn = [st for _, st in run if st.kind == nat.CHAIN_GN and not (srcs_of(st) & produced)]
    gn_outs = set().union(*(outs_of(st) for st in free_gn))
    free_ids = {id(st) for st in free_gn}
    free_ids |= {id(st) for _, st in run if st.kind == nat.CHAIN_LOCAL and srcs_of(st) and srcs_of(st) <= gn_outs}
    free_ids |= {id(st) for _, st in run if st.side}
    return [e for e in run if id(e[1]) in free_ids] + [e for e in run if id(e[1]) not in free_ids]


def _plan_stages(stages, n, dev):
    """lfvdm_chain_plan on the stage array, and again under the device's cap if it holds fewer workgroups at once than the
    plan wants.  -> (deps, deps used, flags, workspace floats, counter ints, grid, lds bytes, room | None), or None."""
    from ._engine import _table_budget
    L = nat.lib()
    cap = 1 << 20
    deps = (C.c_int32 * cap)()
    used, ws_f, cnt_i = C.c_int64(), C.c_int64(), C.c_int64()
    n_flags, grid, lds = C.c_int32(), C.c_int32(), C.c_int32()

    def plan():         # (grid on entry: the most workgroups the chain may use; 0: those of a whole MI355X)
        return L.lfvdm_chain_plan(stages, n, deps, cap, C.byref(used), C.byref(n_flags), C.byref(ws_f), C.byref(cnt_i),
                                  C.byref(grid), C.byref(lds))

    if plan() != 0:
        return None
    # the chain's waits only end if ALL its workgroups are resident: ask the device how many it holds with this much
    # LDS (a partitioned / CU-masked / smaller part than the 256 CUs of a whole MI355X) and plan again under that cap
    room = None
    if dev.type == "cuda":
        room = int(L.lfvdm_chain_capacity(lds.value))
        if room < max(8, min(64, grid.value)):
            _table_budget.log(f"persistent level chain refused: the device holds {room} of its workgroups at once")
            return None
        if grid.value > room:
            grid.value = room // 8 * 8
            if plan() != 0 or grid.value > room:
                return None
    return deps, used.value, n_flags.value, ws_f.value, cnt_i.value, grid.value, lds.value, room


def make_chain(plan, run, pos, keep=True):
    """One lfvdm_level_chain launch for a run of chainable steps (list of (step, ChainStage)), or None if the planner or
    the device refuses it.  ``pos``: id(step) -> position in the per-launch step list.  keep=False: the device tables live
    only as long as the returned dict (the in-chain tuner builds hundreds of candidates).

    The chain record is a dict; bench.py, the tests and tools/chain_stamps.py read it by key:
      step     the (lfvdm_level_chain, args) tuple - the very object that stands in ``plan.steps``
      steps    the per-launch steps the chain replaces, in the order of the per-launch step list (what ``disable``
               restores: hoisted stages go back to where their launches stood)
      run      [(step, ChainStage)] in stage order (free and side stages first)
      n        number of stages;  kinds / items / codes: per stage its CHAIN_* kind, work items and tile code
      grid     workgroups;  lds: dynamic LDS bytes;  room: workgroups the device holds at once (None off the GPU)
      ctl      the control words (CHAIN_CTL_ABORT: a wait timed out)
      tensors  every device table of the launch, ctl among them: alive as long as the step may run"""
    n, dev = len(run), plan.dev
    run = _free_first(run)
    stages = (nat.ChainStage * n)(*[st for _, st in run])
    planned = _plan_stages(stages, n, dev)
    if planned is None:
        return None
    deps, used, n_flags, ws_floats, cnt_ints, grid, lds, room = planned
    ws = th.empty(max(1, ws_floats), device=dev)
    cnt = th.zeros(max(1, cnt_ints), dtype=th.int32, device=dev)
    for st in stages:
        if st.kind != nat.CHAIN_GN:
            cv = st.conv
            cv.splitk_ws, cv.splitk_cnt = _p(ws) + 4 * st.ws_off, _p(cnt) + 4 * st.cnt_off
            cv.splitk_ws_floats, cv.splitk_cnt_ints = ws.numel() - st.ws_off, cnt.numel() - st.cnt_off
    stages_dev = th.frombuffer(bytearray(bytes(memoryview(stages))), dtype=th.uint8).to(dev)
    deps_dev = th.frombuffer(bytearray(bytes(memoryview(deps))[:4 * max(1, used)]), dtype=th.int32).to(dev)
    flags = th.zeros(max(1, n_flags), dtype=th.int32, device=dev)
    ctl = th.zeros(nat.CHAIN_CTL_INTS, dtype=th.int32, device=dev)
    ch = dict(steps=sorted((sp for sp, _ in run), key=lambda sp: pos[id(sp)]), run=list(run), n=n, ctl=ctl, grid=grid, lds=lds,
              items=[s.n_items for s in stages], kinds=[s.kind for s in stages], codes=[s.conv.tune for s in stages],
              room=room, tensors=[ws, cnt, stages_dev, deps_dev, flags, ctl])
    ch["step"] = (nat.lib().lfvdm_level_chain, (_p(stages_dev), n, _p(deps_dev), _p(flags), _p(ctl), grid, lds, CHAIN_TIMEOUT_S))
    if keep:
        plan.keep += ch["tensors"]
    return ch


# ---------------------------------------------------------------------- build / take apart
def set_steps(plan, steps):
    """Replace the plan's step list; the head stays the last step if it was."""
    head_last = plan.head["step"] == len(plan.steps) - 1
    plan.steps = steps
    if head_last:
        plan.head["step"] = len(steps) - 1


def build(plan):
    """Replace every run of >= 2 consecutive chainable launches (tuned implicit GEMMs and one-wave GroupNorms of the
    low-resolution levels) by ONE persistent launch (lfvdm_level_chain) -> number of chains.  Idempotent; called by
    ``Plan.autotune``."""
    if not level_chain_enabled() or plan.chains or plan.chains_off:
        return 0
    pos = {id(sp): i for i, sp in enumerate(plan.steps)}
    # the step list in groups of consecutive (step, stage): chainable runs and, between them, steps with no stage
    staged = [(sp, chain_stage(sp, plan.part_bases)) for sp in plan.steps]
    groups = [(chainable, list(g)) for chainable, g in groupby(staged, key=lambda e: e[1] is not None)]
    # The SKIP SIDE of the decoder's split concat convolutions (GroupNorm of the encoder's skip tensor, then the skip half
    # of the convolution: _final_conv_cat / _res) depends on nothing the decoder computes: SIDE stages of their chain
    # (lfvdm_chain_stage.side: the planner reserves part of the grid for them), listed first and in the order in which the
    # main path needs them, they run beside it from the first microsecond - their operands come from earlier launches.
    # Measured alternatives: on shared workgroups at the front of the chain they kept the main path's first workgroups
    # busy for ~20 us; moved into the encoder-side chain (tail, shared workgroups) they started when that chain's main
    # path had ended (+34 us), and on a reserved quarter of that chain's grid they took 100 us for its 64.
    if os.environ.get("LFVDM_SKIP_SIDE", "1") != "0":
        for step, _ in plan.skip_side:
            for chainable, r in groups:
                for sp, st in r:
                    if chainable and sp is step and any(not x.side and x is not st for _, x in r):
                        st.side = 1
    out = []
    for chainable, r in groups:
        # (LFVDM_CHAIN_SINGLE=1: a lone sample-local launch - the 1x1 projections between the attention kernels of the middle
        # block - as a one-stage "chain".  Measured and left off: 7.7 us per launch against 5.6 for the tile kernel on
        # those 160-row, K = 128 GEMMs - with nothing to wait for, the filter fetch in front of the K loop is exposed)
        single = chainable and len(r) == 1 and r[0][1].kind == nat.CHAIN_LOCAL and os.environ.get("LFVDM_CHAIN_SINGLE", "0") == "1"
        ch = make_chain(plan, r, pos) if single or (chainable and len(r) >= 2) else None
        if ch is not None:
            plan.chains.append(ch)
        out.extend([ch["step"]] if ch is not None else [sp for sp, _ in r])
    set_steps(plan, out)
    return len(plan.chains)


def _take_apart(plan, stage_steps):
    """Every chain launch of the step list replaced by ``stage_steps(chain)``; the plan builds no chain again."""
    by_step = {id(ch["step"]): ch for ch in plan.chains}
    out = []
    for step in plan.steps:
        out.extend(stage_steps(by_step[id(step)]) if id(step) in by_step else [step])
    set_steps(plan, out)
    plan.chains, plan.chains_off = [], True


def disable(plan):
    """Back to one launch per stage (after a chain reported a timeout, or for A/B runs)."""
    _take_apart(plan, lambda ch: ch["steps"])


def split(plan):
    """Every stage of every chain as a chain of its own (one launch per stage, the SAME kernel bodies and work items: no
    flag is waited for, the launch boundary orders the stages) -> number of those launches.  Bitwise the chained plan - the
    guard that a hand-off inside a chain never delivers a stale byte; also what a plan falls back to where it must not
    depend on co-residency but wants the same numerics."""
    def singles(ch):
        at = {id(sp): i for i, sp in enumerate(ch["steps"])}
        ones = [make_chain(plan, [e], at) for e in sorted(ch["run"], key=lambda e: at[id(e[0])])]
        assert None not in ones
        return [one["step"] for one in ones]

    n = sum(ch["n"] for ch in plan.chains)
    if n:
        _take_apart(plan, singles)
    return n


def aborted(plan):
    """Did a wait inside a persistent level chain time out?  (synchronises: ONE read-back for all chains)"""
    return bool(plan.chains) and bool(th.stack([ch["ctl"][nat.CHAIN_CTL_ABORT] for ch in plan.chains]).ne(0).any().item())


# ---------------------------------------------------------------------- tuning inside a chain
def _time_chain(ch, reps, rounds):
    """Microseconds per launch of one chain on its own, back to back (minimum over `rounds`)."""
    fn, args = ch["step"]
    s = nat.stream()
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn(*args, s)
    best = float("inf")
    for _ in range(rounds):
        e0.record()
        for _ in range(reps):
            fn(*args, s)
        e1.record()
        e1.synchronize()
        best = min(best, 1000.0 * e0.elapsed_time(e1) / reps)
    if int(ch["ctl"][nat.CHAIN_CTL_ABORT].item()) != 0:
        return float("inf")
    return best


def _choice(st, a, value=None):
    """What the in-chain tuner chooses for a stage - row tiles per item (sample-local) or tile code; ``value``: set it.  The
    launch's own argument record ``a`` runs when the chain is taken apart: it gets the same tile code.  -> is it legal?"""
    local = st.kind == nat.CHAIN_LOCAL
    if value is None:
        return st.cfg if local else st.conv.tune
    if local:
        st.cfg = value
        return nat.lib().lfvdm_chain_local_ok(C.byref(st.conv), value) == 0
    st.conv.tune = a.tune = value
    return nat.lib().lfvdm_chain_conv_ok(C.byref(st.conv)) == 0


def tune(plan, reps=20, rounds=3):
    """Tile codes of the chains' GEMM stages chosen INSIDE the chain (one pass of coordinate descent: every legal code
    of a stage with the other stages at their current choice, the chain timed on its own) -> number of chains changed.
    A stand-alone launch and a chain stage have different optima: in a chain the filter pieces are in flight before the
    wait, so a third LDS-DMA stage (the whole K slice of a k-group requested up front) pays where it did not per launch,
    and a stage with more work items than workgroups runs in rounds.  Cached per launch shape (key + TUNE_IN_CHAIN)."""
    if not plan.chains or th.cuda.is_current_stream_capturing():
        return 0
    L, cache, changed = nat.lib(), nat.tune_cache(), 0
    reps = int(os.environ.get("LFVDM_TUNE_REPS", reps))
    rounds = int(os.environ.get("LFVDM_TUNE_ROUNDS", rounds))
    codes = (C.c_int * 256)()
    for ci, ch in enumerate(plan.chains):
        run, pos = ch["run"], {id(sp): i for i, sp in enumerate(ch["steps"])}
        best = [ch, None]          # the chain as it stands, and its time (None: not measured since it last changed)

        def attempt(st, a, value, measured):
            """Give one stage another choice and rebuild the chain.  Keep it if it plans and, where ``measured``, is faster
            than the best so far; else put the old choice back."""
            old, cand, t = _choice(st, a), None, None
            if _choice(st, a, value):
                if measured and best[1] is None:
                    best[1] = _time_chain(best[0], reps, rounds)
                cand = make_chain(plan, run, pos, keep=False)
            if cand is not None and measured:
                t = _time_chain(cand, reps, rounds)
            if cand is None or (measured and not t < best[1] * 0.995):
                _choice(st, a, old)
            else:
                best[:] = cand, t

        for step, st in run:
            local = st.kind == nat.CHAIN_LOCAL
            if st.kind == nat.CHAIN_GN or (local and os.environ.get("LFVDM_CHAIN_LOCAL_RT")):
                continue
            a = step[1][0]._obj
            key = nat.tune_key(a) + (nat.TUNE_LOCAL_RT if local else nat.TUNE_IN_CHAIN,)
            start = _choice(st, a)
            if key in cache:        # (measured on an earlier stage of the same shape, or in another plan)
                if cache[key] != start:     # (if it does not plan in THIS chain, the stage keeps the choice it runs with)
                    attempt(st, a, cache[key], False)
                continue
            # sample-local: row tiles per item (1 | 2), measured in the chain: one tile = more items (a second round where
            # they outnumber the workgroups), two = half the filter fetches per output row
            for value in [3 - start] if local else list(codes[:L.lfvdm_conv_igemm_candidates(C.byref(a), codes, 256)]):
                if value != start:
                    attempt(st, a, value, True)
            cache[key] = _choice(st, a)
        if best[0] is not ch:
            changed += 1
            plan.keep += best[0]["tensors"]
            set_steps(plan, [best[0]["step"] if sp is ch["step"] else sp for sp in plan.steps])
            plan.chains[ci] = best[0]
    nat.tune_cache_save()
    return changed
