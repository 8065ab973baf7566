"""The hipGraph replay machinery of the samplers and of the bits-per-dim evaluator: ``ReplayedStep`` (a private plan, its
device-side clock, the capture of one step and the chain-timeout protocol), ``GraphSampler`` and ``BpdEvaluator``.  They work
on the diffusion object they are handed; ``gaussian_diffusion`` re-exports the three names."""
import torch as th

from . import _native as nat


class ReplayedStep:
    """One step of a chain over a private plan, captured as a hipGraph over the plan's static buffers: what the sampler and
    the bits-per-dim evaluator share.  The plan and its timestep tables, the device-side clock ``t_buf``, the per-chain
    table build, the warm-up and capture of ``_step_body`` (the subclass's), the chain-timeout check and the fall-back,
    and ``step``: a single replay."""

    def __init__(self, diffusion, unet, shape, clip_denoised, inject_noise, time_tables=True, plan_rows=1):
        # time_tables=False: a plan WITHOUT timestep tables (the embedding and RPE launches stay in the step) - for a step whose
        # frame indices change from one replay to the next, where a table keyed by this chain's frames would be rebuilt every time
        # plan_rows = 2 (a sampler under classifier-free guidance): the private plan runs batch 2B - the window as given and,
        # in rows [B, 2B), the same window without its observed frames; ``clock`` is the plan's step counter (2B rows), and
        # ``t_buf``, like every B-sized buffer of the step, addresses rows [0, B) - a contiguous leading slice
        # inject_noise (parity tests): the replayed step READS ``self.noise`` - the caller fills it before every
        # ``step`` - instead of drawing it (the reference's th.randn_like, gaussian_diffusion.py:396)
        self.diffusion, self.unet, self.shape = diffusion, unet, tuple(shape)
        self.clip = bool(clip_denoised)
        self.inject_noise = bool(inject_noise)
        diffusion._check_native_modes()
        # the mean type is fixed for the life of the captured graphs (the caches live on the diffusion object: they need
        # no key element).  Not to be confused with model_kwargs["x0"], the conditioning frames
        self.x0_mode = diffusion.predicts_xstart
        B, T, Cx, H, W = self.shape
        from ._engine import Plan
        # a private plan: the chain's state lives in its static buffers, so it must not be shared
        # with eager model() calls on the same shape
        self.engine = unet.native_engine()
        # the chain walks a known schedule: everything that depends on (t, frame_indices) alone is tabulated once per
        # chain (Plan.build_time_tables / build_R_tables) instead of being recomputed by four launches in every step
        self.plan = Plan(self.engine, plan_rows * B, T, H, W, False, time_steps=diffusion.num_timesteps if time_tables else None)
        self.plan.refresh_weights()
        dev = self.plan.dev
        self.tb = diffusion.tables(dev)
        self.ts_table = diffusion.model_timestep_table(dev)
        self.clock = self.plan.t_sel if self.plan.time_steps else th.zeros(self.plan.B, dtype=th.int64, device=dev)
        self.t_buf = self.clock if plan_rows == 1 else self.clock[:B]
        self._table_events = None      # (start, end) events around the table build of the last begin()
        self._ts_key = tuple(self.ts_table.tolist())
        self.graph = None
        self.expected_t = None
        self._abort_unchecked = False       # steps have run since the chains' abort words were last read
        self.chain_timeouts = 0

    @property
    def table_build_ms(self):
        """GPU time of the table build of the last ``begin()`` (synchronises on its end event when read)."""
        if self._table_events is None:
            return 0.0
        e0, e1 = self._table_events
        e1.synchronize()
        return e0.elapsed_time(e1)

    def _build_chain_tables(self, frame_indices):
        """Once per chain, plan with timestep tables: the FiLM rows (once per set of weights), this window's R tables, the
        block the chain starts in; then the clock is put on the first timestep, so that the tuning / warm-up launches
        find valid FiLM rows.  Shared by every replayed-step class over a private plan."""
        pl, n = self.plan, self.diffusion.num_timesteps
        if not pl.time_steps:
            return
        e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        e0.record()
        if pl.tables_sig != (pl.time_signature(), self._ts_key):
            pl.build_time_tables(self.ts_table)          # once per set of weights
        pl.build_R_tables(frame_indices)                 # once per chain: R depends on this window's frames
        pl.ensure_R(n - 1)                               # (rolling window: the block the chain starts in)
        e1.record()
        self._table_events = (e0, e1)        # read lazily (table_build_ms): no host stall between windows / chains
        self.clock.fill_(n)
        pl.tick(self.clock, self.ts_table)

    def _capture_step(self):
        """Tune the plan (once), warm ``_step_body`` up on a side stream and capture it as ``self.graph``.  The plan's
        input is saved and restored around it, and so is the caller's RNG stream: building the graph draws warm-up noise,
        and a seed must give the same result whether or not this shape was seen before."""
        import os
        pl = self.plan
        rng_state = th.cuda.get_rng_state(pl.dev)
        if os.environ.get("LFVDM_AUTOTUNE", "1") != "0" and not getattr(pl, "tuned", False):
            saved0 = pl.x_in.clone()
            pl.launch()               # realistic operand contents for the timing runs
            pl.autotune()
            pl.x_in.copy_(saved0)
        # warm-up on a side stream (sets kernel attributes, fills caches), then capture
        saved = pl.x_in.clone()
        self.clock.fill_(self.diffusion.num_timesteps)
        s = th.cuda.Stream()
        s.wait_stream(th.cuda.current_stream())
        with th.cuda.stream(s):
            self._step_body()
        th.cuda.current_stream().wait_stream(s)
        g = th.cuda.CUDAGraph()
        # thread-local capture: a process group's watchdog thread may query events while this thread captures
        with th.cuda.graph(g, capture_error_mode="thread_local"):
            self._step_body()
        self.graph = g
        pl.x_in.copy_(saved)
        th.cuda.synchronize()
        th.cuda.set_rng_state(rng_state, pl.dev)

    def _begin_chain(self, x, model_kwargs):
        """``x`` becomes the plan's input; this chain's tables; the graph (first chain only); the clock on the top."""
        pl = self.plan
        if pl._sig != pl.weight_signature():
            pl.refresh_weights()  # parameters changed since the last chain
        with th.no_grad():
            pl.set_inputs(x, model_kwargs["x0"], th.zeros(pl.B, device=pl.dev), model_kwargs["frame_indices"],
                          model_kwargs["obs_mask"], model_kwargs["latent_mask"])
            self._build_chain_tables(model_kwargs["frame_indices"])
            if self.graph is None:
                self._capture_step()
            self.clock.fill_(self.diffusion.num_timesteps)     # the step pre-decrements
        self.expected_t = self.diffusion.num_timesteps - 1

    def chain_timed_out(self):
        """Did a wait inside one of the plan's persistent level chains give up (LFVDM_CHAIN_TIMEOUT_S)?  Synchronises (one
        read-back for all chains of the plan)."""
        self._abort_unchecked = False
        return bool(self.plan.chains) and self.plan.chains_aborted()

    def fall_back(self):
        """After a chain timeout: the results of the chain that just ran are not to be trusted.  Say so, run this plan one
        launch per stage from now on, and have the step graph captured again."""
        import sys
        print("[lfvdm] ERROR: a persistent level chain timed out (lfvdm_level_chain); falling back to the per-launch plan",
              file=sys.stderr, flush=True)
        self.plan.disable_chains()
        self.graph = None
        self.chain_timeouts += 1

    def step(self, i):
        if i != self.expected_t:  # arbitrary order requested: reset the device-side counter
            self.clock.fill_(i + 1)
        self.plan.ensure_R(i)
        self.graph.replay()
        self._abort_unchecked = True
        self.expected_t = max(i - 1, 0)


class GraphSampler(ReplayedStep):
    """One denoising step (timestep remap -> U-Net forward -> noise -> x_{t-1} update -> t -= 1)
    captured as a hipGraph over the engine's static buffers; ``step`` is a single replay."""

    def __init__(self, diffusion, unet, shape, clip_denoised, inject_noise=False, rule=("ancestral",)):
        # rule: ("ancestral",), ("ddim", eta) or ("dpmpp2m",) - which update closes the step; fixed for the life of the
        # captured graphs
        self.rule = tuple(rule)
        if self.rule[0] not in ("ancestral", "ddim", "dpmpp2m") or len(self.rule) != (2 if self.rule[0] == "ddim" else 1):
            raise ValueError(f"unknown update rule {rule!r}")
        # classifier-free guidance (GaussianDiffusion.set_guidance), read ONCE here - it closes both sampler cache keys: the
        # plan is built for batch 2B, begin() hands it cat[x, x] with obs_mask = 0 in the second half, the captured step
        # combines the two halves of ``plan.out`` into ``xhat`` (lfvdm_cfg_combine), updates rows [0, B) as for an x0 model
        # and mirrors them into rows [B, 2B)
        self.guidance = diffusion.guidance
        super().__init__(diffusion, unet, shape, clip_denoised, inject_noise, plan_rows=1 if self.guidance is None else 2)
        dev = self.plan.dev
        B = self.shape[0]
        # the state, the network output of the window as given: the plan's buffers, or with guidance their rows [0, B)
        self.x_rows = self.plan.x_in if self.guidance is None else self.plan.x_in[:B]
        # device tables k1 / k2 / sigma of the DDIM rule (sigma None: deterministic) or k1 / k2 / k3 of the multistep rule,
        # and what the update is launched with
        self.multistep = self.rule[0] == "dpmpp2m"
        if self.multistep:
            self.ddim = diffusion.dpm_solver_tables(dev)
        else:
            self.ddim = diffusion.ddim_tables(dev, self.rule[1]) if self.rule[0] == "ddim" else None
        self.update = diffusion._update_args(dev, self.rule)
        # dynamic thresholding (GaussianDiffusion.set_dynamic_threshold), read ONCE here - it is part of the sampler cache
        # keys: the threshold launches (lfvdm_dyn_threshold) follow the forward inside the captured step, over static
        # buffers - x0-hat, (v_lo, v_hi, s) per sample, the workspace (zero-filled once) and the window's latent frames
        # (B, T), which begin() uploads - and the update consumes ``xhat`` with the tuple of an x0-prediction model
        self.threshold = diffusion._threshold(self.clip)
        self.xhat = self.dyn_stats = self.dyn_ws = self.frame_mask = self.update_xhat = None
        self.cfg_stats = self.cfg_ws = None
        if self.threshold is not None or self.guidance is not None:
            B, T = self.shape[:2]
            self.update_xhat = diffusion._update_args(dev, self.rule, as_xstart=True)
            self.xhat = th.empty(self.shape, device=dev)
            self.frame_mask = th.ones(B, T, device=dev)
        if self.threshold is not None:
            self.dyn_stats = th.zeros(B, 3, device=dev)
            self.dyn_ws = th.zeros(nat.dyn_threshold_workspace(B, self.xhat[0].numel()), dtype=th.uint8, device=dev)
        if self.guidance is not None:
            self.cfg_stats = th.zeros(B, 3, device=dev)
            if self.guidance[1] > 0.0:
                self.cfg_ws = th.empty(nat.cfg_workspace(B, self.xhat[0].numel()), dtype=th.uint8, device=dev)
        # temporally correlated noise prior (GaussianDiffusion.set_noise_prior), read ONCE here like the threshold - it is
        # part of the sampler cache key.  begin() uploads the window's frame indices and factors their covariance once per
        # chain, outside the graph (lfvdm_noise_prior_factor); the captured step of a stochastic rule then draws L xi into
        # ``noise`` with one launch (lfvdm_noise_prior_fill) in front of the unfused, unchanged update
        self.prior = diffusion.noise_prior
        self.prior_frames = self.prior_L = None
        if self.prior is not None:
            B, T = self.shape[:2]
            self.prior_frames = th.zeros(B, T, dtype=th.int64, device=dev)
            self.prior_L = th.zeros(B, T, T, device=dev)
        self.noise = th.empty(self.shape, device=dev)
        # the step's x0-hat; under the multistep rule also the history the next step reads (in and out of one launch)
        self.pred = th.empty(self.shape, device=dev)
        # the replayed step draws its noise inside the update kernel (lfvdm_update_rng_x0: Philox keyed by a per-chain seed
        # that begin() takes from torch's generator, so th.manual_seed still fixes the video); LFVDM_SAMPLER_NOISE=torch
        # keeps the th.randn launch
        self.seed = th.zeros(1, dtype=th.int64, device=dev)
        # consecutive steps of a chain are also captured K at a time (``run``): a graph launch costs the GPU ~18 us whatever
        # it holds (1063 -> 1080 steps/s at cfg B with 8 steps per launch; 32 and more lose again); LFVDM_STEPS_PER_GRAPH=1: off
        import os
        self.K = max(1, int(os.environ.get("LFVDM_STEPS_PER_GRAPH", "8")))
        if self.plan.time_steps and self.plan.time_ring:
            self.K = min(self.K, self.plan.time_ring // 2)     # a graph launch must not walk more than half the R ring
        self.graph_k = None
        # known-region sampling (``enable_known_region``): static buffers the captured step's last launch reads
        self.known = self.known_mask = self.known_eps = self.known_noise = self.known_tb = None

    def enable_known_region(self, fixed_noise, record_noise=False):
        """Make this a known-region sampler, before its first chain: the captured step then ENDS with the blend launch
        (lfvdm_known_blend) over the static buffers ``known`` (the state's shape), ``known_mask`` (B, T, H, W) and - with
        ``fixed_noise``, the deterministic rules - ``known_eps``; ``begin`` refills them, so every chain replays the same
        graphs.  Without ``fixed_noise`` the blend draws fresh noise under the chain's ``seed`` (its own Philox stream);
        ``record_noise`` keeps what it drew in ``known_noise`` (tests)."""
        if self.graph is not None or self.graph_k is not None:
            raise RuntimeError("enable_known_region comes before the sampler's first chain: its graphs are captured already")
        B, T, _, H, W = self.shape
        dev = self.plan.dev
        self.known_tb = self.diffusion.known_region_tables(dev)
        self.known = th.zeros(self.shape, device=dev)
        self.known_mask = th.zeros(B, T, H, W, device=dev)
        self.known_eps = th.zeros(self.shape, device=dev) if fixed_noise else None
        self.known_noise = th.zeros(self.shape, device=dev) if record_noise and not fixed_noise else None

    def _step_body(self):
        """The denoising step; a known-region sampler then puts the known part back at the level the step arrived at
        (``t_buf`` still holds the timestep the step consumed)."""
        self._denoise_body()
        if self.known is not None:
            nat.known_blend(self.x_rows, self.known, self.known_mask, self.t_buf, self.known_tb["a"], self.known_tb["s"],
                            eps=self.known_eps, seed=self.seed, noise_out=self.known_noise)
            self.extra_launches += 1
        self._mirror()

    def _mirror(self, in_step=True):
        """Under guidance: the new state of rows [0, B) -> rows [B, 2B) of the plan's input (one device copy, captured with
        the step): both evaluations of the next step see the same x_t.  ``in_step`` False: the eager copy behind ``renoise``,
        which is no launch of the step and is not counted."""
        if self.guidance is not None:
            B = self.shape[0]
            self.plan.x_in[B:].copy_(self.x_rows)
            self.extra_launches += int(in_step)

    def renoise(self):
        """Resampling: the state one forward step back up, to the level of the timestep the last step consumed (the clock
        still holds it), with fresh noise under the chain's seed (lfvdm_renoise: a Philox stream of its own).  One eager
        launch between replays; the next ``step`` of the same timestep puts the clock back."""
        tb = self.known_tb
        nat.renoise(self.x_rows, self.t_buf, tb["sqrt_1mbeta"], tb["sqrt_beta"], self.seed)
        self._mirror(in_step=False)

    def _denoise_body(self):
        """The clock and the forward, then at most one update launch, chosen by where the noise comes from."""
        import os
        pl = self.plan
        recip, recipm1, c1, c2, sg, rule, mean_type = self.update
        # DDIM with eta = 0 and the multistep rule (sg is its k3): no noise of any kind, whatever the noise settings say
        det = sg is None or self.multistep
        in_kernel = det or (not self.inject_noise and os.environ.get("LFVDM_SAMPLER_NOISE", "kernel") != "torch")
        # the x_{t-1} update rides in the plan's last launch (output conv + update: lfvdm_conv_out_update_x0) where the
        # shape allows; LFVDM_FUSED_HEAD=0 keeps the two launches (A/B aid)
        # under dynamic thresholding the head conv is never fused with the update (the branch of LFVDM_FUSED_HEAD=0, whatever
        # the environment says): the quantile needs the whole x0-hat before any element can be updated
        dyn = self.threshold is not None
        cfg = self.guidance is not None      # nor under guidance: the update needs both halves of the network output
        # a noise prior takes the same branch where the step draws noise at all: L xi needs its own launch, which writes
        # ``noise`` for lfvdm_update_x0.  The deterministic rules launch nothing extra (only x_T carries the prior), and noise
        # the caller injects is used as given
        prior = self.prior is not None and not det and not self.inject_noise
        fused = (not dyn and not cfg and not prior and os.environ.get("LFVDM_FUSED_HEAD", "1") != "0" and (in_kernel or self.inject_noise)
                 and pl.fuse_head_update(self.t_buf, self.tb, self.clip, self.seed, self.noise, self.pred, self.inject_noise,
                                         ddim=self.ddim, predict_xstart=self.x0_mode))
        # device-side clock: t <- max(t - 1, 0), model timestep <- table[t]  (t_buf holds "previous t"); with timestep
        # tables it also fetches the FiLM rows of the new t, and rides in the first launch of the forward
        tick_in_conv = bool(pl.time_steps) and os.environ.get("LFVDM_TICK_IN_CONV", "1") != "0"
        if tick_in_conv:
            pl.launch(tick=(self.clock, self.ts_table))
        else:
            pl.tick(self.clock, self.ts_table)
            pl.launch()
        draw = not (fused or in_kernel or self.inject_noise)
        # launches of a step beside the plan's own (bench.py reports launches per step): the clock, the update, the draw
        # (+ the four launches of the dynamic threshold, + the fill of the noise prior)
        # (+ the one or two launches of the guidance combine; the mirror copy is counted where it is issued)
        self.extra_launches = (int(not tick_in_conv) + int(not fused) + int(draw) + (4 if dyn else 0) + int(prior)
                               + ((2 if self.guidance[1] > 0.0 else 1) if cfg else 0))
        if fused:
            return
        out, clip, x_in = pl.out, self.clip, self.x_rows
        fma = self.diffusion._x0hat_fma(self.update)
        if cfg:      # both halves of the network output -> the guided x0-hat; from here on an x0 model's output
            nat.cfg_combine(x_in, pl.out, self.t_buf, recip, recipm1, mean_type, fma, self.frame_mask, self.guidance[0],
                            self.guidance[1], self.xhat, self.cfg_stats, self.cfg_ws)
            recip, recipm1, c1, c2, sg, rule, mean_type = self.update_xhat
            out = self.xhat
        if dyn:      # x0-hat of this model's mean type -> xhat, thresholded; the update then sees an x0 model's output
            nat.dyn_threshold(x_in, out, self.t_buf, recip, recipm1, mean_type, fma,
                              self.frame_mask, self.threshold[0], self.threshold[1], self.xhat, self.dyn_stats, self.dyn_ws)
            recip, recipm1, c1, c2, sg, rule, mean_type = self.update_xhat
            out, clip = self.xhat, False
        if self.multistep:
            nat.update_ms_x0(x_in, out, self.pred, self.t_buf, recip, recipm1, c1, c2, sg, mean_type, clip, x_in,
                             self.pred)
            return
        if prior:
            if draw:      # LFVDM_SAMPLER_NOISE=torch: torch's draw, mixed in place
                self.noise.normal_()
                nat.noise_prior_fill(self.prior_L, self.noise, xi=self.noise)
            else:         # xi drawn in the kernel: the chain's key, this step's timesteps, a Philox stream of its own
                nat.noise_prior_fill(self.prior_L, self.noise, seed=self.seed, t=self.t_buf)
            nat.update_x0(x_in, out, self.noise, self.t_buf, recip, recipm1, c1, c2, sg, rule, mean_type, clip, x_in,
                          self.pred)
            return
        if in_kernel:
            nat.update_rng_x0(x_in, out, None if det else self.noise, self.t_buf, recip, recipm1, c1, c2, sg, rule,
                              mean_type, clip, x_in, None if det else self.seed, self.pred)
            return
        if draw:
            self.noise.normal_()
        nat.update_x0(x_in, out, self.noise, self.t_buf, recip, recipm1, c1, c2, sg, rule, mean_type, clip, x_in,
                      self.pred)

    def begin(self, img, model_kwargs, known=None, known_mask=None, known_eps=None):
        # callers that drive step() / run() themselves: checked once per chain, here - unless whoever ran the previous
        # chain has looked already (p_sample_loop does, behind run(): one host synchronisation per chain, not two)
        if self._abort_unchecked and self.chain_timed_out():
            self.fall_back()
        if (self.known is None) != (known is None) or (self.known_eps is None) != (known_eps is None):
            raise ValueError("known / known_mask (and known_eps under a fixed-noise rule) go to a sampler made with "
                             "enable_known_region, and to no other")
        if known is not None:      # this chain's known region -> the static buffers (no draw from torch's generator)
            self.known.copy_(known)
            self.known_mask.copy_(known_mask)
            if known_eps is not None:
                self.known_eps.copy_(known_eps)
        if self.frame_mask is not None:      # the window's latent frames steer the threshold; before the replay, never in it
            lm = model_kwargs.get("latent_mask")
            if lm is None:
                self.frame_mask.fill_(1.0)
            else:
                self.frame_mask.copy_(lm.reshape(self.frame_mask.shape))
        if self.prior is not None:           # this window's factor L, once per chain and before the (first chain's) capture
            self.prior_frames.copy_(model_kwargs["frame_indices"].reshape(self.prior_frames.shape))
            nat.noise_prior_factor(self.prior_frames, *self.prior, out=self.prior_L)
        if self.guidance is not None:        # the doubled batch: cat[x, x], obs_mask = 0 in the second half
            img = th.cat([img, img], dim=0)
            model_kwargs = self.diffusion._doubled_kwargs(model_kwargs, self.shape[0])
        self._begin_chain(img, model_kwargs)
        self.seed.random_()                                 # this chain's noise key (torch's generator: seedable)
        if self.multistep:
            self.pred.zero_()                               # no history (k3 = 0 at the chain's first step: it is not read)

    def fall_back(self):
        super().fall_back()
        self.graph_k = None

    def chain_table_ms(self):
        """GPU milliseconds of ALL table building of one chain of this sampler (every R block once; the FiLM rows are per
        set of weights and not included): with the rolling window the refills ride between the graph launches of ``run``,
        this measures them on their own (synchronises)."""
        pl = self.plan
        if not pl.time_steps:
            return 0.0
        e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        th.cuda.synchronize()
        e0.record()
        pl.fill_whole_chain()
        e1.record()
        e1.synchronize()
        if self.expected_t is not None:
            pl.ensure_R(self.expected_t)
        return e0.elapsed_time(e1)

    def _state(self):
        return {"sample": self.x_rows, "pred_xstart": self.pred, "attn": None}

    def _check_order(self, i):
        """A multistep chain walks consecutive timesteps (its history is the step before); n - 1 starts a chain over."""
        if self.multistep and i != self.expected_t and i != self.diffusion.num_timesteps - 1:
            raise ValueError(f"the multistep rule {self.rule!r} walks consecutive timesteps: expected t = {self.expected_t} "
                             f"(or {self.diffusion.num_timesteps - 1}, a new chain), got {i}")

    def step(self, i):
        self._check_order(i)
        super().step(i)
        return self._state()

    def run(self, i, n):
        """``n`` consecutive steps t = i, i-1, ... (the clock stops at 0): exactly ``step`` n times - the noise is keyed by
        (chain seed, t, element), the clock lives on the device - but K steps per graph launch while at least K remain."""
        if self.inject_noise and n > 1:
            raise ValueError("inject_noise: the caller provides the noise of every step - use step()")
        self._check_order(i)
        if i != self.expected_t:
            self.clock.fill_(i + 1)
        left, t = int(n), int(i)
        if self.K > 1 and left >= self.K:
            if self.graph_k is None:
                g = th.cuda.CUDAGraph()
                th.cuda.synchronize()
                with th.no_grad(), th.cuda.graph(g, capture_error_mode="thread_local"):
                    for _ in range(self.K):
                        self._step_body()
                self.graph_k = g
            while left >= self.K:
                self.plan.ensure_R(t, t - self.K + 1)      # rolling R window: the timesteps this launch walks
                self.graph_k.replay()
                left -= self.K
                t = max(t - self.K, 0)
        for _ in range(left):
            self.plan.ensure_R(t)
            self.graph.replay()
            t = max(t - 1, 0)
        self._abort_unchecked = True
        self.expected_t = max(int(i) - int(n), 0)
        return self._state()


class BpdEvaluator(ReplayedStep):
    """One evaluation step of ``calc_bpd_loop`` (clock tick -> noise draw -> q_sample into the plan's input -> U-Net forward
    -> lfvdm_vb_terms into column j of the (N, T) results) captured as a hipGraph over a private plan with timestep
    tables; ``step(i)`` - a single replay - writes the term of timestep ``i`` to column num_timesteps - 1 - i of ``vb`` /
    ``xstart_mse`` / ``mse``: the column index is derived on the device from the clock."""

    def __init__(self, diffusion, unet, shape, clip_denoised, inject_noise=False):
        super().__init__(diffusion, unet, shape, clip_denoised, inject_noise)
        # the evaluator always walks with timestep tables (the sampler also serves plans without them)
        assert self.plan.time_steps == diffusion.num_timesteps and self.plan.t_sel is not None
        B, T, n, dev = self.plan.B, self.plan.T, diffusion.num_timesteps, self.plan.dev
        self.x_start = th.empty(self.shape, device=dev)
        self.noise = th.empty(self.shape, device=dev)
        self.mask = th.ones(B, T, device=dev)
        self.vb, self.xstart_mse, self.mse = (th.zeros(B, n, device=dev) for _ in range(3))

    def _step_body(self):
        pl, tb, d = self.plan, self.tb, self.diffusion
        pl.tick(self.t_buf, self.ts_table)          # t <- max(t - 1, 0), model timestep and FiLM rows of the new t
        if not self.inject_noise:
            self.noise.normal_()                    # torch's graph-safe generator (th.manual_seed fixes the evaluation)
        nat.q_sample(self.x_start, self.noise, self.t_buf, tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"], pl.x_in)
        pl.launch()
        recip, recipm1, c1, c2, post_lv, model_lv = d._vb_tables(pl.dev)
        nat.vb_terms(self.x_start, pl.x_in, pl.out, self.noise, self.t_buf, recip, recipm1, c1, c2, post_lv, model_lv, self.mask,
                     nat.MEAN_X0 if self.x0_mode else nat.MEAN_EPS, self.clip, self.vb, self.xstart_mse, self.mse, None,
                     col_base=d.num_timesteps - 1)

    def begin(self, x_start, model_kwargs, latent_mask=None):
        with th.no_grad():
            self.x_start.copy_(x_start)
            if latent_mask is None:
                self.mask.fill_(1.0)
            else:
                self.mask.copy_(latent_mask.reshape(self.mask.shape))
        self._begin_chain(self.x_start, model_kwargs)

    def evaluate(self, x_start, model_kwargs, latent_mask=None):
        """Every timestep, descending -> fresh (N, T) copies of vb, xstart_mse, mse.  A persistent level chain that gave
        up a wait leaves garbage behind: the walk is then run again, one launch per stage (the samplers' protocol)."""
        n = self.diffusion.num_timesteps
        for attempt in range(2):
            self.begin(x_start, model_kwargs, latent_mask)
            for i in range(n - 1, -1, -1):
                self.step(i)
            if attempt == 0 and self.chain_timed_out():
                self.fall_back()
                continue
            break
        return self.vb.clone(), self.xstart_mse.clone(), self.mse.clone()
