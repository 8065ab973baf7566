"""Windowed long-video sampling: fill a (B, T, C, H, W) video window by window, each window one
``p_sample_loop`` (``args.use_ddim``: ``ddim_sample_loop`` with ``eta = args.ddim_eta``; ``args.use_dpm_solver``:
``dpm_solver_sample_loop``) over at most ``max_frames`` frames chosen by a sampling scheme.

Behaviour of ``sample_video`` in the reference's scripts/video_sample.py:28-85 (same arguments, same return
value), restructured for the MI355X path:
  * the running ``samples`` tensor lives on the device, so a window costs two device gathers and one scatter
    instead of host<->device round trips of the whole window;
  * windows of the same length share one captured hipGraph and one set of autotuned launches
    (``GaussianDiffusion._graph_sampler`` keeps the few shapes a schedule uses);
  * for latent-space models the window is written back as LATENTS (``return_decoded=False``): the reference
    writes decoded pixels into the latent tensor, which only works for pixel-space models.
"""
from types import SimpleNamespace

import torch as th

from .sampling_schemes import AdaptiveSamplingSchemeBase, sampling_schemes


def window_inputs(samples, obs_frame_indices, latent_frame_indices, device=None):
    """(frame_indices, x0, obs_mask, latent_mask) of one window: observed frames first, then the latents
    (reference video_sample.py:56-61).  ``*_frame_indices`` are per-video lists."""
    B = samples.shape[0]
    device = samples.device if device is None else device
    obs = th.as_tensor(obs_frame_indices, dtype=th.long).view(B, -1)
    lat = th.as_tensor(latent_frame_indices, dtype=th.long).view(B, -1)
    frame_indices = th.cat([obs, lat], dim=1).to(device)
    rows = th.arange(B, device=samples.device)[:, None]
    x0 = samples[rows, frame_indices.to(samples.device)].to(device)      # advanced indexing copies
    obs_mask = th.cat([th.ones_like(obs), th.zeros_like(lat)], dim=1).view(B, -1, 1, 1, 1).float().to(device)
    return frame_indices, x0, obs_mask, 1 - obs_mask


@th.no_grad()
def sample_video(args, model, diffusion, batch, just_get_indices=False, verbose=True, known_video=None, known_mask=None):
    """batch: (B, T, C, H, W); the first ``args.n_obs`` frames are observed, the rest are generated.

    args needs: n_obs, max_frames, max_latent_frames, sampling_scheme, clip_denoised, device and optionally
    optimality / eval_dir (an ``optimal_schedule.pt`` under eval_dir), use_ddim / ddim_eta (DDIM instead of the ancestral
    chain; in the reference ``--use_ddim`` only renames the results folder, here it selects the sampler), use_dpm_solver
    (DPM-Solver++(2M) instead; together with use_ddim: ValueError), dynamic_threshold / dynamic_threshold_max (a percentile
    and an optional cap: ``diffusion.set_dynamic_threshold`` is called with them before the first window; without the
    attribute, LFVDM_DYNAMIC_THRESHOLD="0.995" or "0.995:1.5" is read; neither: the diffusion's setting stays), guidance_scale / guidance_rescale
    (classifier-free guidance on the observed frames: ``diffusion.set_guidance`` is called with them before the first window;
    without guidance_scale, LFVDM_GUIDANCE="2" or "2:0.7" is read; neither: the diffusion's setting stays), noise_prior (a spec
    of ``noise_prior.parse_noise_prior`` for ``diffusion.set_noise_prior``, else LFVDM_NOISE_PRIOR, resolved the same way;
    ``trained_noise_prior``, the spec in the checkpoint's config, is compared with it and a difference is logged; a prior
    together with known_video: NotImplementedError), adaptive_metric (a spec of ``frame_select.parse_frame_metric``, "msl2:1" ..
    "msl2:3", else LFVDM_ADAPTIVE_METRIC: the adaptive schemes pick their conditioning frames by this network-free frame distance
    instead of LPIPS; with a non-adaptive scheme: ValueError; on a device the batch must be float32 - other dtypes: ValueError at
    the first selection - and the running samples are then allocated row-major even for a permuted batch).  Returns ``(samples, indices_used)``
    with ``samples`` on batch's device and ``indices_used`` the list of (obs, latent) index lists per window.

    ``known_video`` (B, T, C, H, W) with ``known_mask`` (B, T, H, W), both or neither (not in the reference): the part of
    the video's generated frames that is known - inpainting, outpainting.  Each window gathers its frames of the two and
    runs ``known_region_sample_loop`` under the sampler the flags above select; where the mask is 1 the sampled frames
    equal ``known_video``.
    """
    if (known_video is None) != (known_mask is None):
        raise ValueError("known_video and known_mask come together")
    if known_video is not None:
        if tuple(known_video.shape) != tuple(batch.shape):
            raise ValueError(f"known_video has the shape of batch {tuple(batch.shape)}, got {tuple(known_video.shape)}")
        if tuple(known_mask.shape) != (batch.shape[0], batch.shape[1], *batch.shape[3:]):
            raise ValueError(f"known_mask is (B, T, H, W) of batch, got {tuple(known_mask.shape)}")
    B, T = batch.shape[:2]
    use_dpm_solver = bool(getattr(args, "use_dpm_solver", False))
    if use_dpm_solver and getattr(args, "use_ddim", False):
        raise ValueError("use_ddim and use_dpm_solver select different samplers: set one of them")
    thr = resolve_dynamic_threshold(args)
    if thr is not None:      # before the first window: the samplers read the setting when they are built
        diffusion.set_dynamic_threshold(**thr)
    cfg = resolve_guidance(args)
    if cfg is not None:      # likewise
        diffusion.set_guidance(**cfg)
    prior = resolve_noise_prior(args)
    if prior is not None:    # likewise; "none" turns a prior off, no setting at all leaves the diffusion object as it is
        diffusion.set_noise_prior(prior)
    if getattr(args, "trained_noise_prior", None) is not None:
        warn_noise_prior_mismatch(args.trained_noise_prior, diffusion.noise_prior)
    device = th.device(args.device)
    metric = resolve_adaptive_metric(args)
    if metric is not None and not issubclass(sampling_schemes[args.sampling_scheme], AdaptiveSamplingSchemeBase):
        raise ValueError(f"adaptive_metric = {metric!r} is for the adaptive sampling schemes; {args.sampling_scheme!r} chooses its "
                         "conditioning frames without looking at them")
    if metric is None:
        samples = th.zeros_like(batch, device=device)
    else:      # the distance kernel reads the frames in place: row-major, whatever the strides of a permuted batch
        samples = th.zeros_like(batch, device=device, memory_format=th.contiguous_format)
    samples[:, :args.n_obs] = batch[:, :args.n_obs].to(device)
    optimality = getattr(args, "optimality", None)
    schedule_path = None if optimality is None else args.eval_dir / "optimal_schedule.pt"
    scheme = iter(sampling_schemes[args.sampling_scheme](
        video_length=T, num_obs=args.n_obs, max_frames=args.max_frames, step_size=args.max_latent_frames,
        optimal_schedule_path=schedule_path))
    if metric is not None:
        scheme.set_frame_metric(metric)
    batch_dev = batch.to(device) if just_get_indices else None
    decoded = getattr(diffusion, "diffusion_space", None) in (None, "pixel")
    rows = th.arange(B, device=device)[:, None]
    if known_video is not None:
        known_video, known_mask = known_video.to(device), known_mask.to(device=device, dtype=th.float32)
    indices_used = []
    while True:
        scheme.set_videos(samples)         # only the adaptive schemes look at the frames
        try:
            obs_idx, lat_idx = next(scheme)
        except StopIteration:
            break
        if verbose:
            print(f"Conditioning on {sorted(obs_idx)} frames, predicting {sorted(lat_idx)}.")
        frame_indices, x0, obs_mask, latent_mask = window_inputs(samples, obs_idx, lat_idx, device)
        n_lat = len(lat_idx[0])
        if just_get_indices:
            local = batch_dev[rows, frame_indices]
        elif known_video is not None:
            sampler = "dpm_solver" if use_dpm_solver else "ddim" if getattr(args, "use_ddim", False) else "ancestral"
            local = diffusion.known_region_sample_loop(
                model, tuple(x0.shape), known_video[rows, frame_indices], known_mask[rows, frame_indices], sampler=sampler,
                eta=getattr(args, "ddim_eta", 0.0), clip_denoised=args.clip_denoised,
                model_kwargs=dict(frame_indices=frame_indices, x0=x0, obs_mask=obs_mask, latent_mask=latent_mask),
                latent_mask=latent_mask, return_decoded=decoded)
        elif use_dpm_solver:
            local = diffusion.dpm_solver_sample_loop(
                model, tuple(x0.shape), clip_denoised=args.clip_denoised,
                model_kwargs=dict(frame_indices=frame_indices, x0=x0, obs_mask=obs_mask, latent_mask=latent_mask),
                latent_mask=latent_mask, return_decoded=decoded)
        elif getattr(args, "use_ddim", False):
            local = diffusion.ddim_sample_loop(
                model, tuple(x0.shape), clip_denoised=args.clip_denoised,
                model_kwargs=dict(frame_indices=frame_indices, x0=x0, obs_mask=obs_mask, latent_mask=latent_mask),
                eta=getattr(args, "ddim_eta", 0.0), latent_mask=latent_mask, return_decoded=decoded)
        else:
            local, _ = diffusion.p_sample_loop(
                model, tuple(x0.shape), clip_denoised=args.clip_denoised,
                model_kwargs=dict(frame_indices=frame_indices, x0=x0, obs_mask=obs_mask, latent_mask=latent_mask),
                latent_mask=latent_mask, return_attn_weights=False, return_decoded=decoded)
        samples[rows, frame_indices[:, -n_lat:]] = local[:, -n_lat:]
        indices_used.append((obs_idx, lat_idx))
    return samples.to(batch.device), indices_used


def resolve_dynamic_threshold(args):
    """``args.dynamic_threshold`` (with ``args.dynamic_threshold_max``) > LFVDM_DYNAMIC_THRESHOLD > None (leave the diffusion
    object as it is) -> the keyword arguments of ``GaussianDiffusion.set_dynamic_threshold``, or None."""
    import os
    from .gaussian_diffusion import parse_dynamic_threshold
    pct = getattr(args, "dynamic_threshold", None)
    if pct is not None:
        return {"percentile": pct, "max_value": getattr(args, "dynamic_threshold_max", None)}
    if getattr(args, "dynamic_threshold_max", None) is not None:
        raise ValueError("dynamic_threshold_max needs dynamic_threshold")
    spec = os.environ.get("LFVDM_DYNAMIC_THRESHOLD")
    return None if spec is None else parse_dynamic_threshold(spec)


def resolve_guidance(args):
    """``args.guidance_scale`` (with ``args.guidance_rescale``) > LFVDM_GUIDANCE > None (leave the diffusion object as it is)
    -> the keyword arguments of ``GaussianDiffusion.set_guidance``, or None."""
    import os
    from .gaussian_diffusion import parse_guidance
    scale = getattr(args, "guidance_scale", None)
    rescale = getattr(args, "guidance_rescale", None)
    if scale is not None:
        return {"scale": scale, "rescale": 0.0 if rescale is None else rescale}
    if rescale is not None:
        raise ValueError("guidance_rescale needs guidance_scale")
    spec = os.environ.get("LFVDM_GUIDANCE")
    return None if spec is None else parse_guidance(spec)


def resolve_noise_prior(args):
    """``args.noise_prior`` > LFVDM_NOISE_PRIOR > None (leave the diffusion object as it is) -> the spec for
    ``GaussianDiffusion.set_noise_prior`` ("none" included: it turns a prior off), or None.  Malformed: ValueError."""
    import os
    from .noise_prior import parse_noise_prior
    spec = getattr(args, "noise_prior", None)
    if spec is None:
        spec = os.environ.get("LFVDM_NOISE_PRIOR")
    if spec is None:
        return None
    parse_noise_prior(spec)
    return spec


def resolve_adaptive_metric(args):
    """``args.adaptive_metric`` > LFVDM_ADAPTIVE_METRIC > None (the adaptive schemes keep their embedding route) -> the spec for
    ``AdaptiveSamplingSchemeBase.set_frame_metric`` ("msl2:L").  Malformed: ValueError."""
    import os
    from .frame_select import parse_frame_metric
    spec = getattr(args, "adaptive_metric", None)
    if spec is None:
        spec = os.environ.get("LFVDM_ADAPTIVE_METRIC")
    if spec is None:
        return None
    parse_frame_metric(spec)
    return spec


def warn_noise_prior_mismatch(trained, sampling):
    """A checkpoint records the prior it was trained with (``config["noise_prior"]``; a caller hands it over as
    ``args.trained_noise_prior``).  Sampling it under another prior is allowed - and said in the log.  -> whether it warned."""
    import logging
    from .noise_prior import format_noise_prior, parse_noise_prior
    if trained is None:
        return False
    a, b = parse_noise_prior(trained), parse_noise_prior(sampling)
    if a == b:
        return False
    logging.getLogger("improved_diffusion").warning(
        "the checkpoint was trained with the noise prior %r and is sampled with %r", format_noise_prior(a), format_noise_prior(b))
    return True


def default_sampling_args(**kw):
    """Namespace with the defaults of the reference CLI (video_sample.py:171-192) for programmatic use."""
    d = dict(sampling_scheme="autoreg", n_obs=36, max_frames=20, max_latent_frames=None, clip_denoised=True,
             optimality=None, eval_dir=None, use_ddim=False, ddim_eta=0.0, use_dpm_solver=False,
             dynamic_threshold=None, dynamic_threshold_max=None, guidance_scale=None, guidance_rescale=None, noise_prior=None, adaptive_metric=None,
             device="cuda" if th.cuda.is_available() else "cpu")
    d.update(kw)
    if d["use_ddim"] and d["use_dpm_solver"]:
        raise ValueError("use_ddim and use_dpm_solver select different samplers: set one of them")
    if d["max_latent_frames"] is None:
        d["max_latent_frames"] = d["max_frames"] // 2
    return SimpleNamespace(**d)
