"""Frame distances and greedy farthest-point selection that need no network: what the adaptive sampling schemes
(``sampling_schemes.AdaptiveSamplingSchemeBase.set_frame_metric``, ``sample_video`` with ``adaptive_metric``) choose their
conditioning frames with when the LPIPS package is not there.

    parse_frame_metric(spec)                                  -> levels L of "msl2:L", L in {1, 2, 3}
    frame_distance_reference(a, b, levels)                    -> the definition, float64 torch (CPU path and test oracle)
    frame_distances(videos, new, cand, levels, out=None)      -> dist (B, T, T): rows / columns of ``new`` against new + cand
    farthest_point_select(dist, cand, n, forced=(0,))         -> per video, n frame indices (Python lists)
    FrameDistanceCache(levels).update(videos, done_frames)    -> dist with every pair of done frames, each computed once

The metric is a multi-scale mean squared difference.  For two frames a, b of shape (C, H, W)

    d_L(a, b) = (1 / L) * sum_{l = 0..L-1} mean((P_l(a - b))^2),     P_0 = identity, P_l = 2^l x 2^l average pooling,

H and W multiples of 2^(L-1).  "msl2:1" is the plain mean squared difference: the same argmax structure as an identity
``embed_fn``.  It is taken in whatever space ``sample_video`` holds its samples in (pixels, wavelet coefficients, VAE
latents).  NO claim is made that it matches LPIPS perceptually, and its effect on sample quality has not been measured.

Device tensors go through csrc/frame_select.hip (lfvdm_frame_dist_rows, lfvdm_fps_select: fixed summation order, no
atomics, d(i, j) and d(j, i) the same bits, one launch for all picks of a window and ONE device-to-host copy of (B, n)
int32, the only synchronisation of a window); CPU tensors take the same semantics in float64 torch.
"""
import numpy as np
import torch
import torch.nn.functional as F

MAX_LEVELS = 3
MAX_FRAMES = 4096      # the cache's (B, T, T) float32 matrix is 64 MB per video there


def parse_frame_metric(spec):
    """"msl2:L" with L in {1, 2, 3} -> L.  Anything else: ValueError."""
    if isinstance(spec, str):
        name, sep, lv = spec.strip().partition(":")
        if name == "msl2" and sep and lv in ("1", "2", "3"):
            return int(lv)
    raise ValueError(f"frame metric must be 'msl2:L' with L in 1..{MAX_LEVELS}, got {spec!r}")


def _check_levels(levels, H, W):
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels must be an integer in 1..{MAX_LEVELS}, got {levels!r}")
    S = 1 << (levels - 1)
    if H % S or W % S:
        usable = max(lv for lv in range(1, MAX_LEVELS + 1) if H % (1 << (lv - 1)) == 0 and W % (1 << (lv - 1)) == 0)
        raise ValueError(f"frames of {H} x {W} are no multiple of {S} x {S}: {levels} levels do not fit, the largest usable "
                         f"L is {usable} ('msl2:{usable}')")
    return int(levels)


def frame_distance_reference(a, b, levels=1):
    """d_L of ``a`` against ``b``, both (..., C, H, W) and broadcastable, in float64 -> float64 of the broadcast lead shape."""
    if a.dim() < 3 or b.dim() < 3:
        raise ValueError(f"frames are (..., C, H, W), got {tuple(a.shape)} and {tuple(b.shape)}")
    d = a.double() - b.double()
    C, H, W = d.shape[-3:]
    levels = _check_levels(levels, H, W)
    lead = d.shape[:-3]
    d = d.reshape(-1, C, H, W)
    total = torch.zeros(d.shape[0], dtype=torch.float64, device=d.device)
    for lv in range(levels):
        p = d if lv == 0 else F.avg_pool2d(d, 1 << lv)
        total = total + (p * p).mean(dim=(1, 2, 3))
    return (total / levels).reshape(lead)


def _as_frames(videos):
    """(B, T, C, H, W), or (B, T, D) vectors as C = D, H = W = 1."""
    if not torch.is_tensor(videos) or videos.dim() not in (3, 5):
        raise ValueError("videos must be a (B, T, C, H, W) or (B, T, D) tensor")
    if videos.numel() == 0:
        raise ValueError(f"empty videos {tuple(videos.shape)}")
    if videos.dim() == 3:
        return videos.unsqueeze(-1).unsqueeze(-1)
    return videos


def _index_list(name, idx, T):
    idx = [int(i) for i in idx]
    for i in idx:
        if not 0 <= i < T:
            raise ValueError(f"{name} holds frame {i}, outside [0, {T})")
    return idx


def frame_distances(videos, new, cand, levels=1, out=None):
    """For every video b, every i in ``new`` and every j in ``new`` + ``cand`` (lists of frame indices shared by the batch; any
    order, may repeat and overlap): dist[b, i, j] = dist[b, j, i] = d_L(videos[b, i], videos[b, j]), exactly 0 for i == j.
    Nothing else of ``out`` (B, T, T) is touched; without ``out`` a NaN-filled matrix is made.  Device videos (float32,
    contiguous): one native launch into a float32 matrix; CPU videos: float64 torch into a float64 matrix."""
    v = _as_frames(videos)
    B, T, C, H, W = v.shape
    levels = _check_levels(levels, H, W)
    new, cand = _index_list("new", new, T), _index_list("cand", cand, T)
    dtype = torch.float32 if v.is_cuda else torch.float64
    if out is None:
        out = torch.full((B, T, T), float("nan"), dtype=dtype, device=v.device)
    elif tuple(out.shape) != (B, T, T) or out.dtype != dtype or out.device != v.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous ({B}, {T}, {T}) {dtype} tensor on {v.device}")
    if not new:
        return out
    if v.is_cuda:
        if v.dtype != torch.float32 or not v.is_contiguous():
            raise ValueError(f"device videos must be contiguous float32, got {v.dtype}" + ("" if v.is_contiguous() else ", strided"))
        from . import _native as nat
        with torch.cuda.device(v.device):
            lists = torch.tensor(new + cand, dtype=torch.int32).to(v.device, non_blocking=True)
            nat.frame_dist_rows(v, B, T, C, H, W, levels, lists[:len(new)], lists[len(new):] if cand else None, out)
        return out
    tgt = new + cand
    for i in new:
        d = frame_distance_reference(v[:, tgt], v[:, i:i + 1], levels)      # (B, n_tgt)
        d[:, [k for k, j in enumerate(tgt) if j == i]] = 0.0
        out[:, i, tgt] = d
        out[:, tgt, i] = d
    return out


def _host_select(row_of, n_cand, n, forced):
    """The selection loop on one video: row_of(p) -> distances of candidate p to all candidates (numpy)."""
    min_d = np.full(n_cand, np.inf)
    picks = [forced[0]]
    for i in range(1, n):
        min_d = np.minimum(min_d, row_of(picks[-1]))
        picks.append(forced[i] if i < len(forced) else int(np.argmax(min_d)))
    return picks


def farthest_point_select(dist, cand, n, forced=(0,)):
    """Greedy farthest-point selection on ``dist`` (B, T, T) among the frames ``cand`` (a list shared by the batch):

        picks[0] = forced[0];  for i = 1..n-1:  min_d = min(min_d, dist[cand[picks[i-1]], cand]), starting from +inf,
        picks[i] = forced[i] if i < len(forced) else the lowest position of the maximum of min_d   (np.argmax)

    ``forced``: positions into ``cand``, at least one.  n > len(cand) repeats frames as that loop does.  -> per video the
    list of n frame indices.  Device matrices: one launch and one device-to-host copy of (B, n) int32."""
    if not torch.is_tensor(dist) or dist.dim() != 3 or dist.shape[1] != dist.shape[2]:
        raise ValueError("dist must be a (B, T, T) tensor")
    B, T = dist.shape[:2]
    cand = _index_list("cand", cand, T)
    forced = [int(p) for p in forced]
    n = int(n)
    if not cand or not forced or n < 1:
        raise ValueError("farthest_point_select needs at least one candidate, one forced position and n >= 1")
    for p in forced:
        if not 0 <= p < len(cand):
            raise ValueError(f"forced position {p} is outside the {len(cand)} candidates")
    forced = forced[:n]
    if dist.is_cuda:
        if dist.dtype != torch.float32 or not dist.is_contiguous():
            raise ValueError("a device dist must be contiguous float32")
        if len(cand) > MAX_FRAMES:
            raise ValueError(f"at most {MAX_FRAMES} candidates on the device, got {len(cand)}")
        from . import _native as nat
        with torch.cuda.device(dist.device):
            lists = torch.tensor(cand + forced, dtype=torch.int32).to(dist.device, non_blocking=True)
            picks = torch.empty(B, n, dtype=torch.int32, device=dist.device)
            nat.fps_select(dist, B, T, lists[:len(cand)], lists[len(cand):], n, picks)
        picks = picks.cpu().tolist()      # the one synchronisation
    else:
        ci = torch.as_tensor(cand, dtype=torch.long)
        sub = dist[:, ci][:, :, ci].numpy()      # (B, n_cand, n_cand)
        picks = [_host_select(lambda p, b=b: sub[b, p], len(cand), n, forced) for b in range(B)]
    return [[cand[p] for p in row] for row in picks]


class FrameDistanceCache:
    """The (B, T, T) distance matrix of one batch of videos that is filled in while they are generated, and the set of frames
    it covers: every pair of finished frames is compared once per video, not once per window."""

    def __init__(self, levels=1):
        if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= levels <= MAX_LEVELS:
            raise ValueError(f"levels must be an integer in 1..{MAX_LEVELS}, got {levels!r}")
        self.levels = int(levels)
        self.dist = None
        self.cached = []        # frames covered, in the order they came
        self._key = None

    def update(self, videos, done_frames):
        """Bring the matrix up to ``done_frames`` (frames of ``videos`` that hold their final value) -> dist.  One launch for the
        frames that became done since the last call; a different tensor (data_ptr, shape or device) starts over."""
        v = _as_frames(videos)
        T = v.shape[1]
        if T > MAX_FRAMES:
            raise ValueError(f"videos of {T} frames: the distance cache holds a T x T matrix per video and stops at {MAX_FRAMES} "
                             f"frames (64 MB per video)")
        key = (v.data_ptr(), tuple(v.shape), v.device, v.dtype)
        if key != self._key:
            self._key, self.cached, self.dist = key, [], None
        have = set(self.cached)
        new = sorted(set(_index_list("done_frames", done_frames, T)) - have)
        if self.dist is None:
            self.dist = frame_distances(v, [], [], self.levels)
        if new:
            frame_distances(v, new, self.cached, self.levels, out=self.dist)
            self.cached.extend(new)
        return self.dist
