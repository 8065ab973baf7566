"""The ``bouncing_shapes`` dataset: a few coloured discs and squares that move and bounce in the frame (the family of
Moving-MNIST and of the stochastic bouncing shapes of Denton & Fergus 2018).  No files: a video is a function of
``(seed, split, video index)`` and the parameters, defined in INTEGER arithmetic by the header comment of
``csrc/shapes.hip``.  This module is the host reference written from that comment (numpy) - what ``Dataset.__getitem__``
returns, so the dataset works with a DataLoader and without a GPU - plus the device source that renders the same bytes with
the two kernels (``lfvdm_shapes_trajectories``, ``lfvdm_shapes_render``), straight into a training micro-batch.

    python -m improved_diffusion.shapes --out V.npy --n 8 --T 40 [--split test] [--uint8]

writes videos (N, T, 3, H, W) for eyeballing, or as the ``--truth`` file of ``python -m improved_diffusion.video_metrics``.
"""
import argparse
import os
from dataclasses import dataclass

import numpy as np
import torch as th
from torch.utils.data import Dataset

from .video_datasets import _frames_uint8_to_signed_unit

DATASET_NAME = "bouncing_shapes"
SPLITS = {"train": 0, "test": 1}
STREAM, INIT, VELOCITY, BOUNCE = 0x53480000, 0, 1, 2
PALETTE = np.array([[230, 40, 40], [40, 200, 60], [60, 90, 240], [240, 220, 50],
                    [230, 60, 220], [50, 220, 230], [250, 140, 30], [245, 245, 245]], dtype=np.int64)
BACKGROUND = (0, 0, 0)
KIND_DISC, KIND_SQUARE = 0, 1

_M32 = np.uint64(0xFFFFFFFF)
_SH32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) of the counter words under the key (k0, k1), vectorised -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> _SH32) ^ c1 ^ np.uint64(k0)) & _M32, p1 & _M32, ((p0 >> _SH32) ^ c3 ^ np.uint64(k1)) & _M32, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def split_seed(seed):
    s = int(seed) % (1 << 64)
    return s & 0xFFFFFFFF, s >> 32


def stream_word(split, purpose):
    return STREAM | (SPLITS[split] << 8) | purpose


@dataclass(frozen=True)
class ShapesParams:
    H: int = 64
    W: int = 64
    n_shapes: int = 2
    T: int = 100
    stochastic: bool = True
    seed: int = 0

    def __post_init__(self):
        for name, v in (("H", self.H), ("W", self.W)):
            if not (8 <= v <= 256 and v % 4 == 0):
                raise ValueError(f"bouncing_shapes: {name} must be a multiple of 4 in [8, 256], got {v}")
        if not 1 <= self.n_shapes <= 4:
            raise ValueError(f"bouncing_shapes: n_shapes must be 1..4, got {self.n_shapes}")
        if not 1 <= self.T <= 1024:
            raise ValueError(f"bouncing_shapes: T must be 1..1024, got {self.T}")


def params_from_env(T=None, size=None):
    """The dataset parameters the environment selects: LFVDM_SHAPES_N, LFVDM_SHAPES_STOCHASTIC, LFVDM_SHAPES_SEED and
    LFVDM_SHAPES_SIZE ("64" or "HxW"; default ``size``, else 64)."""
    env = os.environ
    text = env.get("LFVDM_SHAPES_SIZE") or str(size or 64)
    h, _, w = text.lower().partition("x")
    return ShapesParams(H=int(h), W=int(w or h), n_shapes=int(env.get("LFVDM_SHAPES_N") or 2), T=100 if T is None else int(T),
                        stochastic=(env.get("LFVDM_SHAPES_STOCHASTIC") or "1") != "0", seed=int(env.get("LFVDM_SHAPES_SEED") or 0))


# ------------------------------------------------------------------------------------------------ host reference
def _speed(w):
    return 8 + ((w.astype(np.int64) >> 8) % 41)


def _signed(w):
    s = _speed(w)
    return np.where(w & np.uint32(1), -s, s)


def trajectories_ref(params, split, video_idx, return_events=False):
    """Video indices (N,) -> (traj (N, T, S, 2) int32: x, y in 1/16 pixel;  consts (N, S, 4) int32: kind, radius,
    r | g << 8 | b << 16, 0).  ``return_events``: also bounced (N, T, S, 2) bool - which axis hit a wall at which frame."""
    p = params
    vid = np.asarray(video_idx, dtype=np.int64).reshape(-1)
    if vid.size and (vid.min() < 0 or vid.max() >= 1 << 32):
        raise ValueError("bouncing_shapes: video indices lie in [0, 2^32)")
    N, S, T = len(vid), p.n_shapes, p.T
    k0, k1 = split_seed(p.seed)
    s_ix, v_ix = np.arange(S, dtype=np.int64)[None, :], vid[:, None]
    lmin = min(p.H, p.W)
    r = philox4x32_10(s_ix, v_ix, 0, stream_word(split, INIT), k0, k1)
    kind = (r[0] & np.uint32(1)).astype(np.int64)
    rad = 2 * lmin + (r[0].astype(np.int64) >> 8) % (2 * lmin + 1)
    colour = PALETTE[(r[1].astype(np.int64) >> 8) % 8]                      # (N, S, 3)
    xlo, xhi, ylo, yhi = rad, 16 * p.W - rad, rad, 16 * p.H - rad
    x = rad + r[2].astype(np.int64) % (16 * p.W - 2 * rad + 1)
    y = rad + r[3].astype(np.int64) % (16 * p.H - 2 * rad + 1)
    r = philox4x32_10(s_ix, v_ix, 0, stream_word(split, VELOCITY), k0, k1)
    vx, vy = _signed(r[0]), _signed(r[1])
    traj = np.zeros((N, T, S, 2), dtype=np.int32)
    bounced = np.zeros((N, T, S, 2), dtype=bool)
    traj[:, 0, :, 0], traj[:, 0, :, 1] = x, y

    def move(pos, vel, lo, hi):
        pos = pos + vel
        low, high = pos < lo, pos > hi
        pos = np.where(low, 2 * lo - pos, np.where(high, 2 * hi - pos, pos))
        hit = low | high
        return pos, np.where(hit, -vel, vel), hit

    for t in range(1, T):
        x, vx, bx = move(x, vx, xlo, xhi)
        y, vy, by = move(y, vy, ylo, yhi)
        if p.stochastic and (bx | by).any():
            r = philox4x32_10(s_ix, v_ix, t, stream_word(split, BOUNCE), k0, k1)
            any_hit = bx | by
            vx = np.where(bx, np.where(vx < 0, -_speed(r[0]), _speed(r[0])), np.where(any_hit, _signed(r[2]), vx))
            vy = np.where(by, np.where(vy < 0, -_speed(r[1]), _speed(r[1])), np.where(any_hit, _signed(r[3]), vy))
        traj[:, t, :, 0], traj[:, t, :, 1] = x, y
        bounced[:, t, :, 0], bounced[:, t, :, 1] = bx, by
    consts = np.zeros((N, S, 4), dtype=np.int32)
    consts[..., 0], consts[..., 1] = kind, rad
    consts[..., 2] = colour[..., 0] | (colour[..., 1] << 8) | (colour[..., 2] << 16)
    return (traj, consts, bounced) if return_events else (traj, consts)


def coverage_ref(pos, kind, rad, H, W):
    """Subsample counts k (M, H, W) in 0..16 of one shape at the centres ``pos`` (M, 2)."""
    pos = np.asarray(pos, dtype=np.int64)
    dx = (4 * np.arange(4 * W, dtype=np.int64) + 2)[None, :] - pos[:, 0:1]          # subsample a of a row sits at 4 a + 2
    dy = (4 * np.arange(4 * H, dtype=np.int64) + 2)[None, :] - pos[:, 1:2]
    M = len(pos)
    if kind == KIND_SQUARE:
        nx = (np.abs(dx) <= rad).reshape(M, W, 4).sum(2)
        ny = (np.abs(dy) <= rad).reshape(M, H, 4).sum(2)
        return ny[:, :, None] * nx[:, None, :]
    inside = (dx * dx)[:, None, :] + (dy * dy)[:, :, None] <= rad * rad
    return inside.reshape(M, H, 4, W, 4).sum((2, 4))


def render_ref(pos, consts, H, W):
    """Frames of ONE video: centres ``pos`` (M, S, 2) of its shapes in M frames, ``consts`` (S, 4) -> uint8 (M, 3, H, W)."""
    pos = np.asarray(pos)
    M, S = pos.shape[:2]
    canvas = np.empty((M, 3, H, W), dtype=np.int64)
    for c in range(3):
        canvas[:, c] = BACKGROUND[c]
    for s in range(S):
        kind, rad, rgb = (int(v) for v in consts[s][:3])
        k = coverage_ref(pos[:, s], kind, rad, H, W)
        for c in range(3):
            canvas[:, c] = (canvas[:, c] * (16 - k) + ((rgb >> (8 * c)) & 255) * k + 8) >> 4
    return canvas.astype(np.uint8)


def videos_ref(params, split, video_idx):
    """uint8 (N, T, 3, H, W): the whole videos of the given video indices, host reference."""
    traj, consts = trajectories_ref(params, split, video_idx)
    if not len(traj):
        return np.zeros((0, params.T, 3, params.H, params.W), dtype=np.uint8)
    return np.stack([render_ref(traj[n], consts[n], params.H, params.W) for n in range(len(traj))])


def uint8_to_float(frames_u8):
    """uint8 (..., 3, H, W) tensor -> float32 in [-1, 1], by the function that converts the uint8 frames of every other dataset."""
    shape = frames_u8.shape
    v = frames_u8.reshape(-1, *shape[-3:]).permute(0, 2, 3, 1)
    return _frames_uint8_to_signed_unit(v).reshape(shape)


def float_table():
    """The 256 floats the render kernel looks its float32 output up in: ``uint8_to_float`` of 0..255."""
    return _frames_uint8_to_signed_unit(th.arange(256, dtype=th.uint8).view(256, 1, 1, 1)).reshape(256).contiguous()


# ------------------------------------------------------------------------------------------------ dataset
class BouncingShapes(Dataset):
    """Items are ``(video (T, 3, H, W) float32 in [-1, 1], {})`` from the host reference renderer.  Item ``i`` of shard
    ``shard`` / ``num_shards`` is video ``shard + num_shards * i`` of the split's Philox stream: ranks see disjoint videos,
    the train and test splits disjoint streams."""

    LENGTH = {"train": 65536, "test": 1024}

    def __init__(self, params=None, split="train", shard=0, num_shards=1, length=None):
        if split not in SPLITS:
            raise ValueError(f"bouncing_shapes: split must be 'train' or 'test', got {split!r}")
        self.params = params or ShapesParams()
        self.split, self.shard, self.num_shards = split, int(shard), int(num_shards)
        self.T = self.params.T
        self.length = (self.LENGTH[split] // self.num_shards) if length is None else int(length)
        self.is_test = False

    def set_test(self):
        self.is_test = True           # items are deterministic either way: the first T frames ARE the video

    def __len__(self):
        return self.length

    def video_indices(self, items):
        """Dataset item indices -> video indices of the split's stream (int64 array)."""
        items = np.asarray(items, dtype=np.int64)
        if items.size and (items.min() < 0 or items.max() >= self.length):
            raise IndexError("bouncing_shapes: item index out of range")
        return self.shard + self.num_shards * items

    def videos_uint8(self, items):
        return th.from_numpy(videos_ref(self.params, self.split, self.video_indices(np.asarray(items).reshape(-1))))

    def __getitem__(self, idx):
        return uint8_to_float(self.videos_uint8([int(idx)])[0]), {}


class ShapesDeviceSource:
    """What lets a consumer render the batches of a ``ShapesBatches`` iterator on the device instead of taking them from the
    host: ``next_indices()`` hands out the dataset items of the next batch (the iterator's own ``__next__`` draws from the same
    sequence), ``render`` / ``render_batch`` produce their frames with the two kernels, bit for bit what the host items hold."""

    def __init__(self, dataset, batch_size, deterministic=False):
        if batch_size > len(dataset):
            raise ValueError("bouncing_shapes: batch_size exceeds the dataset")
        self.dataset, self.batch_size, self.deterministic = dataset, int(batch_size), bool(deterministic)
        self._epoch, self._order, self._at = 0, None, 0
        self._lut = {}

    def next_indices(self):
        """int64 (batch_size,) dataset items of the next batch; epochs are seeded permutations (whole batches only)."""
        n, B = len(self.dataset), self.batch_size
        if self._order is None or self._at + B > n:
            if self.deterministic:
                self._order = np.arange(n, dtype=np.int64)
            else:
                seed = (self.dataset.params.seed * 1_000_003 + 7919 * self._epoch + self.dataset.shard) % (1 << 32)
                self._order = np.random.RandomState(seed).permutation(n).astype(np.int64)
            self._epoch, self._at = self._epoch + 1, 0
        out = self._order[self._at:self._at + B]
        self._at += B
        return th.from_numpy(out.copy())

    # -- device side
    def lut(self, device):
        device = th.device(device)
        if device not in self._lut:
            self._lut[device] = float_table().to(device)
        return self._lut[device]

    def trajectories(self, video_idx):
        """Device int64 VIDEO indices (N,) -> (traj (N, T, S, 2), consts (N, S, 4)) int32 on that device.  Capturable."""
        from . import _native as nat
        p, N = self.dataset.params, video_idx.numel()
        traj = th.empty(N, p.T, p.n_shapes, 2, device=video_idx.device, dtype=th.int32)
        consts = th.empty(N, p.n_shapes, 4, device=video_idx.device, dtype=th.int32)
        nat.shapes_trajectories(video_idx.reshape(-1), traj, consts, p.seed, SPLITS[self.dataset.split], p.stochastic, p.H, p.W)
        return traj, consts

    def _video_idx(self, items, device):
        items = items.cpu().numpy() if isinstance(items, th.Tensor) else items
        return th.from_numpy(self.dataset.video_indices(items)).to(device)

    def render(self, indices, device, dtype=th.float32):
        """Whole videos of the dataset items ``indices`` -> (N, T, 3, H, W) ``dtype`` (float32 / uint8) on ``device``."""
        from . import _native as nat
        p = self.dataset.params
        vid = self._video_idx(indices, device).reshape(-1)
        traj, consts = self.trajectories(vid)
        out = th.empty(vid.numel(), p.T, 3, p.H, p.W, device=device, dtype=dtype)
        nat.shapes_render(traj, consts, out, lut=self.lut(device) if dtype == th.float32 else None)
        return out

    def render_table(self, video_idx, table, dtype=th.float32, masks=True):
        """The capturable core of ``render_batch``: device VIDEO indices (B, 2) [video 1, padding video] and the device index
        table (B, F, 4) -> (batch (B, F, 3, H, W), frame_indices, obs_mask, latent_mask); the last three None without ``masks``."""
        from . import _native as nat
        p, dev = self.dataset.params, table.device
        B, F = table.shape[:2]
        traj, consts = self.trajectories(video_idx.reshape(-1))
        batch = th.empty(B, F, 3, p.H, p.W, device=dev, dtype=dtype)
        fi = obs = lat = None
        if masks:
            fi = th.empty(B, F, device=dev, dtype=th.int64)
            obs = th.empty(B, F, 1, 1, 1, device=dev, dtype=th.float32)
            lat = th.empty_like(obs)
        nat.shapes_render(traj, consts, batch, table=table, lut=self.lut(dev) if dtype == th.float32 else None,
                          frame_indices=fi, obs_mask=obs, latent_mask=lat)
        return batch, fi, obs, lat

    def render_batch(self, indices1, indices2, table, device, dtype=th.float32):
        """The training micro-batch the index table names (``TrainLoop.sample_index_table``: rows < T are frames of the videos
        ``indices1``, rows >= T frames of the padding videos ``indices2``), rendered in one launch pair."""
        v = th.stack([self._video_idx(indices1, device).reshape(-1), self._video_idx(indices2, device).reshape(-1)], dim=1)
        table = th.as_tensor(table, dtype=th.int32).to(device).contiguous()
        return self.render_table(v.contiguous(), table, dtype)


class ShapesBatches:
    """Endless iterator of host batches ``(video (B, T, 3, H, W) float32, {})`` - what ``load_data`` returns for this dataset.
    It carries ``device_source``: a consumer that can render takes ``device_source.next_indices()`` INSTEAD of ``next()`` and
    gets the same sequence of batches without the host rendering them."""

    def __init__(self, dataset, batch_size, deterministic=False):
        self.dataset = dataset
        self.device_source = ShapesDeviceSource(dataset, batch_size, deterministic)

    def __iter__(self):
        return self

    def __next__(self):
        items = self.device_source.next_indices()
        return uint8_to_float(self.dataset.videos_uint8(items.numpy())), {}


def open_dataset(T, split, shard, num_shards, size=None):
    return BouncingShapes(params_from_env(T, size), split, shard, num_shards)


# ------------------------------------------------------------------------------------------------ command line
def main(argv=None):
    ap = argparse.ArgumentParser(description="Write bouncing_shapes videos (N, T, 3, H, W) to a .npy file.")
    ap.add_argument("--out", required=True)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--T", type=int, default=None)
    ap.add_argument("--split", choices=sorted(SPLITS), default="train")
    ap.add_argument("--first", type=int, default=0, help="first dataset item")
    ap.add_argument("--uint8", action="store_true", help="uint8 0..255 instead of float32 in [-1, 1]")
    ap.add_argument("--host", action="store_true", help="use the host reference even when a GPU is present")
    a = ap.parse_args(argv)
    ds = open_dataset(a.T, a.split, 0, 1)
    items = np.arange(a.first, a.first + a.n)
    dtype = th.uint8 if a.uint8 else th.float32
    if th.cuda.is_available() and not a.host:
        videos = ShapesDeviceSource(ds, 1).render(items, th.device("cuda"), dtype).cpu()
    else:
        videos = ds.videos_uint8(items)
        videos = videos if a.uint8 else uint8_to_float(videos)
    np.save(a.out, videos.numpy())
    print(f"{a.out}: {tuple(videos.shape)} {videos.dtype} ({a.split} items {a.first}..{a.first + a.n - 1})")


if __name__ == "__main__":
    main()
