"""The bouncing_shapes dataset without a GPU: the module's Philox against the oracle's, determinism and disjointness, the
bounce code against the closed-form triangle wave, the coverage against the shapes' areas, the float output against the
uint8 -> float conversion of the other datasets, the dataset / loader surface, the exports and the host-side refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import philox_ref
from improved_diffusion import shapes as sh
from improved_diffusion import video_datasets as vd

NEW_EXPORTS = ("lfvdm_shapes_trajectories", "lfvdm_shapes_render")


def test_philox_equals_the_oracle_word_for_word():
    rng = np.random.RandomState(0)
    c = rng.randint(0, 1 << 32, size=(4, 257), dtype=np.uint64)
    for seed in (0, 1, 0xDEADBEEF12345678, (1 << 64) - 1):
        k0, k1 = sh.split_seed(seed)
        assert (k0, k1) == philox_ref.split_seed(seed)
        for a, b in zip(sh.philox4x32_10(*c, k0, k1), philox_ref.philox4x32_10(*c, k0, k1)):
            assert a.dtype == np.uint32 and np.array_equal(a, b)
    # the counters the dataset uses: (shape, video, frame, stream word)
    s, v = np.arange(4)[None, :], np.array([0, 1, 65535, (1 << 32) - 1])[:, None]
    for split in ("train", "test"):
        for purpose, frame in ((sh.INIT, 0), (sh.VELOCITY, 0), (sh.BOUNCE, 1023)):
            w = sh.stream_word(split, purpose)
            for a, b in zip(sh.philox4x32_10(s, v, frame, w, 7, 9), philox_ref.philox4x32_10(s, v, frame, w, 7, 9)):
                assert np.array_equal(a, b)
    assert len({sh.stream_word(sp, pu) for sp in sh.SPLITS for pu in (sh.INIT, sh.VELOCITY, sh.BOUNCE)}) == 6


def test_same_key_same_bytes_and_everything_else_differs():
    p = sh.ShapesParams(H=16, W=16, T=12, seed=5)
    a = sh.videos_ref(p, "train", [3])
    assert a.shape == (1, 12, 3, 16, 16) and a.dtype == np.uint8
    assert np.array_equal(a, sh.videos_ref(p, "train", [3]))
    assert not np.array_equal(a, sh.videos_ref(p, "test", [3]))
    assert not np.array_equal(a, sh.videos_ref(p, "train", [4]))
    assert not np.array_equal(a, sh.videos_ref(sh.ShapesParams(H=16, W=16, T=12, seed=6), "train", [3]))
    r0, r1 = sh.BouncingShapes(p, "train", 0, 2), sh.BouncingShapes(p, "train", 1, 2)
    assert len(r0) == len(r1) == sh.BouncingShapes.LENGTH["train"] // 2
    assert not set(r0.video_indices(np.arange(64)).tolist()) & set(r1.video_indices(np.arange(64)).tolist())
    assert not torch.equal(r0[3][0], r1[3][0])
    assert torch.equal(r0[3][0], sh.BouncingShapes(p, "train", 0, 2)[3][0])
    assert any(frame.any() for frame in a[0]) and tuple(sh.BACKGROUND) not in {tuple(c) for c in sh.PALETTE.tolist()}


@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("hw", [(8, 8), (16, 24), (64, 64), (256, 8)])
def test_centres_stay_inside_the_walls(hw, stochastic):
    p = sh.ShapesParams(H=hw[0], W=hw[1], n_shapes=4, T=200, stochastic=stochastic, seed=11)
    traj, consts = sh.trajectories_ref(p, "train", np.arange(16))
    rad = consts[..., 1][:, None, :]
    lmin = min(hw)
    assert (rad >= 2 * lmin).all() and (rad <= 4 * lmin).all() and set(np.unique(consts[..., 0])) <= {0, 1}
    assert (traj[..., 0] >= rad).all() and (traj[..., 0] <= 16 * p.W - rad).all()
    assert (traj[..., 1] >= rad).all() and (traj[..., 1] <= 16 * p.H - rad).all()
    speed = np.abs(np.diff(traj.astype(np.int64), axis=1))
    assert speed.max() <= 48                                   # at most 3 pixels per frame (less across a reflection)


def test_deterministic_motion_is_the_triangle_wave():
    """stochastic=False: x_t is p0 + v t folded into [lo, hi] - an independent closed form of the sequential bounce code."""
    p = sh.ShapesParams(H=16, W=24, n_shapes=4, T=300, stochastic=False, seed=2)
    traj, consts, bounced = sh.trajectories_ref(p, "test", np.arange(8), return_events=True)
    assert bounced.any(axis=(0, 1, 2)).all()
    t = np.arange(p.T, dtype=np.int64)[None, :, None]
    for axis, L in ((0, p.W), (1, p.H)):
        pos = traj[..., axis].astype(np.int64)
        lo = consts[..., 1].astype(np.int64)[:, None, :]
        span = 16 * L - 2 * lo
        v = pos[:, 1:2] - pos[:, 0:1]                           # the velocity, where the first step hit no wall
        free = ~bounced[:, 1, :, axis]
        u = np.mod(pos[:, 0:1] - lo + v * t, 2 * span)
        want = lo + np.where(u <= span, u, 2 * span - u)
        assert free.any()
        sel = np.broadcast_to(free[:, None, :], pos.shape)
        assert np.array_equal(pos[sel], want[sel])


@pytest.mark.parametrize("kind", [sh.KIND_DISC, sh.KIND_SQUARE])
def test_coverage_sums_to_the_area_within_the_perimeter_bound(kind):
    """sum k / 16 against the area of a fully interior shape.  Only pixels the boundary passes through can be wrong, each by
    less than one pixel; a convex curve crosses at most 2 (ceil(w) + ceil(h)) + 4 pixels of its w x h bounding box - the
    perimeter of the square itself, 4 / pi times that of the disc."""
    H = W = 64
    rng = np.random.RandomState(3)
    for _ in range(8):
        rad = int(rng.randint(2 * H, 4 * H + 1))
        pos = np.array([[rng.randint(rad, 16 * W - rad + 1), rng.randint(rad, 16 * H - rad + 1)]])
        k = sh.coverage_ref(pos, kind, rad, H, W)[0]
        assert k.min() >= 0 and k.max() == 16
        r_px = rad / 16.0
        area = (2 * r_px) ** 2 if kind == sh.KIND_SQUARE else np.pi * r_px ** 2
        bound = 4 * np.ceil(2 * r_px) + 4
        assert abs(k.sum() / 16.0 - area) <= bound, (k.sum() / 16.0, area, bound)
        # and the rendered frame shows exactly this coverage in the shape's colour
        consts = np.array([[kind, rad, 200 | (100 << 8) | (50 << 16), 0]], dtype=np.int32)
        frame = sh.render_ref(pos[None], consts, H, W)[0]
        for c, col in enumerate((200, 100, 50)):
            assert np.array_equal(frame[c], (col * k + 8) >> 4)


def test_painters_order_blends_over_the_previous_shape():
    pos = np.array([[[256, 256], [300, 260]]])
    consts = np.array([[0, 128, 255, 0], [1, 96, 255 << 8, 0]], dtype=np.int32)
    both = sh.render_ref(pos, consts, 32, 32)[0].astype(np.int64)
    first = sh.render_ref(pos[:, :1], consts[:1], 32, 32)[0].astype(np.int64)
    k1 = sh.coverage_ref(pos[0, 1:2], 1, 96, 32, 32)[0]
    assert ((k1 > 0) & (first[0] > 0)).any()                    # they overlap
    assert np.array_equal(both[0], (first[0] * (16 - k1) + 8) >> 4) and np.array_equal(both[1], (255 * k1 + 8) >> 4)


def test_float_output_is_the_uint8_conversion_of_the_other_datasets():
    ds = sh.BouncingShapes(sh.ShapesParams(H=16, W=24, T=9, n_shapes=3, seed=1), "train")
    u8 = ds.videos_uint8([5])[0]
    video, extra = ds[5]
    assert extra == {} and video.dtype == torch.float32 and video.shape == (9, 3, 16, 24)
    assert torch.equal(video, vd._frames_uint8_to_signed_unit(u8.permute(0, 2, 3, 1)))
    lut = sh.float_table()
    assert lut.shape == (256,) and float(lut[0]) == -1.0 and float(lut[255]) == 1.0
    assert torch.equal(video, lut[u8.long()])                   # what the kernel's table lookup gives


def test_dataset_and_loader_surface(monkeypatch):
    for k in ("LFVDM_SHAPES_N", "LFVDM_SHAPES_STOCHASTIC", "LFVDM_SHAPES_SEED", "LFVDM_SHAPES_SIZE"):
        monkeypatch.delenv(k, raising=False)
    assert vd.default_T_dict["bouncing_shapes"] == 100 and vd.default_image_size_dict["bouncing_shapes"] == 64
    test = vd.get_test_dataset("bouncing_shapes", T=7)
    assert test.is_test and test.split == "test" and len(test) == 1024
    assert test.params == sh.ShapesParams(H=64, W=64, n_shapes=2, T=7, stochastic=True, seed=0)
    video, extra = test[0]
    assert video.shape == (7, 3, 64, 64) and video.dtype == torch.float32 and extra == {}
    assert float(video.min()) >= -1.0 and float(video.max()) <= 1.0
    assert vd.get_train_dataset("bouncing_shapes").T == 100
    monkeypatch.setenv("LFVDM_SHAPES_SIZE", "16x24")
    monkeypatch.setenv("LFVDM_SHAPES_N", "3")
    monkeypatch.setenv("LFVDM_SHAPES_STOCHASTIC", "0")
    monkeypatch.setenv("LFVDM_SHAPES_SEED", "9")
    data = vd.load_data("bouncing_shapes", batch_size=2, T=6, num_workers=0)
    assert data.dataset.params == sh.ShapesParams(H=16, W=24, n_shapes=3, T=6, stochastic=False, seed=9)
    batch, extra = next(data)
    assert batch.shape == (2, 6, 3, 16, 24) and batch.dtype == torch.float32 and extra == {}
    assert next(vd.load_data("bouncing_shapes", batch_size=2, T=6, return_dataset=True)).params == data.dataset.params
    monkeypatch.setenv("LFVDM_SHAPES_SIZE", "18")
    with pytest.raises(ValueError, match="multiple of 4"):
        vd.get_train_dataset("bouncing_shapes")


def test_host_batches_are_the_items_the_device_source_reports():
    p = sh.ShapesParams(H=16, W=16, T=5, seed=4)
    a = sh.ShapesBatches(sh.BouncingShapes(p, "train", 1, 2, length=7), batch_size=3)
    b = sh.ShapesBatches(sh.BouncingShapes(p, "train", 1, 2, length=7), batch_size=3)
    seen = []
    for _ in range(5):                                          # crosses two epoch boundaries (whole batches only)
        items = b.device_source.next_indices()
        assert items.dtype == torch.int64 and items.shape == (3,)
        batch, _ = next(a)
        assert torch.equal(batch, torch.stack([b.dataset[int(i)][0] for i in items]))
        seen.append(items.tolist())
    assert len(set(seen[0] + seen[1])) == 6 and len(set(seen[2] + seen[3])) == 6      # an epoch shows no item twice
    assert seen[0] + seen[1] != seen[2] + seen[3]                                       # and epochs are shuffled afresh
    det = sh.ShapesBatches(sh.BouncingShapes(p, "train", length=7), batch_size=3, deterministic=True).device_source
    assert [det.next_indices().tolist() for _ in range(3)] == [[0, 1, 2], [3, 4, 5], [0, 1, 2]]


def test_cli_writes_the_reference_bytes(tmp_path, monkeypatch):
    for k in ("LFVDM_SHAPES_N", "LFVDM_SHAPES_STOCHASTIC", "LFVDM_SHAPES_SEED"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LFVDM_SHAPES_SIZE", "16")
    out = tmp_path / "v.npy"
    sh.main(["--out", str(out), "--n", "2", "--T", "4", "--split", "test", "--uint8", "--host"])
    got = np.load(out)
    assert got.dtype == np.uint8 and np.array_equal(got, sh.videos_ref(sh.ShapesParams(H=16, W=16, T=4), "test", [0, 1]))


def test_exports_in_header_binding_and_library():
    from improved_diffusion import _native as nat
    with open(os.path.join(ROOT, "include", "lfvdm_hip.h")) as f:
        header = f.read()
    L = nat.lib()
    for name in NEW_EXPORTS:
        assert name in nat._SIGS and name in nat.EXPORTS and hasattr(L, name), name
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(nat._SIGS[name][0]), name      # one ctypes entry per C parameter
    assert L.lfvdm_abi_version() == 9                           # additive: the version stays
    for knob in ("LFVDM_SHAPES_N", "LFVDM_SHAPES_STOCHASTIC", "LFVDM_SHAPES_SEED", "LFVDM_SHAPES_SIZE"):
        assert knob in header
    assert os.path.exists(os.path.join(ROOT, "latent-flexible-video-diffusion-modeling_amd", "csrc", "shapes.hip"))


def test_every_refusal_happens_on_the_host():
    """Stand-in pointers and no device: a refused call launches nothing and reads none of them."""
    from improved_diffusion import _native as nat
    L = nat.lib()
    host = (ctypes.c_float * 8)()
    p = ctypes.addressof(host)
    p -= p % 16                                                 # never dereferenced: only its alignment is looked at

    def traj(**kw):
        a = dict(video_idx=p, traj=p, consts=p, seed=1, split=0, n_videos=2, T=8, n_shapes=2, H=16, W=16, stochastic=1)
        a.update(kw)
        return L.lfvdm_shapes_trajectories(a["video_idx"], a["traj"], a["consts"], a["seed"], a["split"], a["n_videos"], a["T"],
                                           a["n_shapes"], a["H"], a["W"], a["stochastic"], None)

    def render(**kw):
        a = dict(traj=p, consts=p, table=p, lut=p, out=p, dtype=nat.PIX_F32, fi=p, obs=p, lat=p, B=2, F=4, Tp=16, T=8, n_shapes=2,
                 H=16, W=16)
        a.update(kw)
        return L.lfvdm_shapes_render(a["traj"], a["consts"], a["table"], a["lut"], a["out"], a["dtype"], a["fi"], a["obs"], a["lat"],
                                     a["B"], a["F"], a["Tp"], a["T"], a["n_shapes"], a["H"], a["W"], None)

    refused = {
        **{f"trajectories: no {k}": traj(**{k: None}) for k in ("video_idx", "traj", "consts")},
        "trajectories: H % 4": traj(H=18), "trajectories: W % 4": traj(W=18), "trajectories: H < 8": traj(H=4),
        "trajectories: W > 256": traj(W=260), "trajectories: H > 256": traj(H=260), "trajectories: n_shapes 0": traj(n_shapes=0),
        "trajectories: n_shapes 5": traj(n_shapes=5), "trajectories: T 0": traj(T=0), "trajectories: T 1025": traj(T=1025),
        "trajectories: no videos": traj(n_videos=0), "trajectories: split": traj(split=2), "trajectories: traj % 8": traj(traj=p + 4),
        **{f"render: no {k}": render(**{k: None}) for k in ("traj", "consts", "out", "lut")},
        "render: one mask missing": render(obs=None), "render: masks without a table": render(table=None, F=4),
        "render: H % 4": render(H=18), "render: W % 4": render(W=18), "render: W < 8": render(W=4), "render: H > 256": render(H=260),
        "render: n_shapes 0": render(n_shapes=0), "render: n_shapes 5": render(n_shapes=5), "render: T 0": render(T=0),
        "render: T 1025": render(T=1025, Tp=1025), "render: B 0": render(B=0), "render: B > 65535": render(B=65536),
        "render: F 0": render(F=0), "render: Tp % T": render(Tp=12), "render: Tp < T": render(Tp=4), "render: Tp = 3 T": render(Tp=24),
        "render: whole videos, F > Tp": render(table=None, fi=None, obs=None, lat=None, F=17),
        "render: out % 16 (float32)": render(out=p + 4), "render: out % 4 (uint8)": render(out=p + 2, dtype=nat.PIX_U8),
        "render: dtype": render(dtype=2),
    }
    for what, rc in refused.items():
        assert rc != 0, what
    assert refused["render: dtype"] == 3 and refused["render: H % 4"] == 1
