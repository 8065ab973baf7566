"""Video prediction metrics on the MI355X (csrc/video_metrics.hip through the C ABI and through frame_metrics /
prediction_metrics): against the float64 yardstick of test_video_metrics_cpu.py on the smallest shapes that can go wrong (one
tile, one valid position, tiles straddled with rows that are no multiple of 4 pixels and K > 1, the workload's frame size, 2 x 2
tiles with one-position strips), float32 in [-1, 1] and uint8, three noise levels and a flat half; identical inputs; bitwise
reproducibility from launch to launch and from sample to sample; the truth not replicated; scalar against 16-byte loads;
the CPU path against the device path; the best-of-K choice on both.

Bounds as in test_video_metrics_cpu.py: against the float64 yardstick at max(floor, 3 x the float32 yardstick's deviation in
that case), floors 1e-4 relative (mse) and 1e-5 absolute (ssim).  Every comparison prints error / bound."""
import pytest
import torch

from test_video_metrics_cpu import DTYPES, SHAPES, compare, make_case, planted_case, reference

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _launch(pred, truth, K, lo, hi):
    """lfvdm_frame_metrics through the binding, outputs and workspace pre-filled with NaN.  pred (K, ..., C, H, W)."""
    from improved_diffusion import _native as nat
    C, H, W = pred.shape[-3:]
    N = pred.numel() // (K * C * H * W)
    need = nat.frame_metrics_workspace(K, N, C, H, W)
    mse, ssim = (torch.full((K, N), NAN, device="cuda") for _ in range(2))
    ws = torch.full((need,), NAN, device="cuda")
    nat.frame_metrics(pred, truth, 1.0 / (hi - lo), -lo / (hi - lo), K, N, C, H, W, mse, ssim, ws)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws).all()), "every slot of the workspace is written"
    return mse, ssim


def _off(x, nbytes):
    """a contiguous copy of ``x`` that starts ``nbytes`` past a 16-byte boundary"""
    n = nbytes // x.element_size()
    buf = torch.zeros(x.numel() + n, device=x.device, dtype=x.dtype)
    v = buf[n:].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == nbytes
    return v


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_the_float64_yardstick(shape, dtype):
    from improved_diffusion.video_metrics import frame_metrics
    pred, truth, (lo, hi) = make_case(shape, dtype)
    m64, s64, bnd = reference(shape, dtype)
    K = shape[0]
    p, t = pred.cuda(), truth.cuda()
    assert t.numel() * K == p.numel()
    mse, ssim = _launch(p, t, K, lo, hi)
    compare(f"C ABI {shape} {dtype}", {"mse": mse.view(shape[:3]), "ssim": ssim.view(shape[:3])}, m64, s64, bnd)
    got = frame_metrics(p, t)
    assert got["mse"].is_cuda and got["mse"].shape == shape[:3]
    assert torch.equal(got["mse"].flatten(), mse.flatten()) and torch.equal(got["ssim"].flatten(), ssim.flatten())
    assert torch.equal(got["psnr"], -10 * torch.log10(got["mse"]))
    # the CPU path and the device path agree within the same bounds
    cpu = frame_metrics(pred, truth)
    em = float((got["mse"].cpu().double() / cpu["mse"].double() - 1).abs().max())
    es = float((got["ssim"].cpu().double() - cpu["ssim"].double()).abs().max())
    print(f"[video metrics cpu vs device {shape} {dtype}] mse {em:.2e} ({em / bnd[0]:.3f} of bound)  ssim {es:.2e} ({es / bnd[1]:.3f} of bound)")
    assert em <= bnd[0] and es <= bnd[1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_identical_inputs(dtype):
    from improved_diffusion.video_metrics import frame_metrics
    for shape in (SHAPES[2], SHAPES[3]):
        pred = make_case(shape, dtype)[0].cuda()
        got = frame_metrics(pred, pred.clone())
        print(f"[video metrics identical {shape} {dtype}] max |ssim - 1| = {float((got['ssim'] - 1).abs().max()):.2e}")
        assert float((got["ssim"] - 1).abs().max()) <= 1e-6
        assert float(got["mse"].abs().max()) == 0.0 and bool(torch.isinf(got["psnr"]).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_bitwise_reproducible_and_the_same_for_every_sample(dtype):
    shape = SHAPES[2]
    pred, truth, (lo, hi) = make_case(shape, dtype)
    p, t = pred.cuda(), truth.cuda()
    a, b = _launch(p, t, 2, lo, hi), _launch(p, t, 2, lo, hi)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # a K-axis stack of one sample against a truth of exactly N C H W elements: every k gives the bits of K = 1
    one = p[1].contiguous()
    stack = torch.stack([one, one, one])
    assert t.numel() == one.numel() and t.untyped_storage().nbytes() == t.numel() * t.element_size()
    m3, s3 = _launch(stack, t, 3, lo, hi)
    m1, s1 = _launch(one, t, 1, lo, hi)
    for k in range(3):
        assert torch.equal(m3[k], m1[0]) and torch.equal(s3[k], s1[0]), k
    assert torch.equal(m1[0], a[0][1]) and torch.equal(s1[0], a[1][1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_misaligned_pointers_take_the_scalar_loads(dtype):
    """64-pixel rows allow 16-byte loads; the same data one element past a 16-byte boundary does not.  Both stage the same
    values, so ssim has the same bits; mse is summed in another order and stays within its bound."""
    shape = SHAPES[3]
    pred, truth, (lo, hi) = make_case(shape, dtype)
    m64, s64, bnd = reference(shape, dtype)
    p, t = pred.cuda(), truth.cuda()
    step = p.element_size()
    mv, sv = _launch(p, t, 1, lo, hi)
    for po, to in ((step, 0), (0, step), (step, step)):
        ms, ss = _launch(_off(p, po), _off(t, to), 1, lo, hi)
        assert torch.equal(ss, sv), (po, to)
        compare(f"offset {po}/{to} {dtype}", {"mse": ms.view(shape[:3]), "ssim": ss.view(shape[:3])}, m64, s64, bnd)


def test_prediction_metrics_chooses_as_on_the_cpu():
    from improved_diffusion.video_metrics import prediction_metrics
    samples, truth, plant = planted_case()
    for dt in (torch.float32, torch.uint8):
        s, t = samples, truth
        if dt == torch.uint8:
            s, t = ((127.5 * (v + 1)).round().to(torch.uint8) for v in (samples, truth))
        for best_of in ("ssim", "psnr"):
            cpu = prediction_metrics(s, t, 2, best_of=best_of)
            dev = prediction_metrics(s.cuda(), t.cuda(), 2, best_of=best_of)
            assert torch.equal(dev["best_index"].cpu(), cpu["best_index"]) and torch.equal(cpu["best_index"], plant)
            for k, v in cpu.items():
                if torch.is_tensor(v) and v.is_floating_point():
                    assert dev[k].shape == (3,) and torch.allclose(dev[k].cpu(), v, rtol=2e-4, atol=2e-5), k
