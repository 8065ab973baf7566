"""csrc/wavelet.hip on the MI355X, through the C ABI with NaN-filled outputs, against the float64 yardstick of
test_wavelet_cpu.py: one block, odd half-width (scalar path), the vector paths of both levels, quarter-width 3, a base pointer
one element off; float32 and uint8 pixels, with and without per-channel statistics, both norms.

Encode bound (derived, not measured): |err| <= 8 L 2^-24 M, M the largest |float64 coefficient| before the affine - three
roundings per level at half an ulp of a value of at most M, with a factor of about 2.7 of slack - plus 2^-23 |y| where the
statistics apply (the subtraction, the product and the float32 reciprocal of std: 3 x 2^-25 |y|).  The yardstick reads the
pixels as the kernel is told to, value = float32(1 / 127.5) raw - 1 for uint8, and the float32 statistics the kernel is given.

Decode bound: against the float64 inverse of the very coefficients the kernel read, |err| <= (8 L 2^-24 + [stats] L 2^-23) Q,
Q the largest |value| among the de-standardised coefficients and the pixels: per level the butterfly is two half-ulps of
sums <= 2 Q and one of a sum <= 4 Q (4 x 2^-24 Q in all, at k = 1), and the one rounding of fma(y, std, mean), 2^-25 Q, enters
four times.

Bitwise checks: uint8 -> encode -> decode to uint8 is the identity for all 256 values at every position of a block; the encode
is reproducible; the vector and the scalar path give the same bits; lfvdm_prepare_batch_wavelet is lfvdm_prepare_batch followed
by lfvdm_wavelet_encode, corrupt table rows included; bad shapes return their code and touch nothing."""
import pytest
import torch

from test_wavelet_cpu import SHAPES, make_pixels, make_stats, to_unit64, yardstick

pytestmark = pytest.mark.gpu

NAN = float("nan")
DTYPES = [torch.float32, torch.uint8]
E_SHAPE, E_UNSUPPORTED = 1, 3


def _stats32(channels):
    """float32 statistics (what the kernel is given) -> (for the yardstick, mean, rstd, std on the device)"""
    from improved_diffusion.wavelet import _rstd
    st = {k: v.float() for k, v in make_stats(channels).items()}
    return st, st["mean"].cuda(), _rstd(st["std"]).cuda(), st["std"].cuda()


def _off(x, n):
    """a contiguous device copy of ``x`` that starts ``n`` elements past a 256-byte boundary"""
    buf = torch.zeros(x.numel() + n, device="cuda", dtype=x.dtype)
    v = buf[n:].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 256 == n * x.element_size()
    return v


def _encode(x, L, norm, mean=None, rstd=None):
    from improved_diffusion import _native as nat
    N, C, H, W = x.shape
    y = torch.full((N, C * 4 ** L, H >> L, W >> L), NAN, device="cuda")
    nat.wavelet_encode(x, y, L, norm, mean, rstd)
    torch.cuda.synchronize()
    return y


def _decode(y, L, norm, dtype, mean=None, std=None, offset=0):
    from improved_diffusion import _native as nat
    N, K, Ho, Wo = y.shape
    shape = (N, K >> (2 * L), Ho << L, Wo << L)
    x = torch.full(shape, NAN, device="cuda") if dtype == torch.float32 else torch.full(shape, 77, device="cuda", dtype=dtype)
    if offset:
        x = _off(x, offset)
    nat.wavelet_decode(y, x, L, norm, mean, std)
    torch.cuda.synchronize()
    return x


def _check_case(tag, x_dev, x_cpu, L, norm, with_stats):
    """encode against the yardstick, decode against the float64 inverse of the kernel's own coefficients"""
    from improved_diffusion.wavelet import wavelet_decode
    C = x_cpu.shape[1]
    st, mean, rstd, std = _stats32(C * 4 ** L) if with_stats else (None, None, None, None)
    want, raw = yardstick(to_unit64(x_cpu), L, norm, st)
    got = _encode(x_dev, L, norm, mean, rstd)
    assert got.shape == want.shape
    M = float(raw.abs().max())
    bound = 8 * L * 2.0 ** -24 * M + (2.0 ** -23 * want.abs() if with_stats else 0.0)
    err = (got.cpu().double() - want).abs()
    print(f"[wavelet encode {tag} L={L} {norm} stats={with_stats}] max err {float(err.max()):.2e}  M {M:.3f}  "
          f"worst err / bound {float((err / bound).max()):.3f}")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())
    # decode: float32 pixels against the float64 inverse of `got`; uint8 pixels of uint8 input exactly
    back = _decode(got, L, norm, torch.float32, mean, std)
    inv = wavelet_decode(got.cpu().double(), L, norm, st)
    destd = got.cpu().double() if st is None else got.cpu().double() * st["std"].double().view(1, -1, 1, 1) + st["mean"].double().view(1, -1, 1, 1)
    Q = max(float(destd.abs().max()), float(inv.abs().max()))
    dbound = (8 * L * 2.0 ** -24 + (L * 2.0 ** -23 if with_stats else 0.0)) * Q
    derr = float((back.cpu().double() - inv).abs().max())
    print(f"[wavelet decode {tag} L={L} {norm} stats={with_stats}] max err {derr:.2e}  Q {Q:.3f}  err / bound {derr / dbound:.3f}")
    assert bool(torch.isfinite(back).all()) and derr <= dbound
    if x_cpu.dtype == torch.uint8:
        assert torch.equal(_decode(got, L, norm, torch.uint8, mean, std).cpu(), x_cpu)
    return got


@pytest.mark.parametrize("norm", ["range", "orthonormal"])
@pytest.mark.parametrize("with_stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_match_the_float64_yardstick(shape, dtype, with_stats, norm):
    N, C, H, W, L = shape
    x = make_pixels((N, C, H, W), dtype)
    got = _check_case(f"{shape} {dtype}", x.cuda(), x, L, norm, with_stats)
    # the public entry takes the same launch
    from improved_diffusion.wavelet import wavelet_decode, wavelet_encode
    st = _stats32(C * 4 ** L)[0] if with_stats else None
    pub = wavelet_encode(x.cuda(), L, norm, st)
    assert pub.is_cuda and torch.equal(pub, got)
    assert torch.equal(wavelet_decode(pub.view((1,) + pub.shape), L, norm, st)[0], _decode(got, L, norm, torch.float32,
                       *(_stats32(C * 4 ** L)[1::2] if with_stats else ())))


@pytest.mark.parametrize("norm", ["range", "orthonormal"])
@pytest.mark.parametrize("with_stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8"])
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4]], ids=lambda s: "x".join(map(str, s)))
def test_misaligned_base_takes_the_scalar_path_with_the_same_bits(shape, dtype, with_stats, norm):
    """A view that starts one element past an aligned address: the vector path cannot take it, nothing is refused, and the
    result has the bits of the aligned launch."""
    N, C, H, W, L = shape
    x = make_pixels((N, C, H, W), dtype)
    aligned = _check_case(f"{shape} {dtype} aligned", x.cuda(), x, L, norm, with_stats)
    shifted = _check_case(f"{shape} {dtype} +1 element", _off(x, 1), x, L, norm, with_stats)
    assert torch.equal(aligned, shifted)
    st, mean, rstd, std = _stats32(C * 4 ** L) if with_stats else (None, None, None, None)
    a = _decode(aligned, L, norm, dtype, mean, std)
    b = _decode(aligned, L, norm, dtype, mean, std, offset=1)
    assert torch.equal(a, b)


@pytest.mark.parametrize("norm", ["range", "orthonormal"])
@pytest.mark.parametrize("with_stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("L", [1, 2])
def test_uint8_round_trip_is_the_identity_for_every_value_at_every_block_position(L, with_stats, norm):
    m = 1 << L
    g = torch.Generator().manual_seed(11 + L)
    x = torch.randint(0, 256, (m * m, 2, m, 256 * m), generator=g, dtype=torch.uint8)
    for p in range(m * m):      # frame p: value v at position p of block v, for all 256 values (channel 1: descending)
        x[p, 0, p // m, (p % m)::m] = torch.arange(256, dtype=torch.uint8)
        x[p, 1, p // m, (p % m)::m] = torch.arange(255, -1, -1, dtype=torch.uint8)
    st, mean, rstd, std = _stats32(2 * 4 ** L) if with_stats else (None, None, None, None)
    for tag, xd in (("vector", x.cuda()), ("scalar", _off(x, 1))):
        y = _encode(xd, L, norm, mean, rstd)
        back = _decode(y, L, norm, torch.uint8, mean, std, offset=0 if tag == "vector" else 1)
        assert torch.equal(back.cpu(), x), tag


def test_uint8_output_rounds_and_clamps():
    """(x + 1) 127.5 = 200.6 -> 201 (a cast gives 200); 127.5 exactly -> 128 (ties to even); out of range clamps."""
    vals = torch.tensor([200.6 / 127.5 - 1.0, 3.0, -3.0, 1.0, -1.0, 0.0])
    coef = torch.zeros(6, 4, 1, 1)
    coef[:, 0, 0, 0] = vals      # ll alone: a constant block of that value
    out = _decode(coef.cuda(), 1, "range", torch.uint8).cpu()
    assert out.shape == (6, 1, 2, 2)
    assert out[:, 0, 0, 0].tolist() == [201, 255, 0, 255, 0, 128]
    assert bool((out == out[:, :, :1, :1]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8"])
def test_encode_is_bitwise_reproducible(dtype):
    for shape in (SHAPES[1], SHAPES[4]):
        N, C, H, W, L = shape
        x = make_pixels((N, C, H, W), dtype).cuda()
        assert torch.equal(_encode(x, L, "orthonormal"), _encode(x, L, "orthonormal"))


def _prepare_wavelet(pool, table, F, L, norm, mean=None, rstd=None):
    from improved_diffusion import _native as nat
    B, Tp, C, H, W = pool.shape
    batch = torch.full((B, F, C * 4 ** L, H >> L, W >> L), NAN, device="cuda")
    fi = torch.full((B, F), -7, device="cuda", dtype=torch.int64)
    obs, lat = (torch.full((B, F, 1, 1, 1), NAN, device="cuda") for _ in range(2))
    nat.prepare_batch_wavelet(pool, table, batch, fi, obs, lat, L, norm, mean, rstd)
    torch.cuda.synchronize()
    return batch, fi, obs, lat


@pytest.mark.parametrize("with_stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("shape", [(3, 8, 10, 1), (3, 8, 12, 1), (3, 8, 12, 2), (4, 16, 32, 2)], ids=lambda s: "x".join(map(str, s)))
def test_prepare_batch_wavelet_is_prepare_batch_then_encode(shape, with_stats):
    from improved_diffusion import _native as nat
    C, H, W, L = shape
    B, Tp, F = 2, 5, 4
    pool_cpu = make_pixels((B * Tp, C, H, W), torch.float32).view(B, Tp, C, H, W)
    pool = pool_cpu.cuda()
    # rows in and out of range (a corrupt table is clamped, never followed), frame indices, flags that are not 0 / 1
    table = torch.tensor([[[4, 11, 1, 0], [0, 3, 0, 1], [-3, 5, 0, 0], [2, 2, 7, 0]],
                          [[1, 0, 0, 1], [99, 19, 1, 1], [5, 6, 0, -1], [3, 1, 0, 0]]], dtype=torch.int32).cuda()
    st, mean, rstd, std = _stats32(C * 4 ** L) if with_stats else (None, None, None, None)
    batch, fi, obs, lat = _prepare_wavelet(pool, table, F, L, "range", mean, rstd)
    # the two launches it replaces
    g = torch.full((B, F, C, H, W), NAN, device="cuda")
    fi2 = torch.zeros(B, F, device="cuda", dtype=torch.int64)
    obs2, lat2 = (torch.full((B, F, 1, 1, 1), NAN, device="cuda") for _ in range(2))
    nat.prepare_batch(pool, table, g, fi2, obs2, lat2)
    want = _encode(g.view(B * F, C, H, W), L, "range", mean, rstd).view(batch.shape)
    assert bool(torch.isfinite(batch).all())
    assert torch.equal(batch, want) and torch.equal(fi, fi2) and torch.equal(obs, obs2) and torch.equal(lat, lat2)
    rows = table[:, :, 0].clamp(0, Tp - 1).cpu()
    assert torch.equal(g.cpu(), torch.stack([pool_cpu[b][rows[b]] for b in range(B)]))
    assert fi.cpu().tolist() == [[11, 3, 5, 2], [0, 19, 6, 1]]
    # a uint8 pool: the gather of torch, then the encode
    pool8_cpu = make_pixels((B * Tp, C, H, W), torch.uint8).view(B, Tp, C, H, W)
    batch8, fi8, obs8, lat8 = _prepare_wavelet(pool8_cpu.cuda(), table, F, L, "range", mean, rstd)
    g8 = torch.stack([pool8_cpu[b][rows[b]] for b in range(B)]).cuda()
    assert torch.equal(batch8, _encode(g8.view(B * F, C, H, W), L, "range", mean, rstd).view(batch8.shape))
    assert torch.equal(fi8, fi2) and torch.equal(obs8, obs2) and torch.equal(lat8, lat2)
    # a pool one element off its alignment: the scalar path, the same bits
    batch_off = _prepare_wavelet(_off(pool_cpu, 1), table, F, L, "range", mean, rstd)[0]
    assert torch.equal(batch_off, batch)


def test_bad_shapes_return_their_code_and_launch_nothing():
    from improved_diffusion import _native as nat
    L = nat.lib()
    s = nat.stream()
    N, C, H, W = 2, 3, 8, 8
    x = make_pixels((N, C, H, W), torch.float32).cuda()
    y = torch.full((N * C * H * W,), NAN, device="cuda")
    m = torch.zeros(64, device="cuda")
    px, py, pm = x.data_ptr(), y.data_ptr(), m.data_ptr()

    def enc(pix=px, dtype=0, coef=py, mean=None, rstd=None, N=N, C=C, H=H, W=W, levels=1, norm=0):
        return L.lfvdm_wavelet_encode(pix, dtype, 1.0, 0.0, coef, mean, rstd, N, C, H, W, levels, norm, s)

    def dec(coef=px, mean=None, std=None, pix=py, dtype=0, N=N, C=C, H=H, W=W, levels=1, norm=0):
        return L.lfvdm_wavelet_decode(coef, mean, std, pix, dtype, N, C, H, W, levels, norm, s)
    for f in (enc, dec):
        assert f(H=7) == E_SHAPE and f(W=6, levels=2) == E_SHAPE and f(H=0) == E_SHAPE and f(N=0) == E_SHAPE and f(C=-1) == E_SHAPE
        assert f(dtype=2) == E_SHAPE and f(norm=2) == E_SHAPE and f(norm=-1) == E_SHAPE
        assert f(levels=3) == E_UNSUPPORTED and f(levels=0) == E_UNSUPPORTED
        assert f(N=1 << 16, C=1, H=1 << 8, W=(1 << 8) + 2) == E_UNSUPPORTED      # just over 2^31 elements
        assert f(N=1 << 20, C=1 << 10, H=1 << 10, W=1 << 10) == E_UNSUPPORTED    # far over: no overflow on the way
        assert f(mean=pm) == E_SHAPE
    assert enc(pix=None) == E_SHAPE and enc(coef=None) == E_SHAPE and enc(rstd=pm) == E_SHAPE
    assert dec(pix=None) == E_SHAPE and dec(coef=None) == E_SHAPE and dec(std=pm) == E_SHAPE

    B, F, Tp = 2, 2, 2
    table = torch.zeros(B, F, 4, device="cuda", dtype=torch.int32)
    fi = torch.full((B, F), -7, device="cuda", dtype=torch.int64)
    obs, lat = (torch.full((B, F), NAN, device="cuda") for _ in range(2))

    def prep(pool=px, dtype=0, table=table.data_ptr(), batch=py, fi_=fi.data_ptr(), obs_=obs.data_ptr(), lat_=lat.data_ptr(),
             mean=None, rstd=None, B=B, F=F, Tp=Tp, C=1, H=4, W=4, levels=1, norm=0):
        return L.lfvdm_prepare_batch_wavelet(pool, dtype, 1.0, 0.0, table, batch, fi_, obs_, lat_, mean, rstd, B, F, Tp, C, H, W,
                                             levels, norm, s)
    assert prep(H=5) == E_SHAPE and prep(W=6, levels=2) == E_SHAPE and prep(B=0) == E_SHAPE and prep(F=0) == E_SHAPE
    assert prep(Tp=0) == E_SHAPE and prep(B=65536) == E_SHAPE and prep(dtype=5) == E_SHAPE and prep(norm=3) == E_SHAPE
    assert prep(levels=4) == E_UNSUPPORTED and prep(mean=pm) == E_SHAPE and prep(rstd=pm) == E_SHAPE
    assert prep(B=1 << 12, F=1 << 10, C=1, H=1 << 5, W=(1 << 5) + 2) == E_UNSUPPORTED
    assert prep(B=1, F=1, Tp=1 << 22, C=1, H=1 << 5, W=(1 << 5) + 2) == E_UNSUPPORTED      # the pool counts too
    for name in ("pool", "table", "batch", "fi_", "obs_", "lat_"):
        assert prep(**{name: None}) == E_SHAPE, name
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(obs).all()) and bool(torch.isnan(lat).all()) and bool((fi == -7).all())
    # and the same pointers with a good shape do launch
    assert enc() == 0 and prep() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(obs).all()) and bool((fi == 0).all())
