"""Host reference of the samplers' in-kernel Gaussian noise (csrc/philox_normal.h), numpy only.

Written from the header comments of philox_normal.h, known_region.hip and schedule_search.hip - the contract - not from
the kernels: Philox4x32-10 (Salmon et al., SC'11) keyed by a 64-bit seed (k0 = low word, k1 = high word), one counter
per quad of four consecutive elements, Box-Muller on the four output words.  The integer part is exact; the Box-Muller
part repeats in ``np.float32`` the roundings the kernel performs on its INPUTS (word -> uniform, uniform -> angle) and
does the transcendental part in float64, so what is left between this reference and the device is the error of the
device's logf / sqrtf / sincosf and of one fp32 product.

Counter layouts:
  row streams     (quad within the batch row, batch row, timestep t[b], stream word)     update 0, blend 1, re-noise 2
  schedule search (quad within the frame, video frame, j << 16 | video, step << 8 | 3)   video = window % V
"""
import numpy as np

STREAM_UPDATE, STREAM_BLEND, STREAM_RENOISE, STREAM_SEARCH = 0, 1, 2, 3

_M32 = np.uint64(0xFFFFFFFF)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)       # the round's two multipliers (of c0 and of c2)
_WEYL0, _WEYL1 = 0x9E3779B9, 0xBB67AE85                           # the key schedule's increments
_SH32 = np.uint64(32)


def _u64(a):
    """Anything integer -> uint64 array of its value modulo 2^32."""
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise TypeError(f"counter and key words are integers, got {a.dtype}")
    return a.astype(np.int64 if a.dtype.kind == "i" else np.uint64).astype(np.uint64) & _M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counters (c0, c1, c2, c3) under the key (k0, k1), vectorised (the arguments broadcast against
    each other) -> four uint32 arrays.  Every word lives in a uint64 and is masked to 32 bits after each operation."""
    c0, c1, c2, c3 = np.broadcast_arrays(_u64(c0), _u64(c1), _u64(c2), _u64(c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2                           # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> _SH32, p0 & _M32, p1 >> _SH32, p1 & _M32
        c0, c1, c2, c3 = (hi1 ^ c1 ^ np.uint64(k0)) & _M32, lo1, (hi0 ^ c3 ^ np.uint64(k1)) & _M32, lo0
        k0, k1 = (k0 + _WEYL0) & 0xFFFFFFFF, (k1 + _WEYL1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def normal4_ref(words):
    """Box-Muller on four uint32 word arrays (r0, r1, r2, r3) -> (z, m): z float64 (..., 4) = (m0 cos a0, m0 sin a0,
    m1 cos a1, m1 sin a1) and m float64 (..., 2), the radius of each pair.  In fp32 as the kernel: u = (f32(r) + 1) * 2^-32
    for the radius words (in (0, 1]), u = f32(r) * 2^-32 for the angle words, a = two_pi_f32 * u; log, sqrt, sin, cos and
    the final product in float64 on those fp32 values."""
    r0, r1, r2, r3 = (np.asarray(w, dtype=np.uint32) for w in words)
    f32 = np.float32
    s32, two_pi, one = f32(2.0 ** -32), f32(6.283185307179586), f32(1.0)

    def pair(ra, rb):
        u = (ra.astype(f32) + one) * s32
        a = two_pi * (rb.astype(f32) * s32)
        assert u.dtype == np.float32 and a.dtype == np.float32
        m = np.sqrt(-2.0 * np.log(u.astype(np.float64)))
        a = a.astype(np.float64)
        return m, m * np.cos(a), m * np.sin(a)
    m0, z0, z1 = pair(r0, r1)
    m1, z2, z3 = pair(r2, r3)
    return np.stack([z0, z1, z2, z3], axis=-1), np.stack([m0, m1], axis=-1)


def split_seed(seed):
    """Any Python int -> (k0, k1): the seed modulo 2^64, low and high 32 bits."""
    s = int(seed) % (1 << 64)
    return s & 0xFFFFFFFF, s >> 32


def _per_element(m):
    """radius per pair (..., Q, 2) -> radius per element (..., 4 Q)"""
    return np.repeat(m, 2, axis=-1).reshape(m.shape[:-2] + (-1,))


def row_stream_noise(seed, stream, t_rows, inner):
    """The noise of a (B, inner) tensor drawn by a row-stream launch: counter (quad, batch row b, t_rows[b], stream), the
    quad's four values at elements 4 quad .. 4 quad + 3 of the row; a trailing partial quad is cut at ``inner``.
    -> (z, m), both float64 (B, inner); m is the radius of the element's pair."""
    t_rows = np.asarray(t_rows, dtype=np.int64)
    B, nq = t_rows.shape[0], (int(inner) + 3) // 4
    k0, k1 = split_seed(seed)
    quad = np.arange(nq, dtype=np.uint64)[None, :]
    row = np.arange(B, dtype=np.uint64)[:, None]
    words = philox4x32_10(quad, row, t_rows[:, None], np.uint64(int(stream)), k0, k1)
    z, m = normal4_ref(words)                                     # (B, nq, 4), (B, nq, 2)
    return z.reshape(B, 4 * nq)[:, :inner], _per_element(m)[:, :inner]


def search_noise(seed, step, j, table, V, frame_elems):
    """The schedule search's noise for the windows of ``table`` (W, K) int (video frame per slot, < 0: padding), window w
    showing video w % V: counter (quad within the frame, video frame, j << 16 | w % V, step << 8 | 3); padding slots are
    zero (and their m is zero).  -> (z, m), both float64 (W, K, frame_elems)."""
    table = np.asarray(table, dtype=np.int64)
    W, K = table.shape
    step, j, V, frame_elems = int(step), int(j), int(V), int(frame_elems)
    if not (0 <= step < 1 << 24 and 0 <= j < 1 << 16 and 0 < V < 1 << 16 and frame_elems % 4 == 0):
        raise ValueError("step has 24 bits, j and the video 16 each, a frame is whole quads")
    k0, k1 = split_seed(seed)
    quad = np.arange(frame_elems // 4, dtype=np.uint64)[None, None, :]
    video = (np.arange(W, dtype=np.int64) % V)[:, None, None]
    frame = np.maximum(table, 0)[:, :, None]
    words = philox4x32_10(quad, frame, (j << 16) | video, np.uint64((step << 8) | STREAM_SEARCH), k0, k1)
    z, m = normal4_ref(words)                                     # (W, K, Q, 4), (W, K, Q, 2)
    live = (table >= 0)[:, :, None]
    return np.where(live, z.reshape(W, K, frame_elems), 0.0), np.where(live, _per_element(m), 0.0)
