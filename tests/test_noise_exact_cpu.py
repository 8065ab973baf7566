"""The host reference of the in-kernel noise (oracle/philox_ref.py) pinned on the CPU: Philox4x32-10 against its published
known-answer vectors and against a scalar restatement in Python integers, the Box-Muller restatement at the extreme
words, the two counter layouts, the key split, and the stream ids against csrc/philox_normal.h.  No GPU.  The kernels are
held to this reference in tests/test_noise_exact_gpu.py."""
import os
import re

import numpy as np
import pytest

from oracle import philox_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "latent-flexible-video-diffusion-modeling_amd", "csrc", "philox_normal.h")

# (counter, key, output) of Philox4x32-10: the known-answer vectors published with Random123 (Salmon et al., SC'11)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox_scalar(c, k):
    """Philox4x32-10 on Python integers, one counter: the round of the paper written out (mulhilo of c0 and c2, the xor
    with the neighbour word and the key, the Weyl key schedule)."""
    c, k, M = list(c), list(k), 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M, (p0 >> 32) ^ c[3] ^ k[1], p0 & M]
        k = [(k[0] + 0x9E3779B9) & M, (k[1] + 0xBB67AE85) & M]
    return tuple(c)


def test_philox_known_answer_vectors():
    for c, k, want in KAT:
        got = pr.philox4x32_10(*c, *k)
        assert all(g.dtype == np.uint32 for g in got)
        assert tuple(int(g) for g in got) == want, [hex(int(g)) for g in got]
        assert philox_scalar(c, k) == want
    # the three at once: the vectorised form, one key
    for c, k, want in KAT:
        cs = [np.array([KAT[0][0][i], c[i], KAT[1][0][i]], dtype=np.uint32) for i in range(4)]
        got = pr.philox4x32_10(*cs, *k)
        assert tuple(int(g[1]) for g in got) == want


def test_philox_vectorised_equals_scalar_on_random_counters():
    rng = np.random.RandomState(0)
    cs = rng.randint(0, 2 ** 32, size=(4, 64), dtype=np.uint64)
    for k in [(0, 0), (0, 1), (1, 0), (0xDEADBEEF, 0x01234567)]:
        got = pr.philox4x32_10(*cs, *k)
        for n in range(cs.shape[1]):
            assert tuple(int(g[n]) for g in got) == philox_scalar([int(c[n]) for c in cs], k), (k, n)
    # the key words are not interchangeable and the high word counts
    a, b = pr.philox4x32_10(*cs, 5, 9), pr.philox4x32_10(*cs, 9, 5)
    assert not any(np.array_equal(x, y) for x, y in zip(a, b))
    a, b = pr.philox4x32_10(*cs, 5, 0), pr.philox4x32_10(*cs, 5, 1)
    assert not any(np.array_equal(x, y) for x, y in zip(a, b))
    # each counter word has its own place
    w = [np.array([1, 0, 0, 0]), np.array([0, 1, 0, 0]), np.array([0, 0, 1, 0]), np.array([0, 0, 0, 1])]
    out = np.stack(pr.philox4x32_10(*w, 0, 0))
    assert len({tuple(out[:, n]) for n in range(4)}) == 4


def test_key_split():
    assert pr.split_seed(0) == (0, 0)
    assert pr.split_seed(1 << 32) == (0, 1)
    assert pr.split_seed(0x0123456789ABCDEF) == (0x89ABCDEF, 0x01234567)
    assert pr.split_seed(2 ** 63 - 1) == (0xFFFFFFFF, 0x7FFFFFFF)
    assert pr.split_seed(-1) == (0xFFFFFFFF, 0xFFFFFFFF)
    assert pr.split_seed(2 ** 64 + 7) == (7, 0)
    assert pr.split_seed(-2 ** 63) == pr.split_seed(2 ** 63) == (0, 0x80000000), "an int64 and the uint64 of the same bits"


def test_box_muller_at_the_extreme_words():
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    # r0 = 0: u0 = 2^-32, the largest radius sqrt(64 ln 2) = 6.6604...; angle word 0: (m, 0)
    z, m = pr.normal4_ref((u32(0), u32(0), u32(0), u32(0)))
    assert z.shape == (1, 4) and m.shape == (1, 2) and z.dtype == m.dtype == np.float64
    top = np.sqrt(64 * np.log(2.0))
    assert abs(top - 6.6604) < 1e-4
    assert m[0, 0] == m[0, 1] == top
    assert z[0].tolist() == [top, 0.0, top, 0.0]
    # r0 = 0xFFFFFFFF and 0xFFFFFF80 round to 2^32 in fp32 (0xFFFFFF80 is the tie, to even), + 1 stays: u0 = 1, m = 0
    z, m = pr.normal4_ref((u32(0xFFFFFFFF, 0xFFFFFF80), u32(123, 456), u32(0xFFFFFF80, 0xFFFFFFFF), u32(7, 0xFFFFFFFF)))
    assert np.array_equal(m, np.zeros((2, 2))) and np.array_equal(np.abs(z), np.zeros((2, 4)))
    # the largest word below that tie gives the smallest positive radius
    _, m = pr.normal4_ref((u32(0xFFFFFF7F), u32(0), u32(0xFFFFFE80), u32(0)))
    assert np.all(m > 0) and np.all(m < 1e-3)
    # r1 = 0xFFFFFFFF: u1 = 1 in fp32, the angle is two_pi_f32 itself
    z, m = pr.normal4_ref((u32(0), u32(0xFFFFFFFF), u32(0x80000000), u32(0xFFFFFFFF)))
    a = float(np.float32(6.283185307179586))
    assert z[0, 0] == m[0, 0] * np.cos(a) and z[0, 1] == m[0, 0] * np.sin(a)
    assert z[0, 2] == m[0, 1] * np.cos(a) and z[0, 3] == m[0, 1] * np.sin(a)
    # the uniform of the radius is rounded in fp32: (f32(r) + 1) * 2^-32, e.g. r = 2^24 + 1 -> 2^24 (+ 1 is absorbed too)
    _, m = pr.normal4_ref((u32(2 ** 24 + 1), u32(0), u32(2 ** 24), u32(0)))
    assert m[0, 0] == m[0, 1] == np.sqrt(-2.0 * np.log(2.0 ** -8))
    # every output finite and inside the largest radius, over a sweep of words that includes all of the above
    edge = u32(0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFE80, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFE, 0xFFFFFFFF)
    rng = np.random.RandomState(1)
    words = np.concatenate([edge, rng.randint(0, 2 ** 32, size=4096, dtype=np.uint64).astype(np.uint32)])
    ra, rb = np.meshgrid(words[:64], words[:64], indexing="ij")
    for r in ((ra, rb, rb, ra), (words, words[::-1], words[::-1], words)):
        z, m = pr.normal4_ref(r)
        assert np.all(np.isfinite(z)) and np.all(np.isfinite(m))
        assert np.all(np.abs(z) <= top) and np.all(m <= top) and np.all(m >= 0)
        assert np.all(np.abs(z[..., :2]) <= m[..., :1]) and np.all(np.abs(z[..., 2:]) <= m[..., 1:])


def direct(c, seed, e):
    """Element e of the quad with counter c under ``seed``, from the scalar Philox and normal4_ref."""
    words = philox_scalar(c, pr.split_seed(seed))
    z, m = pr.normal4_ref(tuple(np.array([w], dtype=np.uint32) for w in words))
    return z[0, e], m[0, e // 2]


def test_row_stream_layout():
    seed, t = 0x0123456789ABCDEF, [999, 1, 0]
    z, m = pr.row_stream_noise(seed, pr.STREAM_BLEND, t, 1027)
    assert z.shape == m.shape == (3, 1027) and z.dtype == np.float64
    # counter = (quad, batch row, t[b], stream); element 4 quad + e is value e of the quad
    for b, i in [(0, 0), (0, 3), (1, 4), (2, 1023), (1, 1024), (2, 1026)]:
        want = direct((i // 4, b, t[b], 1), seed, i % 4)
        assert (z[b, i], m[b, i]) == want, (b, i)
    # a partial quad is the prefix of the full one; a longer row only appends
    zf, mf = pr.row_stream_noise(seed, pr.STREAM_BLEND, t, 1028)
    assert np.array_equal(zf[:, :1027], z) and np.array_equal(mf[:, :1027], m)
    for inner in (1, 2, 3, 5):
        assert np.array_equal(pr.row_stream_noise(seed, 1, t, inner)[0], z[:, :inner])
    # the same (seed, t, row, quad) under another stream word: other values, everywhere
    per_stream = [pr.row_stream_noise(seed, s, t, 1027)[0] for s in (pr.STREAM_UPDATE, pr.STREAM_BLEND, pr.STREAM_RENOISE)]
    assert np.array_equal(per_stream[1], z)
    for a in range(3):
        for b in range(a + 1, 3):
            assert not np.any(per_stream[a] == per_stream[b]), (a, b)
    # a row's noise is a function of (row index, its t): another neighbour changes nothing, another t or row everything
    z2 = pr.row_stream_noise(seed, 1, [999, 7, 0], 1027)[0]
    assert np.array_equal(z2[[0, 2]], z[[0, 2]]) and not np.any(z2[1] == z[1])
    same_t = pr.row_stream_noise(seed, 1, [5, 5], 64)[0]
    assert not np.any(same_t[0] == same_t[1])
    # row and timestep are different counter words: (row 1, t 0) is not (row 0, t 1)
    swap = pr.row_stream_noise(seed, 1, [1, 0], 64)[0]
    assert not np.any(swap[0] == swap[1])
    # the seed: modulo 2^64, both halves count, and they are not interchangeable
    assert np.array_equal(pr.row_stream_noise(seed + 2 ** 64, 1, t, 1027)[0], z)
    assert np.array_equal(pr.row_stream_noise(-1, 0, t, 16)[0], pr.row_stream_noise(2 ** 64 - 1, 0, t, 16)[0])
    assert not np.any(pr.row_stream_noise(seed + 2 ** 32, 1, t, 1027)[0] == z)
    swapped = ((seed & 0xFFFFFFFF) << 32) | (seed >> 32)
    assert not np.any(pr.row_stream_noise(swapped, 1, t, 1027)[0] == z)


def test_search_layout():
    V, fe = 2, 64
    # a padding slot, frame 299, and (video 0, frame 5) / (video 1, frame 5) in different slots of different windows
    table = np.array([[5, 1, -1], [5, 299, 2], [0, 5, 1], [2, 0, 5]], dtype=np.int32)
    seed, step, j = 2 ** 63 + 12345, 2 ** 24 - 1, 65534
    z, m = pr.search_noise(seed, step, j, table, V, fe)
    assert z.shape == m.shape == (4, 3, fe)
    assert np.array_equal(z[0, 2].view(np.uint64), np.zeros(fe, dtype=np.uint64)), "padding: +0, bit for bit"
    assert np.array_equal(m[0, 2], np.zeros(fe))
    # counter = (quad in frame, video frame, j << 16 | video, step << 8 | 3)
    for (w, k), i in [((0, 0), 0), ((1, 1), 63), ((3, 2), 5), ((2, 0), 17)]:
        c = (i // 4, int(table[w, k]), (j << 16) | (w % V), (step << 8) | 3)
        assert (z[w, k, i], m[w, k, i]) == direct(c, seed, i % 4), (w, k, i)
    # the same (video, frame): the same frame of noise, whatever the slot and the window
    assert np.array_equal(z[0, 0], z[2, 1]), "video 0, frame 5"
    assert np.array_equal(z[1, 0], z[3, 2]), "video 1, frame 5"
    assert np.array_equal(z[0, 1], z[2, 2]), "video 0, frame 1"
    assert np.array_equal(z[1, 2], z[3, 0]), "video 1, frame 2"
    # another video, frame, position, window step or seed: other values everywhere
    assert not np.any(z[0, 0] == z[1, 0]) and not np.any(z[0, 0] == z[0, 1])
    live = table >= 0
    for other in (pr.search_noise(seed, step, j - 1, table, V, fe), pr.search_noise(seed, step - 1, j, table, V, fe),
                  pr.search_noise(seed + 2 ** 32, step, j, table, V, fe), pr.search_noise(seed - 2 ** 63, step, j, table, V, fe)):
        assert not np.any(other[0][live] == z[live])
    # j and the video share a word, j above: (j = 0, video 1) is not (j = 1, video 0)
    a = pr.search_noise(seed, 0, 0, np.array([[7], [7]]), 2, fe)[0][1, 0]
    b = pr.search_noise(seed, 0, 1, np.array([[7], [7]]), 2, fe)[0][0, 0]
    assert not np.any(a == b)
    # an int64 key and the uint64 of the same bits are one seed
    assert np.array_equal(pr.search_noise(seed - 2 ** 64, step, j, table, V, fe)[0], z)
    # the search's stream is apart from the row streams: a row-stream counter with the same first three words differs
    row = pr.row_stream_noise(seed, pr.STREAM_SEARCH, [0], fe)[0][0]
    srch = pr.search_noise(seed, 1, 0, np.array([[0]]), 1, fe)[0][0, 0]
    assert not np.any(row == srch)
    with pytest.raises(ValueError):
        pr.search_noise(seed, 2 ** 24, 0, table, V, fe)
    with pytest.raises(ValueError):
        pr.search_noise(seed, 0, 2 ** 16, table, V, fe)


def test_stream_ids_are_the_headers():
    ids = dict(re.findall(r"(NOISE_STREAM_[A-Z]+) = (\d+)", open(HEADER).read()))
    assert {k: int(v) for k, v in ids.items()} == {
        "NOISE_STREAM_UPDATE": pr.STREAM_UPDATE, "NOISE_STREAM_BLEND": pr.STREAM_BLEND,
        "NOISE_STREAM_RENOISE": pr.STREAM_RENOISE, "NOISE_STREAM_SEARCH": pr.STREAM_SEARCH}
    assert (pr.STREAM_UPDATE, pr.STREAM_BLEND, pr.STREAM_RENOISE, pr.STREAM_SEARCH) == (0, 1, 2, 3)
