"""Temporally correlated noise prior, host side (no GPU): the spec parser, the float64 covariance and its factor (unit
diagonal, L L^T = K, PYoCo's two priors as special cases, repeated indices, the sub-matrix property), the empirical
covariance of the CPU ``apply_noise_prior``, every refusal of ``GaussianDiffusion`` under a prior, the front ends'
resolution of the setting, and the two exports."""
import ctypes
import logging
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from improved_diffusion import noise_prior as npr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXEL = {"diffusion_space": "pixel", "pre_encoded": False, "pre_encoded_stats_dict": None}
NAMES = ("lfvdm_noise_prior_factor", "lfvdm_noise_prior_fill")

INDEX_SETS = {
    "sorted": np.arange(20),
    "shuffled": np.random.RandomState(0).permutation(20),
    "wide": np.array([0, 1000000, 3, 2000007, 17, 5000000, 4]),
    "long": np.random.RandomState(1).permutation(300)[:64],
}
PRIORS = ["mixed:1", "progressive:2", "cov:0.2:0.5:0.9", "cov:0.3:0.7:0.99"]


def make_diffusion(resp="ddim10", use_kl=False):
    from improved_diffusion import script_util as su
    return su.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, rescale_timesteps=True, rescale_learned_sigmas=True,
                                        use_kl=use_kl, diffusion_space_kwargs=dict(PIXEL))


# ------------------------------------------------------------------------------------------------ the parser
def test_parser_forms_and_round_trips():
    assert npr.parse_noise_prior("mixed:1") == (0.5, 0.0, 0.0)
    a, c, rho = npr.parse_noise_prior("mixed:2")
    assert (a, c, rho) == (4.0 / 5.0, 0.0, 0.0)
    assert npr.parse_noise_prior("progressive:2") == (0.0, 1.0, 2.0 / math.sqrt(5.0))
    assert npr.parse_noise_prior(" cov:0.2:0.5:0.9 ") == (0.2, 0.5, 0.9)
    assert npr.parse_noise_prior("COV:0.7:0.3:0") == (0.7, 0.3, 0.0), "a + c = 1 up to rounding is allowed"
    for off in (None, "", "none", " None ", "cov:0:0:0.5", "mixed:0", (0.0, 0.0, 0.3)):
        assert npr.parse_noise_prior(off) is None, off
    assert npr.parse_noise_prior((0.25, 0.5, 0.75)) == (0.25, 0.5, 0.75)
    for spec in PRIORS + ["mixed:0.3", "progressive:0.1", "cov:0.1:0.2:0.123456789012345"]:
        prior = npr.parse_noise_prior(spec)
        text = npr.format_noise_prior(prior)
        assert text.startswith("cov:") and npr.parse_noise_prior(text) == prior, spec
        assert npr.format_noise_prior(spec) == text
    assert npr.format_noise_prior(None) == "none" and npr.format_noise_prior("mixed:0") == "none"


@pytest.mark.parametrize("spec", ["cov:0.6:0.5:0.1", "cov:0.2:0.2:1", "cov:0.2:0.2:1.5", "cov:-0.1:0.2:0.5", "cov:0.1:-0.2:0.5",
                                  "cov:0.1:0.2:-0.5", "mixed:-1", "progressive:-2", "cov:0.1:0.2", "mixed", "mixed:1:2",
                                  "progressive:x", "pyoco:1", "none:1", "cov:nan:0.1:0.1", "progressive:inf", 3, (0.1, 0.2),
                                  (0.9, 0.2, 0.1)])
def test_parser_rejections(spec):
    with pytest.raises(ValueError):
        npr.parse_noise_prior(spec)


# ------------------------------------------------------------------------------------------------ K and L
@pytest.mark.parametrize("spec", PRIORS)
@pytest.mark.parametrize("name", list(INDEX_SETS))
def test_cov_has_unit_diagonal_and_the_factor_reproduces_it(name, spec):
    f, prior = INDEX_SETS[name], npr.parse_noise_prior(spec)
    K, L = npr.noise_prior_cov(f, *prior), npr.noise_prior_factor_ref(f, *prior)
    T = len(f)
    assert K.dtype == np.float64 and K.shape == (T, T) and np.array_equal(np.diag(K), np.ones(T)) and np.array_equal(K, K.T)
    a, c, rho = prior
    for i, j in ((0, T - 1), (1, 2), (T - 1, T // 2)):
        assert K[i, j] == a + c * rho ** float(abs(int(f[i]) - int(f[j])))
    assert np.array_equal(L, np.tril(L)) and np.all(np.isfinite(L))
    assert np.abs(L @ L.T - K).max() <= 1e-12
    # batched: one factor per row
    fb = np.stack([f, f[::-1]])
    Lb = npr.noise_prior_factor_ref(fb, *prior)
    assert Lb.shape == (2, T, T) and np.array_equal(Lb[0], L)
    assert np.abs(Lb[1] @ Lb[1].T - npr.noise_prior_cov(f[::-1], *prior)).max() <= 1e-12


def test_progressive_is_pyocos_recursion_on_consecutive_indices():
    """eps_0 = xi_0, eps_i = rho eps_{i-1} + sqrt(1 - rho^2) xi_i  <=>  L_i0 = rho^i, L_ij = rho^(i-j) sqrt(1 - rho^2)."""
    T, alpha = 16, 2.0
    _, _, rho = npr.parse_noise_prior(f"progressive:{alpha}")
    assert rho == alpha / math.sqrt(1 + alpha * alpha)
    L = npr.noise_prior_factor_ref(np.arange(T), 0.0, 1.0, rho)
    want = np.zeros((T, T))
    for i in range(T):
        want[i, 0] = rho ** i
        for j in range(1, i + 1):
            want[i, j] = rho ** (i - j) * math.sqrt(1 - rho * rho)
    assert np.abs(L - want).max() <= 1e-14
    xi = np.random.RandomState(2).randn(T, 5)
    eps = np.empty_like(xi)
    eps[0] = xi[0]
    for i in range(1, T):
        eps[i] = rho * eps[i - 1] + math.sqrt(1 - rho * rho) * xi[i]
    assert np.abs(L @ xi - eps).max() <= 1e-13


def test_mixed_has_constant_off_diagonal_covariance():
    alpha = 1.5
    K = npr.noise_prior_cov(INDEX_SETS["wide"], *npr.parse_noise_prior(f"mixed:{alpha}"))
    off = K[~np.eye(len(K), dtype=bool)]
    assert np.array_equal(off, np.full_like(off, alpha * alpha / (1 + alpha * alpha)))


def test_repeated_indices_give_identical_rows_and_no_nan():
    f = np.array([7, 3, 7, 12, 3, 7])
    for prior in [(0.0, 1.0, 0.8), (0.25, 0.75, 0.5), (1.0, 0.0, 0.0)]:      # a + c = 1 (exactly): K is singular
        L = npr.noise_prior_factor_ref(f, *prior)
        assert np.all(np.isfinite(L))
        assert np.array_equal(L[2], L[0]) and np.array_equal(L[5], L[0]) and np.array_equal(L[4], L[1])
        assert np.array_equal(L[:, 2], np.zeros(6)) and np.array_equal(L[:, 4], np.zeros(6)), "a twin's column is zero"
        assert np.abs(L @ L.T - npr.noise_prior_cov(f, *prior)).max() <= 1e-12
        xi = torch.randn(1, 6, 3, 2, 2, generator=torch.Generator().manual_seed(1))
        eps = npr.apply_noise_prior(xi, torch.from_numpy(f)[None], prior)
        assert bool(torch.isfinite(eps).all())
        assert torch.equal(eps[0, 2], eps[0, 0]) and torch.equal(eps[0, 5], eps[0, 0]) and torch.equal(eps[0, 4], eps[0, 1])
    L = npr.noise_prior_factor_ref(f, 0.2, 0.5, 0.8)      # with an independent part the twins differ
    assert not np.array_equal(L[2], L[0]) and np.abs(L @ L.T - npr.noise_prior_cov(f, 0.2, 0.5, 0.8)).max() <= 1e-12


@pytest.mark.parametrize("spec", PRIORS)
def test_sub_matrix_property(spec):
    """Any subset of the frames, in any order, has the matching sub-matrix of K as its covariance."""
    prior = npr.parse_noise_prior(spec)
    f = INDEX_SETS["shuffled"]
    K = npr.noise_prior_cov(f, *prior)
    pick = np.array([11, 2, 17, 5, 0])
    Ls = npr.noise_prior_factor_ref(f[pick], *prior)
    assert np.abs(Ls @ Ls.T - K[np.ix_(pick, pick)]).max() <= 1e-12


@pytest.mark.parametrize("spec", ["mixed:1", "progressive:2", "cov:0.2:0.5:0.9"])
def test_empirical_covariance_of_the_cpu_path(spec):
    """n i.i.d. columns: the estimate mean(eps_i eps_j) of K_ij (the mean is known to be 0) has variance
    (K_ii K_jj + K_ij^2) / n = (1 + K_ij^2) / n for a Gaussian vector, so every entry lies within 6 standard errors -
    a bound derived from the law, not tuned (6 sigma over 100 entries: a false alarm about once in 10^7 runs)."""
    prior = npr.parse_noise_prior(spec)
    f = torch.tensor([[4, 0, 9, 1, 30, 2, 3, 1000, 8, 5], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]])
    B, T, n = 2, 10, 40000
    xi = torch.randn(B, T, 4, 100, 100, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    eps = npr.apply_noise_prior(xi, f, prior)
    assert eps.dtype == torch.float64 and eps.shape == xi.shape
    for b in range(B):
        K = npr.noise_prior_cov(f[b], *prior)
        e = eps[b].reshape(T, n).numpy()
        emp = e @ e.T / n
        se = np.sqrt((1.0 + K * K) / n)
        assert np.all(np.abs(emp - K) <= 6.0 * se), (b, float((np.abs(emp - K) / se).max()))
    # float32 in, float32 out, rounded from the float64 product
    x32 = xi[:, :, :, :2, :2].float()
    got = npr.apply_noise_prior(x32, f, prior)
    L = torch.from_numpy(npr.noise_prior_factor_ref(f.numpy(), *prior))
    assert got.dtype == torch.float32
    assert torch.equal(got, torch.einsum("bij,bje->bie", L, x32.reshape(B, T, -1).double()).reshape(x32.shape).float())
    assert npr.apply_noise_prior(x32, f, None) is x32 and npr.apply_noise_prior(x32, f, "none") is x32


def test_apply_refusals():
    xi = torch.zeros(2, 3, 1, 2, 2)
    with pytest.raises(ValueError, match="frame_indices"):
        npr.apply_noise_prior(xi, None, "mixed:1")
    with pytest.raises(ValueError, match="one index per frame"):
        npr.apply_noise_prior(xi, torch.zeros(2, 4, dtype=torch.long), "mixed:1")
    with pytest.raises(ValueError, match="at most 64"):
        npr.apply_noise_prior(torch.zeros(1, 65, 4), torch.zeros(1, 65, dtype=torch.long), "mixed:1")


# ------------------------------------------------------------------------------------------------ GaussianDiffusion
def _net(x, timesteps=None, **kw):
    return 0.1 * x, None


def test_setter_attribute_and_noise_draws_on_the_cpu():
    diff = make_diffusion()
    assert diff.noise_prior is None
    diff.set_noise_prior("progressive:2")
    assert diff.noise_prior == (0.0, 1.0, 2.0 / math.sqrt(5.0))
    diff.set_noise_prior("none")
    assert diff.noise_prior is None
    diff.set_noise_prior((0.2, 0.5, 0.9))
    assert diff.noise_prior == (0.2, 0.5, 0.9)
    diff.set_noise_prior()
    assert diff.noise_prior is None
    with pytest.raises(ValueError):
        diff.set_noise_prior("cov:0.9:0.9:0.1")
    assert diff.noise_prior is None, "a refused spec leaves the setting alone"

    # the eager stochastic DDIM step on the CPU (the ``denoised_fn`` route is plain torch): its draw is L randn
    x = torch.randn(2, 5, 1, 4, 4, generator=torch.Generator().manual_seed(3))
    t = torch.tensor([9, 4])
    fi = torch.tensor([[3, 0, 7, 1, 2], [10, 40, 20, 30, 0]])
    mk = {"frame_indices": fi}
    fn = lambda v: v      # noqa: E731
    torch.manual_seed(5)
    plain = diff.ddim_sample(_net, x, t, model_kwargs=mk, eta=1.0, denoised_fn=fn)["sample"]
    diff.set_noise_prior("progressive:2")
    torch.manual_seed(5)
    corr = diff.ddim_sample(_net, x, t, model_kwargs=mk, eta=1.0, denoised_fn=fn)["sample"]
    torch.manual_seed(5)
    noise = npr.apply_noise_prior(torch.randn_like(x), fi, "progressive:2")
    given = diff.ddim_sample(_net, x, t, model_kwargs=mk, eta=1.0, denoised_fn=fn, noise=noise)["sample"]
    assert torch.equal(corr, given) and not torch.equal(corr, plain)
    torch.manual_seed(5)
    assert torch.equal(diff.ddim_sample(_net, x, t, model_kwargs=mk, eta=1.0, denoised_fn=fn, noise=torch.randn_like(x))["sample"],
                       plain), "noise passed in by the caller is used as given"
    det = diff.ddim_sample(_net, x, t, model_kwargs={}, eta=0.0, denoised_fn=fn)["sample"]      # draws nothing: no indices needed
    diff.set_noise_prior(None)
    assert torch.equal(det, diff.ddim_sample(_net, x, t, model_kwargs={}, eta=0.0, denoised_fn=fn)["sample"])


def test_refusals_of_the_diffusion_object():
    from improved_diffusion import optimal_schedule as osch
    from improved_diffusion.sampling_schemes import sampling_schemes
    diff = make_diffusion()
    diff.set_noise_prior("mixed:1")
    x = torch.zeros(2, 3, 1, 4, 4)
    t = torch.tensor([9, 4])
    for kwargs in (None, {}, {"x0": x}):
        with pytest.raises(ValueError, match="frame_indices"):
            diff.training_losses(_net, x, t, model_kwargs=kwargs)
        with pytest.raises(ValueError, match="frame_indices"):
            diff.ddim_sample(_net, x, t, model_kwargs=kwargs, eta=1.0, denoised_fn=lambda v: v)
        with pytest.raises(ValueError, match="frame_indices"):
            diff.p_sample(_net, x, t, model_kwargs=kwargs, denoised_fn=lambda v: v)
        with pytest.raises(ValueError, match="frame_indices"):
            next(diff.ddim_sample_loop_progressive(_net, (2, 3, 1, 4, 4), model_kwargs=kwargs, device="cpu"))
    calls = []

    def counting(x_, timesteps=None, **kw):
        calls.append(1)
        return x_, None
    mk = {"frame_indices": torch.arange(3).repeat(2, 1)}
    with pytest.raises(NotImplementedError, match="cov:0.5:0.0:0.0"):
        diff.calc_bpd_loop(counting, x, model_kwargs=mk)
    with pytest.raises(NotImplementedError, match="cov:0.5:0.0:0.0"):
        diff.calc_bpd_loop_subsampled(counting, x, model_kwargs=mk, t_seq=[3, 1])
    with pytest.raises(NotImplementedError, match="cov:0.5:0.0:0.0"):
        diff.known_region_sample_loop(counting, (2, 3, 1, 4, 4), x, torch.ones(2, 3, 4, 4), model_kwargs=mk, device="cpu",
                                      return_decoded=False)
    with pytest.raises(NotImplementedError, match="cov:0.5:0.0:0.0"):      # raised at the call, not at the first next()
        diff.known_region_sample_loop_progressive(counting, (2, 3, 1, 4, 4), x, torch.ones(2, 3, 4, 4), model_kwargs=mk,
                                                  device="cpu")
    scheme = sampling_schemes["autoreg"](video_length=8, num_obs=2, max_frames=4, step_size=2)
    with pytest.raises(NotImplementedError, match="cov:0.5:0.0:0.0"):
        osch.find_optimal_schedule(counting, diff, torch.zeros(1, 8, 1, 4, 4), scheme, n_timesteps=2)
    assert not calls, "refused before any work"

    kl = make_diffusion(use_kl=True)
    with pytest.raises(ValueError, match="independent noise"):
        kl.set_noise_prior("mixed:1")
    kl.set_noise_prior("none")
    assert kl.noise_prior is None


def test_prior_is_part_of_the_sampler_cache_key(monkeypatch):
    diff = make_diffusion()
    monkeypatch.setattr(diff, "_cached_sampler", lambda cache, key, *a, **k: key)
    unet, shape = object(), (2, 4, 3, 8, 8)
    off = diff._graph_sampler(unet, shape, True)
    diff.set_noise_prior("mixed:1")
    on = diff._graph_sampler(unet, shape, True)
    diff.set_noise_prior("progressive:2")
    other = diff._graph_sampler(unet, shape, True)
    assert len({off, on, other}) == 3 and on[:4] == off[:4] and (0.5, 0.0, 0.0) in on and on[-1] is None
    diff.set_dynamic_threshold(0.995)
    assert diff._graph_sampler(unet, shape, True)[-1] == (0.995, None), "the threshold stays the key's last element"
    diff.set_dynamic_threshold()
    diff.set_noise_prior(None)
    assert diff._graph_sampler(unet, shape, True) == off


# ------------------------------------------------------------------------------------------------ front ends
def test_front_ends_resolve_the_setting(monkeypatch, caplog):
    from improved_diffusion.train_util import resolve_noise_prior as train_resolve
    from improved_diffusion.video_sampler import default_sampling_args, resolve_noise_prior, warn_noise_prior_mismatch
    monkeypatch.delenv("LFVDM_NOISE_PRIOR", raising=False)
    a = default_sampling_args(device="cpu")
    assert a.noise_prior is None and resolve_noise_prior(a) is None and train_resolve(None, a) is None
    monkeypatch.setenv("LFVDM_NOISE_PRIOR", "progressive:2")
    assert resolve_noise_prior(a) == "progressive:2"
    assert train_resolve(None, a) == npr.format_noise_prior("progressive:2")
    b = default_sampling_args(device="cpu", noise_prior="mixed:1")
    assert resolve_noise_prior(b) == "mixed:1", "args win over the environment"
    assert train_resolve(None, b) == "cov:0.5:0.0:0.0" and train_resolve("none", b) == "none", "the keyword wins over args"
    monkeypatch.setenv("LFVDM_NOISE_PRIOR", "pyoco")
    with pytest.raises(ValueError):
        resolve_noise_prior(a)
    with pytest.raises(ValueError):
        train_resolve(None, types.SimpleNamespace())
    with caplog.at_level(logging.WARNING, logger="improved_diffusion"):
        assert not warn_noise_prior_mismatch(None, (0.5, 0.0, 0.0))
        assert not warn_noise_prior_mismatch("cov:0.5:0.0:0.0", "mixed:1")
        assert not warn_noise_prior_mismatch("none", None)
        assert not caplog.records
        assert warn_noise_prior_mismatch("cov:0.5:0.0:0.0", None)
        assert warn_noise_prior_mismatch("none", "progressive:2")
    assert len(caplog.records) == 2 and "trained with the noise prior 'cov:0.5:0.0:0.0'" in caplog.records[0].getMessage()


# ------------------------------------------------------------------------------------------------ the ABI
def test_entries_are_declared_bound_and_exported():
    from improved_diffusion import _native as nat
    header = open(os.path.join(ROOT, "include", "lfvdm_hip.h")).read()
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), f"{name} is not declared in lfvdm_hip.h"
        assert name in nat.EXPORTS
        getattr(L, name)
    assert callable(nat.noise_prior_factor) and callable(nat.noise_prior_fill)
    assert nat.lib().lfvdm_abi_version() == 9
    philox = open(os.path.join(ROOT, "latent-flexible-video-diffusion-modeling_amd", "csrc", "philox_normal.h")).read()
    # the enumerator follows NOISE_STREAM_SEARCH = 3 by position and is pinned to 4; the comment table names it
    assert re.search(r"NOISE_STREAM_SEARCH = 3, NOISE_STREAM_PRIOR\s*\}", philox)
    assert re.search(r"static_assert\(NOISE_STREAM_PRIOR == 4\b", philox) and re.search(r"//\s+NOISE_STREAM_PRIOR\s+4\b", philox)
    # argument checks come before any launch: they answer without a device
    lib = nat.lib()
    one = ctypes.c_void_p(16)      # never dereferenced: every call below is refused
    assert lib.lfvdm_noise_prior_factor(one, 0.0, 1.0, 0.5, one, 1, 65, None) == 1
    assert lib.lfvdm_noise_prior_factor(one, 0.0, 1.0, 0.5, one, 1, 0, None) == 1
    assert lib.lfvdm_noise_prior_factor(one, 0.6, 0.6, 0.5, one, 1, 4, None) == 1
    assert lib.lfvdm_noise_prior_factor(one, 0.0, 1.0, 1.0, one, 1, 4, None) == 1
    assert lib.lfvdm_noise_prior_factor(None, 0.0, 1.0, 0.5, one, 1, 4, None) == 1
    assert lib.lfvdm_noise_prior_fill(one, one, None, None, one, 1, 65, 16, None) == 1
    assert lib.lfvdm_noise_prior_fill(one, None, one, one, one, 1, 4, 6, None) == 1, "draw mode: E % 4 != 0"
    assert lib.lfvdm_noise_prior_fill(one, None, None, one, one, 1, 4, 8, None) == 1, "draw mode without a seed"
    assert lib.lfvdm_noise_prior_fill(one, one, None, None, one, 1, 2, 2 ** 31, None) == 1
