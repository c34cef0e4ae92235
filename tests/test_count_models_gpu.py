"""GPU tier: Poisson and negative binomial regression, linear regression with an estimated noise level and
hierarchical Poisson regression (models/glm.h, models/glm_scale.h, models/hier_glm.h) on the MI355X.

  * the count maths (wnd::dlog1p, dsoftplus, dlgamma_diff, ddigamma_diff) on the device equal the host build of the same
    source bit for bit on 2^20 arguments each (wn_internal_count_math_probe);
  * device = emulation, bit for bit, for the five models at (1, 2), (1, 4), (1, 8) and (1, 16), over logp_grad, warmup
    and sampling transitions; (1, 8) also for determinism and against NumPy;
  * posterior means and variances within 5 Monte Carlo standard errors of quadrature (Poisson intercept + slope and
    negative binomial intercept + s on 2-D grids; linear_regression_sigma with beta integrated out, 1-D over s), and
    R-hat < 1.01;
  * the drop-in calls with data=, datasets= and (x, y, group);
  * chains placed where the energies are non-finite: IEEE results, the other chains finite, check() clean."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_count_reference as hc  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from walnuts_amd import _ffi  # noqa: E402
from test_count_models_sim import (FLAT, FLAT_IDS, HPOIS, HPOIS_C, LSIG, NB, POIS, make_count,  # noqa: E402
                                   make_hier, scale_model, thetas)
from test_count_math import probe  # noqa: E402

pytestmark = pytest.mark.gpu
ALL = FLAT + (HPOIS, HPOIS_C)
ALL_IDS = FLAT_IDS + ["hier_poisson", "hier_poisson_c"]


def probe_args(fn, n, rng):
    if fn == 0:
        x = np.concatenate([-np.exp(rng.uniform(-745, 0, n // 2)), np.exp(rng.uniform(-745, 709, n - n // 2))])
        return x, np.zeros(n)
    if fn == 1:
        return rng.uniform(-800, 800, n) * rng.uniform(0, 1, n) ** 3, np.zeros(n)
    y = np.floor(np.exp(rng.uniform(0, math.log(2.0 ** 41), n)) - 1)
    y[: n // 8] = rng.integers(0, 4, n // 8)
    phi = np.exp(-rng.uniform(-36.8, 27.6, n))
    return y, phi


@pytest.mark.timeout(900)
@pytest.mark.parametrize("fn", [0, 1, 2, 3], ids=["log1p", "softplus", "lgamma_diff", "digamma_diff"])
def test_count_math_device_equals_host(gpu, fn):
    host = _ffi.load_library(simbuild.build())
    dev = wa.load_library()
    x, phi = probe_args(fn, 1 << 20, np.random.default_rng(fn))
    a, b = probe(dev, fn, x, phi), probe(host, fn, x, phi)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), int(np.sum(a.view(np.uint64) != b.view(np.uint64)))


def model_data(model, D, N, seed):
    """(data, model_params) of any of the five models at num_params D"""
    if model in (HPOIS, HPOIS_C):
        P, J = max(1, D // 3), D - max(1, D // 3) - 1
        x, y, group, mp = make_hier(P, J, N, seed)
        return (x, y, group), mp
    x, y, mp = make_count(model, D, N, seed)
    return (x, y), mp


def run(lib, model, D, C, data, mp, geometry, fma, warm=6, samp=6):
    cfg = wa.default_config(lib, fused_multiply_add=fma, waves_per_chain=geometry[0], elems_per_lane=geometry[1])
    e = wa.DeviceEngine(model, D, C, cfg, params=mp, lib_path=lib, data=data)
    theta = np.random.default_rng(D).normal(size=(C, D)) * 0.3
    lp, g = e.logp_grad(theta)
    e.init_positions(seed=17, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=18)
    e.warmup_step()
    e.warmup_steps(warm - 1)
    e.freeze()
    e.sample_step()
    e.sample_steps(samp - 1)
    e.check()
    out = dict(lp_eval=lp, g_eval=g, pos=e.positions(), logp=e.logp(), depth=e.depths(), grads=e.grad_evals(),
               rng=e.rng_draws(), steps=e.step_sizes(), inv_mass=e.inv_mass())
    e.close()
    return out


# (D = 512 at eight per lane: every slot filled, the scale parameter of glm_scale.h and tau in the last slot of lane 63)
@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", ALL, ids=ALL_IDS)
@pytest.mark.parametrize("D,N,geometry", [(5, 70, (1, 2)), (130, 9, (1, 4)), (1000, 61, (1, 16)), (3, 3, (1, 16)),
                                          (300, 9, (1, 8)), (512, 5, (1, 8))])
@pytest.mark.parametrize("fma", [0, 1])
def test_device_equals_emulation(gpu, model, D, N, geometry, fma):
    sim = simbuild.build()
    data, mp = model_data(model, D, N, seed=D + N)
    C = 4 if geometry[1] == 16 else 8
    dev = run(None, model, D, C, data, mp, geometry, fma)
    emu = run(sim, model, D, C, data, mp, geometry, fma)
    for k in dev:
        assert np.array_equal(dev[k], emu[k], equal_nan=True), k


@pytest.mark.timeout(600)
@pytest.mark.parametrize("model", FLAT, ids=FLAT_IDS)
def test_eight_per_lane_on_the_device(gpu, model):
    D, N = 400, 120
    x, y, mp = make_count(model, D, N, seed=11)
    e = wa.DeviceEngine(model, D, 6, wa.default_config(), params=mp, data=(x, y))
    assert e.lanes == 64 and e.dim_padded == 512
    theta = thetas(model, D, 6, np.random.default_rng(2))
    lp, g = e.logp_grad(theta)
    lp_ref, g_ref = hc.numpy_logp_grad(model, x, y, mp, theta)
    assert np.all(np.abs(lp - lp_ref) <= 1e-11 * (1 + np.abs(lp_ref)))
    for c in range(6):
        assert np.linalg.norm(g[c] - g_ref[c]) <= 1e-11 * (1 + np.linalg.norm(g_ref[c]))
    a = run(None, model, D, 6, (x, y), mp, (1, 8), 1)
    b = run(None, model, D, 6, (x, y), mp, (1, 8), 1)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.all(np.isfinite(a["pos"]))


# ---- posteriors against quadrature ----------------------------------------------------------------------------------
def sample(model, D, data, mp, transform, C=4096, warm=300, T=60):
    """per-chain averages of transform(theta) and of its squares over T draws (2 transitions apart)"""
    e = wa.DeviceEngine(model, D, C, wa.default_config(), params=mp, data=data)
    e.init_positions(seed=5, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=6)
    e.warmup_steps(warm)
    e.freeze()
    draws = []
    for _ in range(T):
        e.sample_steps(2)
        draws.append(transform(e.positions()))
    e.check()
    e.close()
    return np.stack(draws, axis=1)  # [C, T, K]


def rhat(draws):
    C, T, _ = draws.shape
    W = draws.var(axis=1, ddof=1).mean(0)
    B = T * draws.mean(axis=1).var(axis=0, ddof=1)
    return np.sqrt(((T - 1) / T * W + B / T) / W)


def check_moments(draws, mean, var):
    """means and variances within 5 Monte Carlo standard errors: the chains are independent, so the spread of their
    averages gives the standard error (C T / ESS = the variance inflation of one chain's average)"""
    assert np.all(rhat(draws) < 1.01), rhat(draws)
    C = draws.shape[0]
    cm = draws.mean(axis=1)
    cv = ((draws - mean) ** 2).mean(axis=1)
    se_m = cm.std(axis=0, ddof=1) / np.sqrt(C)
    se_v = cv.std(axis=0, ddof=1) / np.sqrt(C)
    assert np.all(np.abs(cm.mean(0) - mean) <= 5 * se_m + 1e-3 * np.sqrt(var)), (cm.mean(0), mean, se_m)
    assert np.all(np.abs(cv.mean(0) - var) <= 5 * se_v + 1e-3 * var), (cv.mean(0), var, se_v)


def grid_moments(logp, a, b):
    w = np.exp(logp - logp.max())
    w /= w.sum()
    A, B = np.meshgrid(a, b, indexing="ij")
    mean = np.array([(w * A).sum(), (w * B).sum()])
    var = np.array([(w * A * A).sum(), (w * B * B).sum()]) - mean * mean
    return mean, var


@pytest.mark.timeout(1800)
def test_poisson_against_quadrature(gpu):
    rng = np.random.default_rng(41)
    N = 40
    x = np.stack([np.ones(N), rng.normal(size=N)], axis=1)
    y = rng.poisson(np.exp(0.8 + 0.5 * x[:, 1])).astype(np.float64)
    mp = np.array([4.0, 4.0])
    a, b = np.linspace(-1.0, 2.5, 701), np.linspace(-1.5, 2.0, 701)
    A, B = np.meshgrid(a, b, indexing="ij")
    eta = A[..., None] + B[..., None] * x[:, 1]
    logp = (y * eta - np.exp(eta)).sum(-1) - A * A / 8 - B * B / 8
    mean, var = grid_moments(logp, a, b)
    assert 6 * np.sqrt(var).max() < 1.7  # (the grid holds the posterior)
    check_moments(sample(POIS, 2, (x, y), mp, lambda th: th), mean, var)


@pytest.mark.timeout(1800)
def test_negative_binomial_against_quadrature(gpu):
    rng = np.random.default_rng(43)
    N = 60
    x = np.ones((N, 1))
    kappa = 0.5
    y = rng.negative_binomial(1 / kappa, (1 / kappa) / (1 / kappa + np.exp(1.2)), size=N).astype(np.float64)
    mp = np.array([4.0, 1.0])  # beta_0 ~ normal(0, 2^2), exp(s) ~ half-normal(1)
    a, s = np.linspace(0.2, 2.2, 601), np.linspace(-4.0, 1.5, 801)
    lg = np.array([[math.lgamma(yy + math.exp(-ss)) - math.lgamma(math.exp(-ss)) for yy in y] for ss in s])  # [S, N]
    A, S = np.meshgrid(a, s, indexing="ij")
    t = A[..., None] + S[..., None]
    phi = np.exp(-S)[..., None]
    ll = lg[None, :, :].sum(-1) + (y * t - (y + phi) * np.logaddexp(0.0, t)).sum(-1)
    logp = ll - A * A / 8 + S - np.exp(2 * S) / 2
    mean, var = grid_moments(logp, a, s)
    check_moments(sample(NB, 2, (x, y), mp, lambda th: th), mean, var)


@pytest.mark.timeout(1800)
def test_linear_sigma_against_quadrature(gpu):
    """beta integrated out: given s, beta | y is Gaussian and p(s | y) = N(y; 0, sigma^2 I + X S2 X^T) p(s)."""
    rng = np.random.default_rng(47)
    N, P = 30, 2
    x = rng.normal(size=(N, P))
    y = x @ np.array([0.6, -0.3]) + 0.8 * rng.normal(size=N)
    s2 = np.array([4.0, 4.0])
    mp = np.append(s2, 2.0)
    s_grid = np.linspace(-2.5, 1.5, 2001)
    logw, means, second = [], [], []
    for s in s_grid:
        sig2 = math.exp(2 * s)
        prec = x.T @ x / sig2 + np.diag(1 / s2)
        cov = np.linalg.inv(prec)
        m = cov @ (x.T @ y) / sig2
        K = sig2 * np.eye(N) + x @ np.diag(s2) @ x.T
        _, logdet = np.linalg.slogdet(K)
        logw.append(-0.5 * (y @ np.linalg.solve(K, y)) - 0.5 * logdet + s - sig2 / (2 * 4.0))
        means.append(np.append(m, s))
        second.append(np.append(np.diag(cov) + m * m, s * s))
    logw = np.array(logw)
    w = np.exp(logw - logw.max())
    w /= w.sum()
    mean = w @ np.array(means)
    var = w @ np.array(second) - mean * mean
    check_moments(sample(LSIG, P + 1, (x, y), mp, lambda th: th), mean, var)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("model", [POIS, NB, LSIG, HPOIS_C], ids=["poisson", "negbin", "linear_sigma", "hier_c"])
def test_drop_in_calls(gpu, model):
    D = 9 if model == HPOIS_C else 4
    data, mp = model_data(model, D, 40, seed=2)
    kw = dict(model_params=mp, num_params=D, num_chains=8, seed=9, min_warmup_iter=40, max_warmup_iter=40,
              min_sampling_iter=30, max_sampling_iter=30)
    host = wa.walnuts_device(model, data=data, **kw)
    kept, chains = wa.walnuts_device(model, data=data, keep_on_device=True, thin=1, **kw)
    assert len(host) == 8
    for a, b in zip(host, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b))
        assert np.all(np.isfinite(np.asarray(a)))
    chains.close()
    sets = [model_data(model, D, n, seed=3 + i)[0] for i, n in enumerate((40, 17, 25))]
    kw["num_chains"] = 12
    many = wa.walnuts_device(model, datasets=sets, **kw)
    kept, views = wa.walnuts_device(model, datasets=sets, keep_on_device=True, thin=1, **kw)
    assert len(many) == 12 and len(views) == 3
    for a, b in zip(many, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b))
        assert np.all(np.isfinite(np.asarray(a)))
    for v in views:
        v.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("model", FLAT, ids=FLAT_IDS)
def test_non_finite_energies(gpu, model):
    """Poisson chains placed where exp(eta) overflows, negative binomial and linear_regression_sigma chains at s = +-800:
    logp_grad returns IEEE values, the transitions treat the energies as every non-finite energy, the other chains stay
    finite and check() is clean."""
    D, C = 5, 8
    x, y, mp = make_count(model, D, 50, seed=4)
    e = wa.DeviceEngine(model, D, C, wa.default_config(), params=mp, data=(x, y))
    e.init_positions(seed=1, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=2)
    pos = e.positions()
    if scale_model(model):
        pos[0, -1], pos[1, -1] = 800.0, -800.0
    else:
        direction = np.sign(x[0])
        pos[0] = direction * 3000.0
        pos[1] = direction * 1000.0
    lp, g = e.logp_grad(pos)
    assert np.all(np.isfinite(lp[2:])) and np.all(np.isfinite(g[2:]))
    for c in (0, 1):
        assert not np.isfinite(lp[c]) or not np.all(np.isfinite(g[c]))
    e.set_positions(pos)
    e.warmup_steps(4)
    e.freeze()
    e.sample_steps(4)
    e.check()
    after = e.positions()
    assert np.all(np.isfinite(after[2:])) and np.all(np.isfinite(e.logp()[2:]))
    e.close()
