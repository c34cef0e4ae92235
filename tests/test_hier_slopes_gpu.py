"""GPU tier: hierarchical regression with varying intercepts and slopes by group (walnuts_amd/csrc/models/
hier_slopes_glm.h) on the MI355X.

  * device = emulation, bit for bit, for the three links on the shapes of test_hier_slopes_sim.py, both arithmetic
    modes, with and without offsets and weights: logp_grad, warmup and sampling transitions, and the outputs of the
    pointwise, predict and replicate hooks;
  * one varying coefficient (varying=1) = MODEL_HIER_*, bit for bit, at every one-wavefront geometry;
  * (1, 8) also against NumPy and for determinism;
  * the drop-in call with data=(x, y, group), varying=2 and with datasets=, draws on the host and kept on the device;
  * linear, Q = 2, against its exact posterior: given (s_0, s_1), (beta, tau_q u_q) is Gaussian and p(s | y) is
    closed-form up to a constant, so a two-dimensional quadrature gives the exact means and variances."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
import build as simbuild  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from test_hier_slopes_sim import (IDS, SHAPE_IDS, SHAPES, SIBLING, SLIN, SLOG, SLOPES, config, data_of, hook_arrays,  # noqa: E402
                                  hooks, make_slopes, numpy_parts, run, same, thetas)

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", SLOPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("terms", [False, True], ids=["plain", "terms"])
def test_device_equals_emulation(gpu, model, shape, fma, terms):
    sim = simbuild.build()
    P, J, Q, N, geometry = shape
    c = make_slopes(model, P, J, Q, N, seed=P + J + Q, terms=terms)
    dev = run(None, model, c, 4, geometry, fma)
    emu = run(sim, model, c, 4, geometry, fma)
    for k in dev:
        assert np.array_equal(dev[k], emu[k], equal_nan=True), k


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", SLOPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_hooks_equal_emulation(gpu, model, shape):
    """the log_lik, predict and replicate matrices, the folds, the generated chains block and the 12 check arrays"""
    sim = simbuild.build()
    P, J, Q, N, geometry = shape
    c = make_slopes(model, P, J, Q, N, seed=2 * P + J, terms=True)
    c["offset"][N - 1] = 0.25   # (the hooks apply no weights: every row is evaluated)
    for fma in (0, 1):
        assert same(hook_arrays(hooks(None, model, c, geometry, fma)), hook_arrays(hooks(sim, model, c, geometry, fma))), fma


def drive_both(model, c, geometry, fma, C=6):
    """the slopes model at varying=1 and its MODEL_HIER_* sibling through logp_grad, warmup and sampling"""
    out = []
    for m in (model, SIBLING[model]):
        kw = dict(varying=1) if m == model else {}
        e = wa.DeviceEngine(m, c["D"], C, config(None, geometry, fma), params=c["mp"], data=data_of(c), offset=c["offset"],
                            weights=c["weights"], **kw)
        lp, g = e.logp_grad(thetas(c, C, seed=3))
        e.init_positions(seed=17, chain_offset=0, scale=0.5)
        e.init_masses_from_grad(1e-5)
        e.adapt_step(seed=18)
        e.warmup_step()
        e.warmup_steps(5)
        e.freeze()
        e.sample_steps(6)
        e.check()
        out.append(dict(lp=lp, g=g, pos=e.positions(), logp=e.logp(), depth=e.depths(), grads=e.grad_evals(),
                        rng=e.rng_draws(), steps=e.step_sizes(), inv_mass=e.inv_mass()))
        e.close()
    return out


@pytest.mark.timeout(900)
@pytest.mark.parametrize("model", SLOPES, ids=IDS)
@pytest.mark.parametrize("fma", [0, 1])
def test_one_varying_coefficient_is_the_hier_model(gpu, model, fma):
    for (P, J, N, geometry) in ((3, 6, 70, (1, 2)), (130, 20, 9, (1, 4)), (200, 150, 50, (1, 8)), (129, 500, 61, (1, 16))):
        for terms in (False, True):
            c = make_slopes(model, P, J, 1, N, seed=P + J, terms=terms)
            a, b = drive_both(model, c, geometry, fma, C=4 if geometry[1] == 16 else 6)
            for k in b:
                assert np.array_equal(a[k], b[k], equal_nan=True), (geometry, terms, k)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("model", SLOPES, ids=IDS)
def test_eight_per_lane_on_the_device(gpu, model):
    P, J, Q, N = 200, 100, 2, 250
    c = make_slopes(model, P, J, Q, N, seed=11, terms=True)
    D = c["D"]
    e = wa.DeviceEngine(model, D, 6, wa.default_config(), params=c["mp"], data=data_of(c), offset=c["offset"],
                        weights=c["weights"], varying=Q)
    assert e.lanes == 64 and e.dim_padded == 512
    theta = thetas(c, 6, seed=2, scale=0.2)
    lp, g = e.logp_grad(theta)
    e.close()
    ref = numpy_parts(model, c, theta)
    assert np.all(np.abs(lp - ref["lp"]) <= 1e-12 * np.abs(ref["lp"]).max())
    for ch in range(6):
        assert np.linalg.norm(g[ch] - ref["g"][ch]) <= 1e-12 * np.linalg.norm(ref["g"][ch])
    a = run(None, model, c, 6, (1, 8), 1)
    b = run(None, model, c, 6, (1, 8), 1)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.all(np.isfinite(a["pos"]))


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("model", [SLOG, SLIN], ids=["logistic", "linear"])
def test_drop_in_calls(gpu, model):
    c = make_slopes(model, 3, 5, 2, 40, seed=2)
    D = c["D"]
    kw = dict(model_params=c["mp"], num_params=D, num_chains=8, seed=9, min_warmup_iter=40, max_warmup_iter=40,
              min_sampling_iter=30, max_sampling_iter=30, varying=2)
    host = wa.walnuts_device(model, data=data_of(c), **kw)
    kept, chains = wa.walnuts_device(model, data=data_of(c), keep_on_device=True, thin=1, **kw)
    assert len(host) == 8
    for a, b in zip(host, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b))
        assert np.all(np.isfinite(np.asarray(a)))
    chains.close()
    sets = [data_of(make_slopes(model, 3, 5, 2, n, seed=3 + n)) for n in (40, 17, 25)]
    kw["num_chains"] = 12
    many = wa.walnuts_device(model, datasets=sets, **kw)
    kept, views = wa.walnuts_device(model, datasets=sets, keep_on_device=True, thin=1, **kw)
    assert len(many) == 12 and len(views) == 3
    for a, b in zip(many, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b))
        assert np.all(np.isfinite(np.asarray(a)))
    for v in views:
        v.close()


def trapezoid_weights(s):
    w = np.zeros_like(s)
    ds = np.diff(s)
    w[:-1] += ds / 2
    w[1:] += ds / 2
    return w


def exact_moments(x, y, group, mp, J, step):
    """Means and variances of [beta (P) | tau_0 u_0 (J) | tau_1 u_1 (J) | tau_0, tau_1] of hierarchical linear regression
    (unit noise) with a varying intercept and a varying slope of x_0, by a trapezoid rule of step `step` over
    (s_0, s_1): given s, (beta, a_0, a_1) ~ N(0, diag(s2, tau_0^2, tau_1^2)) a priori and y = W (beta, a) + e with
    W = [x | onehot | onehot * x_0], so (beta, a) | s, y is Gaussian and
    p(s | y) ~ N(y; 0, I + W L W^T) prod_q exp(s_q - tau_q^2 / (2 sigma_q^2))."""
    N, P = x.shape
    onehot = np.eye(J)[group]
    W = np.concatenate([x, onehot, onehot * x[:, :1]], axis=1)
    WtW, Wty = W.T @ W, W.T @ y
    s = np.arange(-12.0, 3.0 + step / 2, step)   # tau from 6e-6 (weight ~ tau) to 20 (exp(-200 / sigma^2))
    w1 = trapezoid_weights(s)
    s0, s1 = (a.reshape(-1) for a in np.meshgrid(s, s, indexing="ij"))
    wq = np.outer(w1, w1).reshape(-1)
    t0, t1 = np.exp(s0), np.exp(s1)
    G = s0.size
    diag = np.concatenate([np.broadcast_to(1.0 / mp[:P], (G, P)), np.repeat((1.0 / t0 ** 2)[:, None], J, axis=1),
                           np.repeat((1.0 / t1 ** 2)[:, None], J, axis=1)], axis=1)
    prec = WtW[None] + diag[:, :, None] * np.eye(P + 2 * J)[None]
    cov = np.linalg.inv(prec)
    m = cov @ Wty
    _, logdet_prec = np.linalg.slogdet(prec)
    logdet_prior = np.sum(np.log(mp[:P])) + 2 * J * (s0 + s1)
    logml = -0.5 * (y @ y - m @ Wty) - 0.5 * (logdet_prior + logdet_prec)
    logw = logml + (s0 - t0 ** 2 / (2 * mp[-2] ** 2)) + (s1 - t1 ** 2 / (2 * mp[-1] ** 2))
    w = wq * np.exp(logw - logw.max())
    w /= w.sum()
    first = np.concatenate([m, t0[:, None], t1[:, None]], axis=1)
    second = np.concatenate([np.diagonal(cov, axis1=1, axis2=2) + m * m, (t0 * t0)[:, None], (t1 * t1)[:, None]], axis=1)
    mean = w @ first
    return mean, w @ second - mean * mean


def exact_posterior_slopes(x, y, group, mp, J):
    """exact_moments on a grid that is fine enough: halving the step moves no value by more than 1e-4 of its posterior
    standard deviation (variances: of the variance)."""
    mean, var = exact_moments(x, y, group, mp, J, 0.125)
    mean2, var2 = exact_moments(x, y, group, mp, J, 0.0625)
    assert np.all(np.abs(mean2 - mean) <= 1e-4 * np.sqrt(var2)), np.max(np.abs(mean2 - mean) / np.sqrt(var2))
    assert np.all(np.abs(var2 - var) <= 1e-4 * np.minimum(var2, np.sqrt(var2))), np.max(np.abs(var2 - var) / var2)
    return mean2, var2


def exact_case():
    P, J, N = 2, 5, 40
    rng = np.random.default_rng(31)
    x = rng.normal(size=(N, P))
    group = np.repeat(np.arange(J), N // J).astype(np.int32)
    a0, a1 = 0.8 * rng.normal(size=J), 0.6 * rng.normal(size=J)
    y = x @ np.array([0.7, -0.4]) + a0[group] + a1[group] * x[:, 0] + rng.normal(size=N)
    mp = np.concatenate([np.full(P, 4.0), np.ones(2 * J), [1.0, 1.0]])
    return x, y, group, mp, P, J


@pytest.mark.timeout(1800)
def test_linear_against_exact_posterior(gpu):
    x, y, group, mp, P, J = exact_case()
    D = P + 2 * (J + 1)
    mean, var = exact_posterior_slopes(x, y, group, mp, J)
    C, T = 4096, 60
    e = wa.DeviceEngine(SLIN, D, C, wa.default_config(), params=mp, data=(x, y, group), varying=2)
    e.init_positions(seed=5, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=6)
    e.warmup_steps(300)
    e.freeze()
    chain_sum = np.zeros((C, D))
    chain_sq = np.zeros((C, D))
    for _ in range(T):
        e.sample_steps(2)
        th = e.positions()
        tau = np.exp(th[:, D - 2:])
        q = np.concatenate([th[:, :P], tau[:, :1] * th[:, P:P + J], tau[:, 1:] * th[:, P + J:P + 2 * J], tau], axis=1)
        chain_sum += q
        chain_sq += (q - mean) ** 2
    e.check()
    e.close()
    # chains are independent: the spread of the per-chain averages gives the Monte Carlo standard error
    cm, cv = chain_sum / T, chain_sq / T
    se_m = cm.std(axis=0, ddof=1) / np.sqrt(C)
    se_v = cv.std(axis=0, ddof=1) / np.sqrt(C)
    print("mean error / allowance", np.abs(cm.mean(0) - mean) / (5 * se_m + 1e-3 * np.sqrt(var)))
    print("var error / allowance", np.abs(cv.mean(0) - var) / (5 * se_v + 1e-3 * var))
    assert np.all(np.abs(cm.mean(0) - mean) <= 5 * se_m + 1e-3 * np.sqrt(var)), (cm.mean(0), mean, se_m)
    assert np.all(np.abs(cv.mean(0) - var) <= 5 * se_v + 1e-3 * var), (cv.mean(0), var, se_v)
