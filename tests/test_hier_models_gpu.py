"""GPU tier: hierarchical regression with varying intercepts by group (walnuts_amd/csrc/models/hier_glm.h) on the MI355X.

  * device = emulation, bit for bit, for all four models at (1, 2), (1, 4), (1, 8) and (1, 16), both arithmetic modes,
    over logp_grad, warmup and sampling transitions; (1, 8) also against NumPy and for determinism;
  * hierarchical linear regression against its exact posterior: given s = log tau, (beta, a) is Gaussian and
    p(s | y) is closed-form up to a constant, so a quadrature over s gives the exact posterior means and variances of
    beta, tau and the group effects; both parameterizations' draws of 4 096 chains within MCSE-based bounds;
  * the drop-in call with data=(x, y, group) and with datasets= (three datasets), draws on the host and kept on the
    device;
  * chains started at a non-finite tau: the run ends with IEEE results and check() clean."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
import build as simbuild  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from test_hier_models_sim import (HIER, HLIN, HLIN_C, HLOG, HLOG_C, IDS, make_grouped_datasets, make_hier,  # noqa: E402
                                  numpy_logp_grad)

pytestmark = pytest.mark.gpu


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


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", HIER, ids=IDS)
@pytest.mark.parametrize("P,J,N,geometry", [(3, 6, 70, (1, 2)), (130, 20, 9, (1, 4)), (129, 500, 61, (1, 16)),
                                            (1, 1, 3, (1, 16)),
                                            # eight per lane, rows narrower than theta: nx = 2 of 4 slot pairs; nx = 1,
                                            # effects over three pairs, tau at coordinate 256 (first slot of a pair);
                                            # nx = 3, D = 512, tau in the very last slot
                                            (200, 150, 50, (1, 8)), (100, 156, 13, (1, 8)), (300, 211, 13, (1, 8))])
@pytest.mark.parametrize("fma", [0, 1])
def test_device_equals_emulation(gpu, model, P, J, N, geometry, fma):
    sim = simbuild.build()
    x, y, group, mp = make_hier(model, P, J, N, seed=P + J)
    D = P + J + 1
    C = 4 if geometry[1] == 16 else 8
    dev = run(None, model, D, C, (x, y, group), mp, geometry, fma)
    emu = run(sim, model, D, C, (x, y, group), mp, geometry, fma)
    for k in dev:
        assert np.array_equal(dev[k], emu[k], equal_nan=True), k


@pytest.mark.timeout(600)
@pytest.mark.parametrize("model", HIER, ids=IDS)
def test_eight_per_lane_on_the_device(gpu, model):
    P, J, N = 200, 150, 250
    D = P + J + 1
    x, y, group, mp = make_hier(model, P, J, N, seed=11)
    e = wa.DeviceEngine(model, D, 6, wa.default_config(), params=mp, data=(x, y, group))
    assert e.lanes == 64 and e.dim_padded == 512
    theta = np.random.default_rng(2).normal(size=(6, D)) * 0.2
    lp, g = e.logp_grad(theta)
    lp_ref, g_ref, _, _ = numpy_logp_grad(model, x, y, group, mp, theta)
    assert np.all(np.abs(lp - lp_ref) <= 1e-12 * np.abs(lp_ref).max())
    for c in range(6):
        assert np.linalg.norm(g[c] - g_ref[c]) <= 1e-12 * np.linalg.norm(g_ref[c])
    a = run(None, model, D, 6, (x, y, group), mp, (1, 8), 1)
    b = run(None, model, D, 6, (x, y, group), mp, (1, 8), 1)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.all(np.isfinite(a["pos"]))


def trapezoid(f, s, axis=0):
    ds = np.diff(s)
    f = np.moveaxis(np.asarray(f), axis, 0)
    return np.tensordot(ds, (f[1:] + f[:-1]) / 2, axes=(0, 0))


def exact_posterior(x, y, group, mp, J):
    """Posterior means and variances of beta, tau and the group effects a = tau z of hierarchical linear regression
    (unit noise), by quadrature over s: given s, (beta, a) ~ N(0, diag(s2, tau^2)) a priori and y = W (beta, a) + e
    with W = [x | one-hot(group)], so (beta, a) | s, y is Gaussian and p(s | y) ~ N(y; 0, I + W L W^T) exp(s - tau^2 /
    (2 sigma_tau^2))."""
    N, P = x.shape
    W = np.concatenate([x, np.eye(J)[group]], axis=1)
    s_grid = np.linspace(-9.0, 5.0, 2801)
    logw, means, second = [], [], []
    WtW, Wty = W.T @ W, W.T @ y
    for s in s_grid:
        tau = np.exp(s)
        prec = WtW + np.diag(np.concatenate([1.0 / mp[:P], np.full(J, 1.0 / tau ** 2)]))
        cov = np.linalg.inv(prec)
        m = cov @ Wty
        # log N(y; 0, I + W L W^T) up to a constant, through the precision form
        _, logdet_prec = np.linalg.slogdet(prec)
        logdet_prior = np.sum(np.log(mp[:P])) + J * 2 * s
        logml = -0.5 * (y @ y - Wty @ m) - 0.5 * (logdet_prior + logdet_prec)
        logw.append(logml + s - tau ** 2 / (2 * mp[-1] ** 2))
        means.append(np.concatenate([m, [tau]]))
        second.append(np.concatenate([np.diag(cov) + m * m, [tau * tau]]))
    logw = np.array(logw)
    w = np.exp(logw - logw.max())
    w /= trapezoid(w, s_grid)
    mean = trapezoid(w[:, None] * np.array(means), s_grid)
    var = trapezoid(w[:, None] * np.array(second), s_grid) - mean * mean
    return mean, var  # over [beta (P) | a (J) | tau]


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [HLIN, HLIN_C], ids=["noncentered", "centered"])
def test_linear_against_exact_posterior(gpu, model):
    P, J, N = 2, 6, 48
    rng = np.random.default_rng(31)
    x = rng.normal(size=(N, P))
    group = np.repeat(np.arange(J), N // J).astype(np.int32)
    a_true = rng.normal(size=J) * 0.8
    y = x @ np.array([0.7, -0.4]) + a_true[group] + rng.normal(size=N)
    mp = np.concatenate([np.full(P, 4.0), np.ones(J), [1.0]])
    D = P + J + 1
    mean, var = exact_posterior(x, y, group, mp, J)
    C, T = 4096, 60
    e = wa.DeviceEngine(model, D, C, wa.default_config(), params=mp, data=(x, y, group))
    e.init_positions(seed=5, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=6)
    e.warmup_steps(300)
    e.freeze()
    chain_sum = np.zeros((C, P + J + 1))
    chain_sq = np.zeros((C, P + J + 1))
    for _ in range(T):
        e.sample_steps(2)
        th = e.positions()
        tau = np.exp(th[:, -1])
        u = th[:, P:P + J]
        q = np.concatenate([th[:, :P], u if model == HLIN_C else tau[:, None] * u, tau[:, None]], axis=1)
        chain_sum += q
        chain_sq += (q - mean) ** 2
    e.check()
    e.close()
    # chains are independent: the spread of the per-chain averages gives the Monte Carlo standard error
    cm, cv = chain_sum / T, chain_sq / T
    se_m = cm.std(axis=0, ddof=1) / np.sqrt(C)
    se_v = cv.std(axis=0, ddof=1) / np.sqrt(C)
    assert np.all(np.abs(cm.mean(0) - mean) <= 5 * se_m + 1e-3 * np.sqrt(var)), (cm.mean(0), mean, se_m)
    assert np.all(np.abs(cv.mean(0) - var) <= 5 * se_v + 1e-3 * var), (cv.mean(0), var, se_v)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("model", [HLOG, HLIN_C], ids=["logistic", "linear_c"])
def test_drop_in_calls(gpu, model):
    x, y, group, mp = make_hier(model, 3, 5, 40, seed=2)
    D = 9
    kw = dict(model_params=mp, num_params=D, num_chains=8, seed=9, min_warmup_iter=40, max_warmup_iter=40,
              min_sampling_iter=30, max_sampling_iter=30)
    host = wa.walnuts_device(model, data=(x, y, group), **kw)
    kept, chains = wa.walnuts_device(model, data=(x, y, group), keep_on_device=True, thin=1, **kw)
    assert len(host) == 8
    for a, b in zip(host, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b))
        assert np.all(np.isfinite(np.asarray(a)))
    chains.close()
    sets, _ = make_grouped_datasets(model, 3, 5, [40, 17, 25], seed=3)
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
@pytest.mark.parametrize("model", HIER, ids=IDS)
def test_non_finite_tau(gpu, model):
    """Chains placed at s = 800 (tau = exp(800) = inf) and s = -800 (tau = 0): logp_grad returns IEEE values, the
    transitions treat the energies as every non-finite energy, the chains elsewhere stay finite and check() is clean."""
    x, y, group, mp = make_hier(model, 4, 6, 50, seed=4)
    D = 11
    C = 8
    e = wa.DeviceEngine(model, D, C, wa.default_config(), params=mp, data=(x, y, group))
    e.init_positions(seed=1, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=2)
    pos = e.positions()
    pos[0, -1], pos[1, -1] = 800.0, -800.0
    lp, g = e.logp_grad(pos)
    assert np.all(np.isfinite(lp[2:])) and np.all(np.isfinite(g[2:]))
    assert not np.isfinite(lp[0]) or not np.all(np.isfinite(g[0]))
    e.set_positions(pos)
    e.warmup_steps(4)
    e.freeze()
    e.sample_steps(4)
    e.check()
    after = e.positions()
    assert np.all(np.isfinite(after[2:])) and np.all(np.isfinite(e.logp()[2:]))
    e.close()
