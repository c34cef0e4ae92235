"""GPU tier: per-row offsets and weights of the data models and weight sets over one shared block of rows, on the
MI355X.

  * device = emulation, bit for bit, with offsets and weights (a zero-weight row inside a block) at N = B - 1 and B + 1,
    the four one-wavefront geometries, both arithmetic modes: logistic, negative binomial and hierarchical logistic regression;
  * weight sets (W = 4, k = 4): each set's block equals the emulation's;
  * the edge matrix of test_weights_sim.py against the high-precision reference, Poisson with exposure;
  * weighted linear regression with offsets against its exact Gaussian posterior;
  * the drop-in call with weight sets, resident draws and per-set R-hat."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_reference as hp  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from test_datasets_sim import state  # noqa: E402
from test_weights_sim import (HLOG, LIN, LOG, NB, POIS, check_edge_matrix, engine, fold_weights, make_case,  # noqa: E402
                              thetas)

pytestmark = pytest.mark.gpu
GEOMETRIES = ((1, 2), (1, 4), (1, 8), (1, 16))
COLUMNS = {2: 100, 4: 200, 8: 400, 16: 1000}


def short_run(e, theta):
    """logp_grad, then 3 warmup and 3 sampling transitions: everything the engine exposes after each phase"""
    lp, g = e.logp_grad(theta)
    out = [dict(lp=lp, g=g)]
    e.init_positions(seed=11, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=12)
    e.seed_chains(13, 0)
    e.warmup_steps(3)
    out.append(state(e))
    e.freeze()
    e.sample_steps(3)
    e.check()
    s = state(e)
    s.pop("masses")
    out.append(s)
    e.close()
    return out


def assert_same(a, b):
    for u, v in zip(a, b):
        for key in u:
            assert np.array_equal(u[key], v[key], equal_nan=True), key


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [LOG, NB, HLOG], ids=["logistic", "negbin", "hier_logistic"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("fma", [0, 1])
def test_device_equals_emulation(gpu, model, geometry, fma):
    sim = simbuild.build()
    epl = geometry[1]
    B = hp.block_rows(epl)
    for N in (B - 1, B + 1):
        c = make_case(model, COLUMNS[epl], N, seed=90 + N)
        w = c["weights"].copy()
        w[min(1, N - 1)] = 0.0  # a zero-weight row inside the first block
        theta = thetas(model, c["D"], 8, seed=N)
        runs = [short_run(engine(lib, model, c, 8, geometry, fma, offset=c["offset"], weights=w), theta)
                for lib in (None, sim)]
        assert_same(*runs)
        assert np.all(np.isfinite(runs[0][-1]["logp"]))


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_weight_sets_on_device(gpu, geometry):
    sim = simbuild.build()
    epl = geometry[1]
    W, k = 4, 4
    N = 2 * hp.block_rows(epl) + 1
    c = make_case(LOG, COLUMNS[epl], N, seed=70 + epl)
    sets = fold_weights(W, N, np.random.default_rng(8))
    theta = thetas(LOG, c["D"], W * k, seed=5)
    runs = [short_run(engine(lib, LOG, c, W * k, geometry, 1, offset=c["offset"], weight_sets=sets), theta)
            for lib in (None, sim)]
    for g in range(W):
        for u, v in zip(*runs):
            for key in u:
                assert np.array_equal(u[key][g * k:(g + 1) * k], v[key][g * k:(g + 1) * k], equal_nan=True), (g, key)
    pos = runs[0][-1]["pos"]
    assert not np.array_equal(pos[:k], pos[k:2 * k])


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("fma", [0, 1])
def test_poisson_exposure_edges_against_high_precision(gpu, geometry, fma, record_property):
    record_property("max_error_over_bound", check_edge_matrix(None, POIS, geometry, fma))


def mcse_mean(z):  # [C, S]: per-chain means are independent; their spread gives the standard error
    m = z.mean(axis=1)
    return m.std(ddof=1) / np.sqrt(len(m))


def rhat(d):  # [C, S] split-free Gelman-Rubin
    C, S = d.shape
    W = d.var(axis=1, ddof=1).mean()
    B = S * d.mean(axis=1).var(ddof=1)
    return np.sqrt(((S - 1) / S * W + B / S) / W)


@pytest.mark.timeout(1800)
def test_weighted_linear_regression_exact_posterior(gpu):
    """Precision X^T W X + S^-1, mean from X^T W (y - o); the chain counts and z-score criterion of
    test_data_models_gpu.test_linear_regression_exact_posterior.  Half of the rows carry weight 0.1 and the other half 4,
    with different coefficients behind the halves, and the offsets are of the size of the signal: the posterior mean
    that ignores the weights, or the offsets, lies tens of standard errors away (asserted below)."""
    import torch
    D, N, C = 16, 400, 4096
    rng = np.random.default_rng(21)
    x = rng.normal(size=(N, D))
    x[:, 0] = 1.0
    o = rng.normal(size=N)
    w = np.where(np.arange(N) % 2 == 0, 0.1, 4.0)
    beta = rng.normal(size=(2, D))
    y = np.einsum("nd,nd->n", x, beta[np.arange(N) % 2]) + o + rng.normal(size=N)
    s2 = np.full(D, 4.0)
    e = wa.DeviceEngine(LIN, D, C, wa.default_config(), params=s2, data=(x, y), offset=o, weights=w)
    e.init_positions(seed=5, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=6)
    e.warmup_steps(200)
    e.freeze()
    samp = 200
    dev = torch.empty((C, samp, D), dtype=torch.float64, device="cuda")
    e.sample_steps(samp, dev.data_ptr(), samp * D, D)
    e.synchronize()
    e.check()
    draws = dev.cpu().numpy()
    e.close()
    cov = np.linalg.inv((x * w[:, None]).T @ x + np.diag(1.0 / s2))
    mu = cov @ ((x * w[:, None]).T @ (y - o))
    L = np.linalg.cholesky(cov)
    z = np.linalg.solve(L, (draws.reshape(-1, D) - mu).T).T.reshape(C, -1, D)
    for i in range(D):
        zi = z[:, :, i]
        assert abs(zi.mean()) <= 5 * mcse_mean(zi), i
        assert abs(zi.var() - 1.0) <= 0.03, (i, zi.var())
        assert rhat(zi) <= 1.01, i
    corr = np.corrcoef(z.reshape(-1, D).T)  # (whitened by the weighted covariance: a wrong off-diagonal of X^T W X shows)
    assert np.max(np.abs(corr - np.eye(D))) < 0.02
    # what ignoring a field would give is far away, in standard errors of the mean of all draws
    se = np.sqrt(np.diag(cov) / (C * samp))
    for ww, oo in ((np.ones(N), o), (w, np.zeros(N))):
        cov_u = np.linalg.inv((x * ww[:, None]).T @ x + np.diag(1.0 / s2))
        mu_u = cov_u @ ((x * ww[:, None]).T @ (y - oo))
        assert np.max(np.abs(mu_u - mu) / se) > 50


@pytest.mark.timeout(1800)
def test_drop_in_call_with_weight_sets(gpu):
    W, k, P, N = 4, 16, 100, 60
    c = make_case(LOG, P, N, seed=33)
    sets = fold_weights(W, N, np.random.default_rng(9))
    args = dict(model_params=c["params"], num_params=c["D"], num_chains=W * k, seed=9, id=2, init_radius=0.5,
                max_trajectory_doublings=5, min_warmup_iter=3, max_warmup_iter=3, min_sampling_iter=3,
                max_sampling_iter=3, data=c["data"], offset=c["offset"])
    results, views = wa.walnuts_device(LOG, weight_sets=sets, keep_on_device=True, thin=1, **args)
    assert len(views) == W and len(results) == W * k
    host = np.array([np.asarray(r) for r in results])  # [C, 3, D]
    for g, v in enumerate(views):
        assert v.num_chains() == k and v.dims() == c["D"]
        block = host[g * k:(g + 1) * k]
        assert np.allclose(v.mean(), block.reshape(-1, c["D"]).mean(axis=0), rtol=1e-10, atol=1e-12)
        r = v.r_hat()
        assert r.shape == (c["D"],) and np.all(np.isfinite(r))
        # set g's block is what the call with weights=sets[g] writes for the same chain ids
        alone = np.array([np.asarray(r_) for r_ in wa.walnuts_device(LOG, weights=sets[g], **args)])
        assert np.array_equal(block, alone[g * k:(g + 1) * k]), g
