"""GPU tier: the pointwise log-likelihood and the predictive fold on the device (walnuts_amd/csrc/wn_pointwise.h) --
bit for bit against the workgroup emulation of the same source, against the high-precision reference
(tests/helpers/hp_pointwise_reference.py), end to end behind walnuts_device(weight_sets=, keep_on_device=True), and
against the closed-form predictive density of a linear regression."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_weighted_reference as hw  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from test_pointwise_sim import (SMALL, U, case_for, check_log_lik, numpy_fold, ragged_chains, thetas_for,  # noqa: E402
                                valid_folds)
from test_weights_sim import config, engine, make_case  # noqa: E402

pytestmark = pytest.mark.gpu
LIN, LOG, POIS, NB, LSIG, HLOG = hw.LIN, hw.LOG, hw.POIS, hw.NB, hw.LSIG, hw.HLOG
GEOMETRIES = ((1, 2), (1, 4), (1, 8), (1, 16))


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


@pytest.mark.parametrize("model", [LOG, NB, HLOG], ids=["logistic", "negbin", "hier_logistic"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("fma", [0, 1])
def test_device_equals_emulation(gpu, sim, model, geometry, fma):
    """log_lik and all four outputs of log_predictive: 4 chains of ragged length <= 5, W = 2 weight sets with a mask."""
    epl = geometry[1]
    for N in (63, 65):
        c = case_for(model, SMALL[epl], N, seed=3 * N + model)
        sets = np.stack([(np.arange(N) % 3 != g).astype(np.float64) for g in range(2)])
        got = {}
        for lib in (None, sim):
            draws, ch = ragged_chains(model, c["D"], (5, 3, 4, 1), 17, lib)
            e = engine(lib, model, c, 2, geometry, fma, offset=c["offset"], weight_sets=sets)
            assert e.num_datasets == 2
            got[lib] = (e.log_lik(np.concatenate(draws)),) + e.log_predictive(ch, sets == 0)
            e.close()
        for a, b in zip(got[None], got[sim]):
            assert np.array_equal(a, b, equal_nan=True), (N, np.nanmax(np.abs(a - b)))
        assert np.array_equal(got[None][4], np.where(sets == 0, np.array([[8], [5]]), 0))


@pytest.mark.parametrize("model", [POIS, LSIG], ids=["poisson_exposure", "linear_sigma"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_edge_matrix_against_high_precision(gpu, model, geometry, record_property):
    """The CPU tier's matrix on the device: N at the 64-row pack boundaries, both arithmetic modes, offsets (the Poisson
    exposure), a theta that overflows the Poisson link."""
    record_property("max_error_over_bound", max(check_log_lik(None, model, geometry, N) for N in (1, 63, 64, 65)))


def test_kfold_end_to_end(gpu):
    """The shapes of test_weights_gpu.test_drop_in_call_with_weight_sets: K = 4 refits in one run, draws resident;
    kfold_elpd on the views equals the fold (wn_pointwise.h, in numpy) of DeviceEngine.log_lik over the same draws taken
    from the host results, within the fold's bound."""
    W, k, P, N = 4, 16, 100, 60
    c = make_case(LOG, P, N, seed=33)
    sets = valid_folds(W, N, np.random.default_rng(9))
    results, views = wa.walnuts_device(LOG, weight_sets=sets, keep_on_device=True, thin=1, model_params=c["params"],
                                       num_params=c["D"], num_chains=W * k, seed=9, id=2, init_radius=0.5,
                                       max_trajectory_doublings=5, min_warmup_iter=3, max_warmup_iter=3,
                                       min_sampling_iter=3, max_sampling_iter=3, data=c["data"], offset=c["offset"])
    host = np.array([np.asarray(r) for r in results])  # [C, 3, D]
    kf = wa.kfold_elpd(LOG, views, num_params=c["D"], data=c["data"], weight_sets=sets, offset=c["offset"])
    assert kf.lpd.shape == (N,) and np.all(kf.count == 3 * k) and np.isfinite(kf.elpd) and np.isfinite(kf.se)
    e = wa.DeviceEngine(LOG, c["D"], 1, params=np.ones(c["D"]), data=c["data"], offset=c["offset"])
    T, C = 3 * k, k
    for g in range(W):
        lls = [e.log_lik(host[ch]) for ch in range(g * k, (g + 1) * k)]
        lpd, mean, var = numpy_fold(lls)
        rows = np.concatenate(lls)
        spread, big = rows.max(axis=0) - rows.min(axis=0), np.abs(rows).max(axis=0)
        held = np.flatnonzero(sets[g] == 0)
        lpd_b = 2 * U * ((T + C) * (6 + spread) + 6 * (2 * big + np.log(T) + 1))
        mean_b = 2 * 4 * (T + C) * U * big
        dev = np.abs(rows - rows.mean(axis=0)).max(axis=0)
        var_b = 2 * dev * mean_b * T / (T - 1) + 2 * 8 * (T + C) * U * var
        assert np.all(np.abs(kf.lpd[held] - lpd[held]) <= lpd_b[held]), g
        assert np.all(np.abs(kf.mean[held] - mean[held]) <= mean_b[held]), g
        assert np.all(np.abs(kf.var[held] - var[held]) <= var_b[held]), g
    e.close()


def test_exact_predictive_of_linear_regression(gpu):
    """Linear regression with unit noise, D = 8: the posterior is normal(mu, Sigma), the predictive density of a held-out
    row is N(y_n; x_n . mu, 1 + x_n' Sigma x_n).  1 024 chains, 100 warmup + 100 sampling transitions, draws resident;
    |lpd_n - exact| <= 5 SE_n with SE_n the standard deviation over 16 chain_blocks views of the per-view lpd_n, divided
    by 4 -- and the plug-in value l_n(mu) lies more than 5 SE away for at least half the rows, so a point estimate fails."""
    D, N, C, S, B = 8, 64, 1024, 100, 16
    rng = np.random.default_rng(2024)
    beta = rng.normal(size=D)
    x_fit = rng.normal(size=(12, D))
    y_fit = x_fit @ beta + rng.normal(size=12)
    x_out = rng.normal(size=(N, D))
    y_out = x_out @ beta + rng.normal(size=N)
    s2 = np.full(D, 4.0)
    Sigma = np.linalg.inv(x_fit.T @ x_fit + np.diag(1.0 / s2))
    mu = Sigma @ x_fit.T @ y_fit
    v = 1.0 + np.einsum("nd,de,ne->n", x_out, Sigma, x_out)
    exact = -0.5 * (y_out - x_out @ mu) ** 2 / v - 0.5 * np.log(2 * np.pi * v)
    plug_in = -0.5 * (y_out - x_out @ mu) ** 2 - 0.5 * np.log(2 * np.pi)
    _, chains = wa.walnuts_device(LIN, model_params=s2, num_params=D, num_chains=C, seed=5, id=1, init_radius=0.5,
                                  min_warmup_iter=100, max_warmup_iter=100, min_sampling_iter=S, max_sampling_iter=S,
                                  data=(x_fit, y_fit), keep_on_device=True, thin=0)
    res = wa.log_predictive(LIN, chains, num_params=D, data=(x_out, y_out))
    assert np.all(res.count == C * S)
    views = chains.chain_blocks(B, S, np.full(C, S))
    per_view = np.stack([wa.log_predictive(LIN, v_, num_params=D, data=(x_out, y_out)).lpd for v_ in views])
    se = per_view.std(axis=0, ddof=1) / 4.0
    z = np.abs(res.lpd - exact) / se
    print("max |lpd - exact| / SE:", z.max(), " plug-in:", np.sort(np.abs(plug_in - exact) / se)[N // 2])
    assert np.all(z <= 5.0), z.max()
    assert np.sum(np.abs(plug_in - exact) > 5.0 * se) >= N // 2
