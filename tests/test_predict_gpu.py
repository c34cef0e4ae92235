"""GPU tier: predictions on the device (walnuts_amd/csrc/wn_predict.h) -- bit for bit against the workgroup emulation of
the same source, against the high-precision reference (tests/helpers/hp_predict_reference.py), the stated fold replayed
exactly, and end to end against the closed-form posterior predictive of a linear regression."""
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
from test_pointwise_sim import GEOMETRIES, MAIN, MAIN_IDS, OTHER_IDS, OTHERS  # noqa: E402
from test_predict_sim import (LENGTHS, check_eta_is_pointwise_eta, check_fold_invariance,  # noqa: E402
                              check_fold_is_the_stated_fold, check_generated_chains, check_predict, check_wrappers, download,
                              fold_case)

pytestmark = pytest.mark.gpu
LIN, LOG, NB, HLOG = hw.LIN, hw.LOG, hw.NB, hw.HLOG


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


@pytest.mark.parametrize("model", [LOG, NB, HLOG], ids=["logistic", "negbin", "hier_logistic"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("fma", [0, 1])
def test_device_equals_emulation(gpu, sim, model, geometry, fma):
    """the matrix, the fold's six outputs and one generated block: 4 chains of ragged length <= 5 in 2 blocks, a mask"""
    for N in (63, 65):
        got = {}
        for lib in (None, sim):
            f = fold_case(lib, model, geometry, fma, N=N)
            got[lib] = [a for m in f["matrices"] for a in m] + list(f["fold"]) + download(f["gen"], max(LENGTHS[2:]), LENGTHS[2:])
        assert len(got[None]) == len(got[sim]) == 3 * 4 + 6 + 2
        for a, b in zip(got[None], got[sim]):
            assert np.array_equal(a, b, equal_nan=True), (N, np.nanmax(np.abs(a - b)))


@pytest.mark.parametrize("model", MAIN, ids=MAIN_IDS)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_values_against_high_precision(gpu, model, geometry, record_property):
    """the CPU tier's matrix on the device: N at the 64-row pack boundaries, both arithmetic modes, a theta that
    overflows the Poisson link"""
    record_property("max_error_over_bound", max(check_predict(None, model, geometry, N, sensitivity=N == 65)
                                                for N in (1, 63, 64, 65) + ((129,) if geometry[1] == 2 else ())))


@pytest.mark.parametrize("model", OTHERS, ids=OTHER_IDS)
def test_values_of_the_other_models(gpu, model):
    check_predict(None, model, (1, 2), 65, sensitivity=True)


@pytest.mark.parametrize("model", [LIN, hw.HLIN, hw.HLIN_C], ids=["linear", "hier_linear", "hier_linear_centered"])
def test_eta_is_the_pointwise_eta(gpu, model):
    check_eta_is_pointwise_eta(None, model)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_fold_and_generated_chains(gpu, geometry, monkeypatch):
    f = fold_case(None, LOG, geometry, 1)
    check_fold_is_the_stated_fold(f)
    check_generated_chains(f)
    if geometry[1] == 2:
        check_fold_invariance(None, monkeypatch)


def test_wrappers(gpu):
    check_wrappers(None)


def test_exact_prediction_of_linear_regression(gpu):
    """The fit of test_pointwise_gpu.test_exact_predictive_of_linear_regression: unit-noise linear regression, D = 8, 12
    fit rows, 64 new rows, 1 024 chains, 100 + 100 transitions, seed 5, draws resident.  The posterior is normal(mu,
    Sigma), so for a new row x_n: E eta = E mean = x_n . mu, Var eta = Var mean = x_n' Sigma x_n, the predictive variance
    is 1 + x_n' Sigma x_n and the noise variance is exactly 1.  Each within 5 SE_n, SE_n the standard deviation of the
    statistic over the 16 chain_blocks views divided by 4 -- and the noise alone (1.0) lies more than 5 SE_n from the
    predictive variance for at least half the rows, so a prediction that ignored parameter uncertainty fails."""
    D, N, C, S, B = 8, 64, 1024, 100, 16
    rng = np.random.default_rng(2024)
    beta = rng.normal(size=D)
    x_fit = rng.normal(size=(12, D))
    y_fit = x_fit @ beta + rng.normal(size=12)
    x_out = rng.normal(size=(N, D))
    s2 = np.full(D, 4.0)
    Sigma = np.linalg.inv(x_fit.T @ x_fit + np.diag(1.0 / s2))
    mu = Sigma @ x_fit.T @ y_fit
    center = x_out @ mu
    spread = np.einsum("nd,de,ne->n", x_out, Sigma, x_out)
    _, chains = wa.walnuts_device(LIN, model_params=s2, num_params=D, num_chains=C, seed=5, id=1, init_radius=0.5,
                                  min_warmup_iter=100, max_warmup_iter=100, min_sampling_iter=S, max_sampling_iter=S,
                                  data=(x_fit, y_fit), keep_on_device=True, thin=0)
    res = wa.predict(LIN, chains, num_params=D, data=x_out)
    assert np.all(res.count == C * S) and res.evaluated.all()
    assert np.all(res.noise_var == 1.0)
    views = chains.chain_blocks(B, S, np.full(C, S))
    per_view = [wa.predict(LIN, v_, num_params=D, data=x_out) for v_ in views]
    worst = 0.0
    for name, exact in (("eta_mean", center), ("mean", center), ("eta_var", spread), ("mean_var", spread),
                        ("var", 1.0 + spread)):
        se = np.stack([getattr(p, name) for p in per_view]).std(axis=0, ddof=1) / 4.0
        z = np.abs(getattr(res, name) - exact) / se
        print(f"max |{name} - exact| / SE: {z.max():.3f}")
        worst = max(worst, float(z.max()))
        assert np.all(z <= 5.0), (name, z.max())
    se_var = np.stack([p.var for p in per_view]).std(axis=0, ddof=1) / 4.0
    assert np.sum(np.abs(1.0 - res.var) > 5.0 * se_var) >= N // 2
    print("largest z:", worst)
