"""GPU tier: simulated replicates and posterior predictive checks on the device (walnuts_amd/csrc/wn_replicate.h) -- bit
for bit against the workgroup emulation of the same source, the CPU tier's purity, reduction, invariance and NaN checks
run on the device, and end to end against the closed-form posterior predictive of a linear regression."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_math_reference as hm  # noqa: E402
import hp_weighted_reference as hw  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from test_pointwise_sim import GEOMETRIES  # noqa: E402
from test_replicate_sim import (IDS, MODELS, NB, bits, check_generated_quantiles, check_invariance,  # noqa: E402
                                check_nan_rule_and_masks, check_purity, check_reduction, check_seeds_and_streams,
                                check_wrappers, rep_case)

pytestmark = pytest.mark.gpu
LIN = hw.LIN


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


@pytest.mark.parametrize("model", MODELS, ids=IDS)
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("fma", [0, 1])
def test_device_equals_emulation(gpu, sim, model, geometry, fma):
    """the matrix of every chain's draws, both generated blocks and all 12 check arrays with and without the mask: 4
    chains of ragged length <= 5 in 2 blocks"""
    for N in (1, 63, 65):
        a, b = bits(rep_case(None, model, geometry, fma, N=N)), bits(rep_case(sim, model, geometry, fma, N=N))
        assert len(a) == len(b) == 4 + 4 + 2 + 2
        for x, y in zip(a, b):
            assert hm.same_bits(x, y), (N, x.shape)


@pytest.mark.parametrize("model", MODELS, ids=IDS)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_purity_and_reduction(gpu, model, geometry):
    f = rep_case(None, model, geometry, 1)
    check_purity(None, f)
    check_reduction(f)
    if model == NB:
        check_generated_quantiles(f)


def test_invariance_under_grid_mask_and_row_order(gpu, monkeypatch):
    check_invariance(None, monkeypatch)


@pytest.mark.parametrize("geometry", GEOMETRIES[1:])
def test_invariance_at_the_wider_geometries(gpu, monkeypatch, geometry):
    check_invariance(None, monkeypatch, geometry)


def test_seeds_ids_and_the_engines_own_streams(gpu):
    check_seeds_and_streams(None)


def test_nan_rule_one_live_row_and_an_all_masked_block(gpu):
    check_nan_rule_and_masks(None)


@pytest.mark.parametrize("geometry", GEOMETRIES[1:])
def test_nan_rule_and_masks_at_the_wider_geometries(gpu, geometry):
    check_nan_rule_and_masks(None, geometry)


def test_wrappers(gpu):
    check_wrappers(None)


def test_exact_replicates_of_linear_regression(gpu):
    """The fit of test_predict_gpu.test_exact_prediction_of_linear_regression: unit-noise linear regression, D = 8, 12 fit
    rows, 64 new rows, 1 024 chains, 100 + 100 transitions, seed 5, draws resident.  The posterior is normal(mu, Sigma),
    so a replicate of a new row x_n is normal(x_n . mu, 1 + x_n' Sigma x_n): its mean and variance over all draws lie
    within 5 SE_n of these, SE_n the standard deviation of the statistic over the 16 chain_blocks views divided by 4.
    (Each view is replicated under a seed of its own: a view numbers its chains from 0, so under one seed the 16 views
    would share their noise and the spread between them would leave it out.)  The noise-free variance x_n' Sigma x_n
    lies more than 5 SE_n away for every row, so replicates that forgot the observation noise fail.  The observations
    were simulated from the model, so the posterior predictive p-value of their sum lies inside (0.01, 0.99)."""
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
    gen = wa.replicate_draws(LIN, chains, num_params=D, data=x_out, seed=11)
    assert gen.num_chains() == C and gen.dims() == N and gen.num_draws() == C * S
    mean, var = gen.mean(), gen.sample_variance()
    views = chains.chain_blocks(B, S, np.full(C, S))
    per_view = [wa.replicate_draws(LIN, v_, num_params=D, data=x_out, seed=100 + b) for b, v_ in enumerate(views)]
    for name, got, exact, stat in (("mean", mean, center, lambda g: g.mean()),
                                   ("var", var, 1.0 + spread, lambda g: g.sample_variance())):
        se = np.stack([stat(g) for g in per_view]).std(axis=0, ddof=1) / 4.0
        z = np.abs(got - exact) / se
        print(f"max |{name} - exact| / SE: {z.max():.3f}")
        assert np.all(z <= 5.0), (name, z.max())
        if name == "var":
            assert np.all(np.abs(got - spread) > 5.0 * se)
    res = wa.posterior_predictive_check(LIN, chains, num_params=D, data=(x_fit, y_fit), seed=11)
    p = res.p_value["sum"]
    print("posterior predictive p-value of sum:", p, "invalid", res.invalid)
    assert p.shape == (1,) and 0.01 < p[0] < 0.99 and res.invalid.tolist() == [0]
    assert res.rep["sum"].shape == (C, S) and not np.isnan(res.rep["sum"]).any()
