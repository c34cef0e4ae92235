"""GPU tier: many datasets of one data model in one engine, on the MI355X.

  * device = emulation, bit for bit, for batched engines at (1, 2), (1, 4), (1, 8) and (1, 16), both arithmetic modes;
  * (1, 8) with four datasets: batched = standalone engines on the device, bit for bit;
  * the per-dataset statistics = standalone device engines' pooled ones, bit for bit, at 300 chains per dataset (each
    dataset's 256-chain runs start at its own offset);
  * an observation block over 4 GiB after padding (a 32-bit byte offset would wrap): gradients of the last datasets'
    chains against the high-precision reference, and a short run that is finite and deterministic;
  * linear regression on datasets with distinct coefficients through walnuts_device(datasets=..., keep_on_device=True):
    each dataset's MarkovChains view against its exact conjugate posterior."""
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
from test_data_models_sim import LIN, LOG  # noqa: E402
from test_datasets_sim import (DIM, check_statistics_per_dataset, compare_blocks, config, dataset_sizes, drive,  # noqa: E402
                               make_datasets)

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", [LIN, LOG])
@pytest.mark.parametrize("geometry", [(1, 2), (1, 4), (1, 8), (1, 16)])
@pytest.mark.parametrize("fma", [0, 1])
def test_device_equals_emulation(gpu, model, geometry, fma):
    sim = simbuild.build()
    epl = geometry[1]
    D, k = DIM[epl], 2
    datasets, s2 = make_datasets(model, D, dataset_sizes(epl, 2), seed=60 + epl)
    runs = []
    for lib in (None, sim):
        e = wa.DeviceEngine(model, D, 3 * k, config(lib, geometry, fma), params=s2, lib_path=lib, datasets=datasets)
        theta = np.random.default_rng(D).normal(size=(3 * k, D)) * 0.3
        lp, g = e.logp_grad(theta)
        runs.append([dict(lp=lp, g=g)] + drive(e, 0))
        e.close()
    for a, b in zip(*runs):
        for key in a:
            assert np.array_equal(a[key], b[key], equal_nan=True), key


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [LIN, LOG])
@pytest.mark.parametrize("fma", [0, 1])
def test_eight_per_lane_equals_standalone_engines(gpu, model, fma):
    geometry, D, k = (1, 8), 300, 3
    datasets, s2 = make_datasets(model, D, [1, 4, 5, 11], seed=80)
    cfg = config(None, geometry, fma)
    e = wa.DeviceEngine(model, D, 4 * k, cfg, params=s2, datasets=datasets)
    batched = drive(e, 0)
    for g, d in enumerate(datasets):
        alone = wa.DeviceEngine(model, D, k, cfg, params=s2, data=d)
        compare_blocks(batched, drive(alone, g * k), g, k)
        alone.close()
    e.close()


@pytest.mark.timeout(1800)
def test_statistics_per_dataset_on_device(gpu):
    check_statistics_per_dataset(None, 300)


@pytest.mark.timeout(3600)
def test_block_over_4_gib(gpu):
    G, k, D, N = 4096, 4, 100, 1100  # rows padded to 128 doubles: 4096 * 1100 * 1 KiB = 4.3 GiB
    rng = np.random.default_rng(3)
    x = rng.normal(size=(G * N, D)) / np.sqrt(D)
    beta = rng.normal(size=(G, D))
    eta = np.einsum("gnd,gd->gn", x.reshape(G, N, D), beta).reshape(-1)
    y = (rng.random(G * N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    del eta
    datasets = [(x[g * N:(g + 1) * N], y[g * N:(g + 1) * N]) for g in range(G)]
    s2 = np.full(D, 4.0)
    assert G * N * 128 * 8 > 4 * 2**30
    cfg = wa.default_config(fused_multiply_add=1)
    e = wa.DeviceEngine(LOG, D, G * k, cfg, params=s2, datasets=datasets)
    assert e.dim_padded == 128
    theta = np.random.default_rng(4).normal(size=(G * k, D)) * 0.1
    lp, g = e.logp_grad(theta)
    for ds in (G - 1, G - 2, G // 2):  # datasets beyond the first 4 GiB (and one inside)
        rows = slice(ds * k, ds * k + 2)
        xd, yd = datasets[ds]
        assert hp.error_ratio(lp[rows], g[rows], hp.glm_case(LOG, xd, yd, s2, theta[rows], 2)) <= 1.0, ds
    e.close()

    def short():
        eng = wa.DeviceEngine(LOG, D, G * k, cfg, params=s2, datasets=datasets)
        eng.init_positions(seed=5, chain_offset=0, scale=0.3)
        eng.init_masses_from_grad(1e-5)
        eng.adapt_step(seed=6)
        eng.warmup_steps(2)
        eng.freeze()
        eng.sample_steps(2)
        eng.check()
        out = eng.positions(), eng.logp(), eng.grad_evals()
        eng.close()
        return out

    a, b = short(), short()
    assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1]))
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def mcse_mean(z):  # [k, S]: per-chain means are independent; their spread gives the standard error
    m = z.mean(axis=1)
    return m.std(ddof=1) / np.sqrt(len(m))


@pytest.mark.timeout(1800)
def test_linear_regression_posteriors_per_dataset(gpu):
    G, k, D = 8, 512, 6
    rng = np.random.default_rng(12)
    s2 = np.full(D, 4.0)
    datasets, truth = [], []
    for g in range(G):
        n = 30 + 20 * g
        x = rng.normal(size=(n, D))
        x[:, 0] = 1.0
        beta = rng.normal(size=D) * (1 + g)  # distinct coefficients per dataset
        y = x @ beta + rng.normal(size=n)
        cov = np.linalg.inv(x.T @ x + np.diag(1.0 / s2))
        datasets.append((x, y))
        truth.append((cov @ (x.T @ y), cov))
    results, views = wa.walnuts_device(LIN, model_params=s2, num_params=D, num_chains=G * k, seed=3, init_radius=0.5,
                                       datasets=datasets, keep_on_device=True, thin=1, min_warmup_iter=1000,
                                       max_warmup_iter=1000, min_sampling_iter=300, max_sampling_iter=300)
    assert len(views) == G
    for g, (v, (mu, cov)) in enumerate(zip(views, truth)):
        assert v.num_chains() == k
        draws = np.array([np.asarray(r) for r in results[g * k:(g + 1) * k]])  # [k, S, D]
        assert np.allclose(v.mean(), draws.reshape(-1, D).mean(axis=0), rtol=1e-10, atol=1e-12)
        sd = np.sqrt(np.diag(cov))
        for i in range(D):
            zi = (draws[:, :, i] - mu[i]) / sd[i]
            assert abs(zi.mean()) <= 5 * mcse_mean(zi), (g, i)
        var = v.sample_variance()
        assert np.all(np.abs(var / np.diag(cov) - 1.0) <= 0.1), (g, var / np.diag(cov), v.r_hat(),
                                                                  draws.var(axis=1).mean(axis=0) / np.diag(cov))
