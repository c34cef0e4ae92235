"""GPU tier: hierarchical linear regression with an estimated noise level (walnuts_amd/csrc/models/hier_scale_glm.h) on
the MI355X.

  * device = emulation, bit for bit, for the two models on the shapes of test_hier_scale_sim.py, both arithmetic modes,
    with and without offsets and weights: logp_grad, warmup and sampling transitions, check(); and the outputs of the
    pointwise, predict and replicate hooks: the three matrices, the three folds, the generated chains block and the
    twelve check arrays;
  * (1, 8) also against NumPy and for determinism;
  * the drop-in call with data=(x, y, group) and with datasets=, draws on the host and kept on the device, and
    log_predictive and posterior_predictive_check from the resident draws;
  * hier_linear_regression_sigma and _centered against the exact posterior: given (s_tau, s), (beta, tau u) is Gaussian
    and p(s_tau, s | y) is closed-form up to a constant, so a two-dimensional quadrature (tests/helpers/
    hp_hier_scale_reference.py; its convergence is asserted on the CPU tier too) gives the exact means and variances;
  * chains started at a non-finite tau or scale: the run ends with IEEE results and check() clean."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_hier_scale_reference as hs  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from test_hier_scale_sim import (HSIG, HSIG_C, IDS, MODELS, SHAPE_IDS, SHAPES, data_of, hook_arrays,  # noqa: E402
                                 hook_case, hooks, make_case, numpy_logp_grad, run, same, thetas)

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", MODELS, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("terms", [False, True], ids=["plain", "terms"])
def test_device_equals_emulation(gpu, model, shape, fma, terms):
    sim = simbuild.build()
    P, J, N, geometry = shape
    c = make_case(model, P, J, N, seed=P + J, terms=terms)
    dev = run(None, model, c, 4, geometry, fma)
    emu = run(sim, model, c, 4, geometry, fma)
    assert len(dev) == 9
    for k in dev:
        assert np.array_equal(dev[k], emu[k], equal_nan=True), k


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", MODELS, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_hooks_equal_emulation(gpu, model, shape):
    """the log_lik, predict and replicate matrices, the folds, the generated chains block and the 12 check arrays"""
    sim = simbuild.build()
    P, J, N, geometry = shape
    c = hook_case(model, P, J, N, seed=2 * P + J)
    for fma in (0, 1):
        assert same(hook_arrays(hooks(None, model, c, geometry, fma)), hook_arrays(hooks(sim, model, c, geometry, fma))), fma


@pytest.mark.timeout(600)
@pytest.mark.parametrize("model", MODELS, ids=IDS)
def test_eight_per_lane_on_the_device(gpu, model):
    P, J, N = 200, 150, 250
    c = make_case(model, P, J, N, seed=11, terms=True)
    D = c["D"]
    e = wa.DeviceEngine(model, D, 6, wa.default_config(), params=c["mp"], data=data_of(c), offset=c["offset"],
                        weights=c["weights"])
    assert e.lanes == 64 and e.dim_padded == 512
    theta = thetas(c, 6, seed=2, scale=0.2)
    lp, g = e.logp_grad(theta)
    e.close()
    lp_ref, g_ref = numpy_logp_grad(model, c, theta)
    assert np.all(np.abs(lp - lp_ref) <= 1e-12 * np.abs(lp_ref).max())
    for ch in range(6):
        assert np.linalg.norm(g[ch] - g_ref[ch]) <= 1e-12 * np.linalg.norm(g_ref[ch])
    a = run(None, model, c, 6, (1, 8), 1)
    b = run(None, model, c, 6, (1, 8), 1)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.all(np.isfinite(a["pos"]))


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("model", [HSIG_C, HSIG], ids=["linear_sigma_c", "linear_sigma"])
def test_drop_in_calls(gpu, model):
    c = make_case(model, 3, 5, 40, seed=2)
    D = c["D"]
    kw = dict(model_params=c["mp"], num_params=D, num_chains=8, seed=9, min_warmup_iter=40, max_warmup_iter=40,
              min_sampling_iter=30, max_sampling_iter=30)
    host = wa.walnuts_device(model, data=data_of(c), **kw)
    kept, chains = wa.walnuts_device(model, data=data_of(c), keep_on_device=True, thin=1, **kw)
    assert len(host) == 8
    for a, b in zip(host, kept):
        assert np.asarray(a).shape == (30, D)
        assert np.array_equal(np.asarray(a), np.asarray(b))
        assert np.all(np.isfinite(np.asarray(a)))
    res = wa.log_predictive(model, chains, num_params=D, data=data_of(c))
    assert res.lpd.shape == (40,) and np.all(np.isfinite(res.lpd))
    ppc = wa.posterior_predictive_check(model, chains, num_params=D, seed=3, data=data_of(c))
    assert np.all((ppc.p_value["mean"] >= 0) & (ppc.p_value["mean"] <= 1))
    chains.close()
    sets = [data_of(make_case(model, 3, 5, n, seed=3 + n)) for n in (40, 17, 25)]
    kw["num_chains"] = 12
    many = wa.walnuts_device(model, datasets=sets, **kw)
    kept, views = wa.walnuts_device(model, datasets=sets, keep_on_device=True, thin=1, **kw)
    assert len(many) == 12 and len(views) == 3
    for a, b in zip(many, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b))
        assert np.all(np.isfinite(np.asarray(a)))
    for v in views:
        v.close()


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [HSIG, HSIG_C], ids=["noncentered", "centered"])
def test_linear_sigma_against_exact_posterior(gpu, model):
    """test_hier_slopes_gpu.test_linear_against_exact_posterior with s in place of the second group scale: its chain
    count, iteration counts and MCSE-based acceptance multipliers, unchanged."""
    x, y, group, mp, P, J = hs.exact_case()
    D = P + J + 2
    mean, var = hs.exact_posterior(x, y, group, mp, J)
    C, T = 4096, 60
    e = wa.DeviceEngine(model, D, C, wa.default_config(), params=mp, data=(x, y, group))
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
        tau, sig = np.exp(th[:, D - 2]), np.exp(th[:, D - 1])
        u = th[:, P:P + J]
        q = np.concatenate([th[:, :P], u if model == HSIG_C else tau[:, None] * u, tau[:, None], sig[:, None]], axis=1)
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


@pytest.mark.timeout(600)
@pytest.mark.parametrize("model", MODELS, ids=IDS)
def test_non_finite_tau_or_scale(gpu, model):
    """Chains placed at s_tau = 800 (tau = inf), s_tau = -800 (tau = 0), s = 800 and s = -800: logp_grad returns IEEE
    values, the transitions treat the energies as every non-finite energy, the chains elsewhere stay finite and check()
    is clean."""
    c = make_case(model, 4, 6, 50, seed=4)
    D = c["D"]
    e = wa.DeviceEngine(model, D, 8, wa.default_config(), params=c["mp"], data=data_of(c))
    e.init_positions(seed=1, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=2)
    pos = e.positions()
    pos[0, D - 2], pos[1, D - 2], pos[2, D - 1], pos[3, D - 1] = 800.0, -800.0, 800.0, -800.0
    lp, g = e.logp_grad(pos)
    assert np.all(np.isfinite(lp[4:])) and np.all(np.isfinite(g[4:]))
    for ch in (0, 2, 3):
        assert not np.isfinite(lp[ch]) or not np.all(np.isfinite(g[ch])), ch
    e.set_positions(pos)
    e.warmup_steps(4)
    e.freeze()
    e.sample_steps(4)
    e.check()
    after = e.positions()
    assert np.all(np.isfinite(after[4:])) and np.all(np.isfinite(e.logp()[4:]))
    e.close()
