"""GPU tier: varying intercepts and slopes by group with an estimated noise level (walnuts_amd/csrc/models/
hier_slopes_scale_glm.h: hier_linear_regression_slopes_sigma) on the MI355X.

  * device = emulation, bit for bit, on the nine shapes of test_hier_slopes_scale_sim.py, both arithmetic modes, with and
    without offsets and weights: logp_grad, warmup and sampling transitions, check(); and the outputs of the pointwise,
    predict and replicate hooks on the five hook shapes;
  * varying=1 against hier_linear_regression_sigma on the device, at all four geometries;
  * (1, 8) also against NumPy and for determinism;
  * the drop-in call with data=(x, y, group) and with datasets=, draws on the host and kept on the device, and
    log_predictive, psis_loo, predict and posterior_predictive_check from the resident draws;
  * against the exact posterior: given (s_0, s_1, s), (beta, tau_q u_q) is Gaussian and p(s_0, s_1, s | y) is closed-form up
    to a constant, so a three-dimensional quadrature (tests/helpers/hp_hier_slopes_scale_reference.py; its convergence is
    asserted on the CPU tier too) gives the exact means and variances;
  * chains started at a non-finite tau_q or scale: the run ends with IEEE results and check() clean."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_hier_slopes_scale_reference as hss  # noqa: E402
import hp_reference as hp  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from test_hier_slopes_scale_sim import (HOOK_SHAPE_IDS, HOOK_SHAPES, HSIG, MODEL, SHAPE_IDS, SHAPES,  # noqa: E402
                                        SIM_GEOMETRIES, data_of, hook_arrays, hook_case, hooks, make_case,
                                        numpy_logp_grad, run, same, thetas)

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("terms", [False, True], ids=["plain", "terms"])
def test_device_equals_emulation(gpu, shape, fma, terms):
    sim = simbuild.build()
    P, J, Q, N, geometry = shape
    c = make_case(P, J, Q, N, seed=P + J + Q, terms=terms)
    dev = run(None, c, 4, geometry, fma)
    emu = run(sim, c, 4, geometry, fma)
    assert len(dev) == 9
    for k in dev:
        assert np.array_equal(dev[k], emu[k], equal_nan=True), k


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("shape", HOOK_SHAPES, ids=HOOK_SHAPE_IDS)
def test_hooks_equal_emulation(gpu, shape):
    """the log_lik, predict and replicate matrices, the folds, the generated chains block and the 12 check arrays"""
    sim = simbuild.build()
    P, J, Q, N, geometry = shape
    c = hook_case(P, J, Q, N, seed=2 * P + J)
    for fma in (0, 1):
        assert same(hook_arrays(hooks(None, c, geometry, fma)), hook_arrays(hooks(sim, c, geometry, fma))), fma


@pytest.mark.timeout(600)
@pytest.mark.parametrize("geometry", SIM_GEOMETRIES, ids=lambda g: f"nw{g[0]}_epl{g[1]}")
def test_one_varying_coefficient_is_hier_linear_regression_sigma_on_the_device(gpu, geometry):
    """varying=1 gives the bits of MODEL_HIER_LINEAR_REGRESSION_SIGMA: logp_grad, transitions, the hooks"""
    epl = geometry[1]
    P, J = {2: (3, 6), 4: (130, 7), 8: (200, 150), 16: (200, 40)}[epl]
    N = 2 * hp.block_rows(epl) + 3
    for terms in (False, True):
        c = make_case(P, J, 1, N, seed=40 + epl, terms=terms)
        for fma in (0, 1):
            a, b = run(None, c, 4, geometry, fma, model=MODEL), run(None, c, 4, geometry, fma, model=HSIG)
            for k in a:
                assert np.array_equal(a[k], b[k], equal_nan=True), (terms, fma, k)
    c = hook_case(P, J, 1, N, seed=8)
    assert same(hook_arrays(hooks(None, c, geometry, 1)), hook_arrays(hooks(None, c, geometry, 1, model=HSIG)))


@pytest.mark.timeout(600)
def test_eight_per_lane_on_the_device(gpu):
    P, J, Q, N = 120, 60, 3, 250
    c = make_case(P, J, Q, N, seed=11, terms=True)
    D = c["D"]
    e = wa.DeviceEngine(MODEL, D, 6, wa.default_config(), params=c["mp"], data=data_of(c), offset=c["offset"],
                        weights=c["weights"], varying=Q)
    assert e.lanes == 64 and e.dim_padded == 512
    theta = thetas(c, 6, seed=2, scale=0.2)
    lp, g = e.logp_grad(theta)
    e.close()
    lp_ref, g_ref = numpy_logp_grad(c, theta)
    assert np.all(np.abs(lp - lp_ref) <= 1e-12 * np.abs(lp_ref).max())
    for ch in range(6):
        assert np.linalg.norm(g[ch] - g_ref[ch]) <= 1e-12 * np.linalg.norm(g_ref[ch])
    a = run(None, c, 6, (1, 8), 1)
    b = run(None, c, 6, (1, 8), 1)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.all(np.isfinite(a["pos"]))


@pytest.mark.timeout(1200)
def test_drop_in_calls(gpu):
    P, J, Q, N = 3, 5, 2, 40
    c = make_case(P, J, Q, N, seed=2)
    D = c["D"]
    kw = dict(model_params=c["mp"], num_params=D, num_chains=8, seed=9, min_warmup_iter=40, max_warmup_iter=40,
              min_sampling_iter=30, max_sampling_iter=30, varying=Q)
    host = wa.walnuts_device(MODEL, data=data_of(c), **kw)
    kept, chains = wa.walnuts_device(MODEL, data=data_of(c), keep_on_device=True, thin=1, **kw)
    assert len(host) == 8
    for a, b in zip(host, kept):
        assert np.asarray(a).shape == (30, D)
        assert np.array_equal(np.asarray(a), np.asarray(b))
        assert np.all(np.isfinite(np.asarray(a)))
    common = dict(num_params=D, data=data_of(c), varying=Q)
    res = wa.log_predictive(MODEL, chains, **common)
    assert res.lpd.shape == (N,) and np.all(np.isfinite(res.lpd))
    loo = wa.psis_loo(MODEL, chains, **common)
    assert loo.lpd.shape == (N,) and np.all(np.isfinite(loo.lpd)) and np.all(np.isfinite(loo.elpd_loo))
    pr = wa.predict(MODEL, chains, num_params=D, data=(c["x"][:7], c["group"][:7]), varying=Q)
    assert pr.mean.shape == (7,) and np.all(np.isfinite(pr.mean)) and np.all(pr.noise_var > 0)
    ppc = wa.posterior_predictive_check(MODEL, chains, seed=3, **common)
    assert np.all((ppc.p_value["mean"] >= 0) & (ppc.p_value["mean"] <= 1))
    chains.close()
    sets = [data_of(make_case(P, J, Q, n, seed=3 + n)) for n in (40, 17, 25)]
    kw["num_chains"] = 12
    many = wa.walnuts_device(MODEL, datasets=sets, **kw)
    kept, views = wa.walnuts_device(MODEL, datasets=sets, keep_on_device=True, thin=1, **kw)
    assert len(many) == 12 and len(views) == 3
    for a, b in zip(many, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b))
        assert np.all(np.isfinite(np.asarray(a)))
    for v in views:
        v.close()


@pytest.mark.timeout(1800)
def test_against_exact_posterior(gpu):
    """test_hier_scale_gpu.test_linear_sigma_against_exact_posterior with two group scales: its chain count, iteration
    counts and MCSE-based acceptance rule, unchanged (4096 chains, 300 warmup, 60 x 2 sampling, 5 se + 1e-3 sd)."""
    x, y, group, mp, P, J, Q = hss.exact_case()
    D = hss.dim(P, J, Q)
    mean, var = hss.exact_posterior(x, y, group, mp, J)
    C, T = 4096, 60
    e = wa.DeviceEngine(MODEL, D, C, wa.default_config(), params=mp, data=(x, y, group), varying=Q)
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
        tau, sig = np.exp(th[:, D - 1 - Q:D - 1]), np.exp(th[:, D - 1])
        u = th[:, P:P + Q * J].reshape(C, Q, J)
        q = np.concatenate([th[:, :P], (tau[:, :, None] * u).reshape(C, Q * J), tau, sig[:, None]], axis=1)
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
def test_non_finite_scales(gpu):
    """Chains placed at s = +-800 and s_q = +-800 (q = 0 and the last): logp_grad returns IEEE values, the transitions
    treat the energies as every non-finite energy, the chains elsewhere stay finite and check() is clean."""
    c = make_case(4, 6, 3, 50, seed=4)
    D, Q = c["D"], c["Q"]
    e = wa.DeviceEngine(MODEL, D, 8, wa.default_config(), params=c["mp"], data=data_of(c), varying=Q)
    e.init_positions(seed=1, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=2)
    pos = e.positions()
    pos[0, D - 1], pos[1, D - 1] = 800.0, -800.0
    pos[2, D - 1 - Q], pos[3, D - 1 - Q], pos[4, D - 2], pos[5, D - 2] = 800.0, -800.0, 800.0, -800.0
    lp, g = e.logp_grad(pos)
    assert np.all(np.isfinite(lp[6:])) and np.all(np.isfinite(g[6:]))
    for ch in (0, 1, 2, 4):
        assert not np.isfinite(lp[ch]) or not np.all(np.isfinite(g[ch])), ch
    e.set_positions(pos)
    e.warmup_steps(4)
    e.freeze()
    e.sample_steps(4)
    e.check()
    after = e.positions()
    assert np.all(np.isfinite(after[6:])) and np.all(np.isfinite(e.logp()[6:]))
    e.close()
