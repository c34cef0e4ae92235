"""CPU tier: Poisson and negative binomial regression, linear regression with an estimated noise level
(walnuts_amd/csrc/models/glm.h LogLink, models/glm_scale.h; the kScaleParam layout of wn_model_api.h) and hierarchical
Poisson regression (models/hier_glm.h) under the workgroup emulation.

References: a float64 NumPy restatement, an mpmath reference with a per-chain K u bound (tests/helpers/
hp_count_reference.py), central finite differences, the Poisson limit of the negative binomial, linear_regression at
s = 0, the dense one-hot form of the hierarchical model and its two parameterizations.  The device side of the same
kernel source is compared bit for bit in test_count_models_gpu.py."""
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_count_reference as hc  # noqa: E402
import hp_reference as hp  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from test_datasets_sim import compare_blocks, drive  # noqa: E402

POIS, NB, LSIG = wa.MODEL_POISSON_REGRESSION, wa.MODEL_NEG_BINOMIAL_REGRESSION, wa.MODEL_LINEAR_REGRESSION_SIGMA
HPOIS, HPOIS_C = wa.MODEL_HIER_POISSON_REGRESSION, wa.MODEL_HIER_POISSON_REGRESSION_CENTERED
FLAT = (POIS, NB, LSIG)
FLAT_IDS = ["poisson", "negbin", "linear_sigma"]
SIM_GEOMETRIES = ((1, 2), (1, 4), (1, 8), (1, 16))
CSRC = os.path.join(os.path.dirname(HERE), "walnuts_amd", "csrc")


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def scale_model(model):
    return model in (NB, LSIG)


def make_count(model, D, N, seed, sigma0=2.0):
    """x [N, P] (P = D, or D - 1 with a scale), y [N], model_params [D]: counts for POIS / NB, reals for LSIG."""
    rng = np.random.default_rng(seed)
    P = D - 1 if scale_model(model) else D
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    eta = x @ rng.normal(size=P) + 0.5
    if model == LSIG:
        y = eta + 0.7 * rng.normal(size=N)
    elif model == NB:
        y = rng.negative_binomial(2.0, 2.0 / (2.0 + np.exp(eta))).astype(np.float64)
    else:
        y = rng.poisson(np.exp(eta)).astype(np.float64)
    mp = rng.uniform(0.5, 4.0, size=D)
    if scale_model(model):
        mp[-1] = sigma0
    return x, y, mp


def engine(lib, model, D, C, data, mp, epl=0, fma=1, **kw):
    cfg = wa.default_config(lib, fused_multiply_add=fma, waves_per_chain=1 if epl else 0, elems_per_lane=epl, **kw)
    return wa.DeviceEngine(model, D, C, cfg, params=mp, lib_path=lib, data=data)


def thetas(model, D, C, rng, s=(0.3, -0.5, 1.0)):
    th = rng.normal(size=(C, D)) * 0.3
    if scale_model(model):
        th[:, -1] = np.resize(np.asarray(s, dtype=np.float64), C)
    return th


@pytest.mark.timeout(900)
@pytest.mark.parametrize("model", FLAT, ids=FLAT_IDS)
@pytest.mark.parametrize("D,N", [(3, 37), (130, 20), (2, 1)])
@pytest.mark.parametrize("fma", [0, 1])
def test_logp_grad_matches_numpy_and_finite_differences(sim, model, D, N, fma):
    x, y, mp = make_count(model, D, N, seed=D + N)
    e = engine(sim, model, D, 3, (x, y), mp, fma=fma)
    theta = thetas(model, D, 3, np.random.default_rng(9))
    before = e.positions()
    lp, g = e.logp_grad(theta)
    assert np.array_equal(e.positions(), before), "logp_grad must leave the chains' state alone"
    lp_ref, g_ref = hc.numpy_logp_grad(model, x, y, mp, theta)
    assert np.all(np.abs(lp - lp_ref) <= 1e-11 * (1 + np.abs(lp_ref)))
    for c in range(3):
        assert np.linalg.norm(g[c] - g_ref[c]) <= 1e-11 * (1 + np.linalg.norm(g_ref[c]))
    h = 1e-5
    for i in range(D) if D <= 12 else [0, 1, 2, D - 2, D - 1]:
        plus, minus = theta.copy(), theta.copy()
        plus[:, i] += h
        minus[:, i] -= h
        fd = (e.logp_grad(plus)[0] - e.logp_grad(minus)[0]) / (2 * h)
        assert np.all(np.abs(fd - g[:, i]) <= 1e-6 * (1.0 + np.abs(lp))), (i, fd, g[:, i])


# ---- the edge matrix against the mpmath reference -------------------------------------------------------------------
# N at 1, B - 1, B, B + 1 for the block of B rows; D at the smallest (1 for Poisson, 2 with a scale) and at
# Dp - 1 = 64 EPL - 1 and Dp = 64 EPL for each of the emulation's one-wavefront widths.
def edge_ns(epl):
    B = hp.block_rows(epl)
    return sorted({1, max(1, B - 1), B, B + 1})


def edge_thetas(model, x, D, rng):
    """Four chains: moderate; a saturated link (|eta| ~ 700 Poisson, |t| ~ 745 negative binomial); s = +-36."""
    P = x.shape[1]
    th = thetas(model, D, 4, rng, s=(0.2, 0.1, 36.0, -36.0))
    direction = rng.normal(size=P)
    scale = np.abs(x @ direction).max()
    if model == POIS:  # (column 0 of x is all ones: check_edges)
        th[1, :P] = direction * (690.0 / max(scale, 1e-300))  # exp(eta) up to 1e299
        th[2, :P] = 0.0
        th[2, 0] = -745.0  # exp(eta) in the subnormal range on every row
    elif model == NB:
        th[1, :P] = direction * (745.0 / max(scale, 1e-300))
        th[1, -1] = 0.0
        th[2, :P] *= 0.1
        th[3, :P] = direction * (-700.0 / max(scale, 1e-300))
    else:
        th[1, :P] = direction * (50.0 / max(scale, 1e-300))
        th[2, -1], th[3, -1] = 3.0, -3.0
    return th


def check_edges(lib, model, epl, fma):
    worst = 0.0
    rng = np.random.default_rng(epl * 10 + fma + model)
    smallest = 2 if scale_model(model) else 1
    for D in (smallest, 64 * epl - 1, 64 * epl):
        for N in edge_ns(epl):
            x, y, mp = make_count(model, D, N, seed=1000 * N + D)
            if model == POIS:
                x[:, 0] = 1.0
            if model == NB and N > 2:
                y[0], y[1] = 1e6, 2.0 ** 40  # the large counts of the domain
            e = engine(lib, model, D, 4, (x, y), mp, epl=epl, fma=fma)
            assert e.lanes == 64 and e.dim_padded == 64 * epl
            theta = edge_thetas(model, x, D, rng)
            lp, g = e.logp_grad(theta)
            e.close()
            ref = hc.count_case(model, x, y, mp, theta, epl)
            ratio = hp.error_ratio(lp, g, ref)
            assert ratio <= 1.0, (D, N, ratio)
            worst = max(worst, ratio)
            if N >= 2 and not np.array_equal(np.roll(y, 1), y) and x.shape[1] >= 2:  # y shifted by one row: not hidden
                assert hp.error_ratio(lp, g, hc.count_case(model, x, np.roll(y, 1), mp, theta, epl)) >= 100.0
    return worst


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("geometry", SIM_GEOMETRIES, ids=lambda g: f"nw{g[0]}_epl{g[1]}")
@pytest.mark.parametrize("model", FLAT, ids=FLAT_IDS)
def test_edges_against_mpmath(sim, model, geometry, fma, record_property):
    record_property("max_error_over_bound", check_edges(sim, model, geometry[1], fma))


@pytest.mark.timeout(600)
def test_negative_binomial_tends_to_poisson(sim):
    """At s = -36 (phi = 4.3e15) the negative binomial likelihood equals Poisson's within the two bounds and the exact
    difference between the two densities (O(y^2 / phi))."""
    D, N = 4, 25
    x, y, mp = make_count(POIS, D, N, seed=4)
    theta = np.random.default_rng(1).normal(size=(3, D)) * 0.3
    lp_p, g_p = engine(sim, POIS, D, 3, (x, y), mp).logp_grad(theta)
    mpn = np.append(mp, 2.0)
    tn = np.concatenate([theta, np.full((3, 1), -36.0)], axis=1)
    xn = x  # P = D columns, num_params = D + 1
    lp_n, g_n = engine(sim, NB, D + 1, 3, (xn, y), mpn).logp_grad(tn)
    ref_p = hc.count_case(POIS, x, y, mp, theta, 16)
    ref_n = hc.count_case(NB, xn, y, mpn, tn, 16)
    s = -36.0
    prior_s = s - np.exp(2 * s) / (2 * 4.0)
    exact = np.abs((ref_n[0] - prior_s) - ref_p[0])
    assert np.all(np.abs((lp_n - prior_s) - lp_p) <= ref_n[2] + ref_p[2] + exact + 4 * hp.U * abs(prior_s))
    gexact = np.abs(ref_n[1][:, :D] - ref_p[1])
    assert np.all(np.abs(g_n[:, :D] - g_p) <= ref_n[3][:, :D] + ref_p[3] + gexact)
    assert np.all(exact < 1e-10)


@pytest.mark.timeout(600)
def test_linear_sigma_at_zero_is_linear_regression(sim):
    """linear_regression_sigma at s = 0 equals linear_regression plus the scale prior's term s - 1 / (2 sigma_0^2)."""
    D, N = 5, 30
    x, y, mp = make_count(LSIG, D + 1, N, seed=8)
    theta = np.random.default_rng(2).normal(size=(3, D)) * 0.4
    lp_l, g_l = engine(sim, wa.MODEL_LINEAR_REGRESSION, D, 3, (x, y), mp[:D]).logp_grad(theta)
    ts = np.concatenate([theta, np.zeros((3, 1))], axis=1)
    lp_s, g_s = engine(sim, LSIG, D + 1, 3, (x, y), mp).logp_grad(ts)
    assert np.allclose(lp_s, lp_l - 1.0 / (2 * mp[-1] ** 2), rtol=1e-13, atol=1e-13)
    assert np.allclose(g_s[:, :D], g_l, rtol=1e-13, atol=1e-13)
    r = y - theta @ x.T
    assert np.allclose(g_s[:, -1], (r * r).sum(1) - N + 1 - 1.0 / mp[-1] ** 2, rtol=1e-12)


def make_hier(P, J, N, seed, sigma_tau=1.5):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    group = rng.integers(0, J, size=N).astype(np.int32)
    eta = x @ rng.normal(size=P) + rng.normal(size=J)[group]
    y = rng.poisson(np.exp(eta)).astype(np.float64)
    mp = np.concatenate([rng.uniform(0.5, 4.0, size=P), np.ones(J), [sigma_tau]])
    return x, y, group, mp


@pytest.mark.timeout(600)
def test_hier_poisson_equals_flat_poisson_on_one_hot(sim):
    P, J, N = 4, 7, 50
    x, y, group, mp = make_hier(P, J, N, seed=5)
    D = P + J + 1
    theta = np.random.default_rng(3).normal(size=(3, D)) * 0.4
    lp, g = engine(sim, HPOIS, D, 3, (x, y, group), mp).logp_grad(theta)
    beta, z, s = theta[:, :P], theta[:, P:P + J], theta[:, -1]
    tau = np.exp(s)
    ll = lp - (-(beta * beta / (2 * mp[:P])).sum(1) - (z * z).sum(1) / 2 + s - tau * tau / (2 * mp[-1] ** 2))
    xw = np.concatenate([x, np.eye(J)[group]], axis=1)
    tf = np.concatenate([beta, tau[:, None] * z], axis=1)
    big = np.full(P + J, 1e300)  # (a vanishing prior: the flat model's logp is then its likelihood)
    lpf, gf = engine(sim, POIS, P + J, 3, (xw, y), big).logp_grad(tf)
    assert np.allclose(ll, lpf, rtol=1e-12, atol=1e-12)
    assert np.allclose(g[:, :P], gf[:, :P] - beta / mp[:P], rtol=1e-12, atol=1e-12)


@pytest.mark.timeout(600)
def test_hier_poisson_reparameterization_identity(sim):
    """logp_nc(beta, z, s) == logp_c(beta, exp(s) z, s) + J s"""
    P, J, N = 6, 9, 40
    x, y, group, mp = make_hier(P, J, N, seed=21)
    D = P + J + 1
    theta = np.random.default_rng(2).normal(size=(4, D)) * 0.5
    theta[:, -1] = (-1.0, 0.0, 0.5, 1.5)
    lp_nc, _ = engine(sim, HPOIS, D, 4, (x, y, group), mp).logp_grad(theta)
    tc = theta.copy()
    tc[:, P:P + J] *= np.exp(theta[:, -1])[:, None]
    lp_c, _ = engine(sim, HPOIS_C, D, 4, (x, y, group), mp).logp_grad(tc)
    assert np.allclose(lp_nc, lp_c + J * theta[:, -1], rtol=1e-12, atol=1e-12)


@pytest.mark.timeout(600)
def test_refusals(sim):
    D, N = 4, 10
    for model in (POIS, NB, HPOIS):
        bad_values = (-1.0, 0.5, np.nan, np.inf)
        for bad in bad_values:
            if model == HPOIS:
                x, y, group, mp = make_hier(2, 3, N, seed=1)
                y[3] = bad
                data, dim = (x, y, group), 6
            else:
                x, y, mp = make_count(model, D, N, seed=1)
                y[3] = bad
                data, dim = (x, y), D
            with pytest.raises(ValueError, match="count|finite"):
                engine(sim, model, dim, 2, data, mp)
    # the wrong width of x names the expected one
    x, y, mp = make_count(NB, D, N, seed=2)
    with pytest.raises(ValueError, match=r"data x must have shape \(num_obs, 3\)"):
        engine(sim, NB, D, 2, (np.ones((N, D)), y), mp)
    x, y, mp = make_count(POIS, D, N, seed=2)
    with pytest.raises(ValueError, match=r"data x must have shape \(num_obs, 4\)"):
        engine(sim, POIS, D, 2, (x[:, :3], y), mp)
    with pytest.raises(ValueError, match=r"data x must have shape \(num_obs, 3\)"):
        wa.DeviceEngine(LSIG, D, 2, wa.default_config(sim), params=mp, lib_path=sim, datasets=[(x, y), (x, y)])
    # num_params < 2 for a scale model; sigma_0 <= 0
    with pytest.raises(ValueError, match="2 <= num_params"):
        engine(sim, LSIG, 1, 2, (np.ones((N, 0)), y), np.ones(1))
    x, y, mp = make_count(LSIG, D, N, seed=3)
    for s0 in (0.0, -1.0, np.nan):
        mp2 = mp.copy()
        mp2[-1] = s0
        with pytest.raises(ValueError, match="sigma_0"):
            engine(sim, LSIG, D, 2, (x, y), mp2)
    # groups for a model without groups
    with pytest.raises(ValueError, match="reads no groups"):
        engine(sim, NB, D, 2, (x, y, np.zeros(N, dtype=np.int32)), mp)
    # data needed
    with pytest.raises(ValueError, match=r"num_params - 1"):
        wa.DeviceEngine(NB, D, 2, wa.default_config(sim), params=mp, lib_path=sim)


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("geometry", SIM_GEOMETRIES, ids=lambda g: f"nw{g[0]}_epl{g[1]}")
def test_datasets_equal_standalone_engines(sim, geometry):
    epl = geometry[1]
    D, k = 5, 2
    B = hp.block_rows(epl)
    datasets = []
    for g, n in enumerate((1, B + 1, 2 * B + 3)):
        x, y, mp = make_count(NB, D, n, seed=40 + g)
        datasets.append((x, y + 3 * g))
    cfg = wa.default_config(sim, waves_per_chain=1, elems_per_lane=epl)
    e = wa.DeviceEngine(NB, D, 3 * k, cfg, params=mp, lib_path=sim, datasets=datasets)
    batched = drive(e, 0)
    for g, d in enumerate(datasets):
        alone = wa.DeviceEngine(NB, D, k, cfg, params=mp, lib_path=sim, data=d)
        compare_blocks(batched, drive(alone, g * k), g, k)
        alone.close()
    e.close()


def runtime_copy(tmp_path):
    """models/glm_scale.h copied under another namespace: a header of one's own that holds the scale model."""
    src = open(os.path.join(CSRC, "models", "glm_scale.h")).read()
    src = src.replace('#include "glm.h"', '#include "models/glm.h"')
    src = src.replace("namespace wn {", "namespace user {\nusing namespace wn;").replace("}  // namespace wn",
                                                                                         "}  // namespace user")
    path = os.path.join(str(tmp_path), "my_negbin.h")
    with open(path, "w") as f:
        f.write(src)
    return path


@pytest.mark.timeout(900)
def test_runtime_copy_of_the_scale_model(sim, tmp_path):
    """A copy of glm_scale.h compiled at run time under id 19 gives the built-in model's bits: the kScaleParam trait
    reaches run-time models through the ABI (x of num_params - 1 columns, the same kernels)."""
    from walnuts_amd import models
    gxx = ["g++", "-x", "c++", "-std=c++20", "-O1", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden", "-pthread",
           "-DWN_CPU_SIM", "-I", os.path.join(HERE, "cpusim")]
    lib = os.path.join(str(tmp_path), "libwalnuts_sim_copy.so")
    shutil.copy(sim, lib)  # (a library of its own: the run-time model registers into the library it links against)
    D, N = 6, 21
    so = models.build_device_model(runtime_copy(tmp_path), "user::NegBinomialRegressionModel", "user_negbin", 19, D,
                                   out_dir=str(tmp_path), waves_per_chain=1, elems_per_lane=4, lib_path=lib,
                                   compiler=gxx)
    mid = models.load_device_model(so, "user_negbin", lib_path=lib)
    assert mid == 19
    x, y, mp = make_count(NB, D, N, seed=13)
    cfg = wa.default_config(lib, waves_per_chain=1, elems_per_lane=4)
    mine = wa.DeviceEngine(mid, D, 3, cfg, params=mp, lib_path=lib, data=(x, y))
    built_in = wa.DeviceEngine(NB, D, 3, cfg, params=mp, lib_path=lib, data=(x, y))
    theta = thetas(NB, D, 3, np.random.default_rng(4))
    a, b = mine.logp_grad(theta), built_in.logp_grad(theta)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    sa, sb = drive(mine, 0), drive(built_in, 0)
    for u, v in zip(sa, sb):
        for key in v:
            assert np.array_equal(u[key], v[key], equal_nan=True), key
