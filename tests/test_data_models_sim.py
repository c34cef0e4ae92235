"""CPU tier: models conditioned on data (walnuts_amd/csrc/models/glm.h, wn_model_api.h kUsesData) and the
model-agnostic evaluation entry point (wn_engine_eval, DeviceEngine.logp_grad), under the workgroup emulation.

The references are float64 NumPy restatements of the two densities, a central finite difference of the returned log
density, and the high-precision references with per-chain error bounds of tests/helpers/hp_reference.py (the GLM edge
matrix: block sizes, padding boundaries, saturated logits); the device side of the same kernel source is compared bit
for bit in test_data_models_gpu.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpusim"))
import build as simbuild  # noqa: E402
sys.path.insert(0, os.path.join(HERE, "helpers"))
import hp_reference as hp  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from walnuts_amd import models  # noqa: E402

LIN, LOG = wa.MODEL_LINEAR_REGRESSION, wa.MODEL_LOGISTIC_REGRESSION
# one wavefront per chain at 2, 4 and 16 elements per lane, with padding
DIMS = (5, 150, 1000)


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def make_data(model, D, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, D)) / np.sqrt(D)
    x[:, 0] = 1.0  # an intercept column
    theta = rng.normal(size=D)
    eta = x @ theta
    if model == LIN:
        y = eta + rng.normal(size=N)
    else:
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    s2 = rng.uniform(0.5, 4.0, size=D)
    return x, y, s2


def numpy_logp_grad(model, x, y, s2, theta):
    eta = theta @ x.T  # [C, N]
    if model == LIN:
        r = y - eta
        ll = -0.5 * (r * r).sum(axis=1)
    else:
        r = y - 1.0 / (1.0 + np.exp(-eta))
        ll = (y * eta - np.logaddexp(0.0, eta)).sum(axis=1)
    return ll - 0.5 * (theta * theta / s2).sum(axis=1), r @ x - theta / s2


def engine(sim, model, D, C, data, s2, **cfg):
    return wa.DeviceEngine(model, D, C, wa.default_config(sim, **cfg), params=s2, lib_path=sim, data=data)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("model", [LIN, LOG])
@pytest.mark.parametrize("D,N", [(5, 50), (150, 123), (1000, 300)])
@pytest.mark.parametrize("fma", [0, 1])
def test_logp_grad_matches_numpy(sim, model, D, N, fma):
    x, y, s2 = make_data(model, D, N, seed=D + N)
    e = engine(sim, model, D, 4, (x, y), s2, fused_multiply_add=fma)
    theta = np.random.default_rng(7).normal(size=(4, D)) * 0.3
    lp, g = e.logp_grad(theta)
    lp_ref, g_ref = numpy_logp_grad(model, x, y, s2, theta)
    assert np.all(np.abs(lp - lp_ref) <= 1e-12 * np.abs(lp_ref))
    for c in range(4):
        assert np.linalg.norm(g[c] - g_ref[c]) <= 1e-12 * np.linalg.norm(g_ref[c])
    epl = {5: 2, 150: 4, 1000: 16}[D]
    assert hp.error_ratio(lp, g, hp.glm_case(model, x, y, s2, theta, epl)) <= 1.0
    # a central finite difference of the returned log density agrees with the returned gradient
    rng = np.random.default_rng(3)
    coords = rng.choice(D, size=min(D, 4), replace=False)
    h = 1e-5
    for i in coords:
        plus, minus = theta.copy(), theta.copy()
        plus[:, i] += h
        minus[:, i] -= h
        fd = (e.logp_grad(plus)[0] - e.logp_grad(minus)[0]) / (2 * h)
        assert np.all(np.abs(fd - g[:, i]) <= 1e-6 * (1.0 + np.abs(lp))), (i, fd, g[:, i])


@pytest.mark.timeout(600)
@pytest.mark.parametrize("model,D", [(wa.MODEL_STD_NORMAL, 5), (wa.MODEL_STD_NORMAL, 1000), (wa.MODEL_DIAG_NORMAL, 150),
                                     (wa.MODEL_FUNNEL, 150), (wa.MODEL_STD_NORMAL, 300), (wa.MODEL_RW1, 5),
                                     (wa.MODEL_RW1, 150), (wa.MODEL_RW1, 1000), (wa.MODEL_RW1, 257), (wa.MODEL_RW1, 300)])
def test_logp_grad_of_the_existing_models(sim, model, D):
    """The entry point serves every model: the synthetic targets' densities against NumPy and against the
    high-precision references within their bounds (D = 257 and 300 with elems_per_lane=-1: the streaming kernels,
    ending in a ragged tile)."""
    stream = D in (257, 300)
    rng = np.random.default_rng(D)
    C = 3
    theta = rng.normal(size=(C, D))
    params = rng.uniform(0.5, 2.0, size=D) if model == wa.MODEL_DIAG_NORMAL else None
    cfg = dict(waves_per_chain=1, elems_per_lane=-1) if stream else {}
    e = wa.DeviceEngine(model, D, C, wa.default_config(sim, **cfg), params=params, lib_path=sim)
    assert e.streaming == stream
    before = e.positions()
    lp, g = e.logp_grad(theta)
    if model == wa.MODEL_STD_NORMAL:
        lp_ref, g_ref = -0.5 * (theta * theta).sum(1), -theta
    elif model == wa.MODEL_DIAG_NORMAL:
        lp_ref, g_ref = -0.5 * (theta * theta / params).sum(1), -theta / params
    elif model == wa.MODEL_FUNNEL:  # Neal's funnel: v ~ N(0, 3^2), x_i | v ~ N(0, e^v)
        v, xs = theta[:, 0], theta[:, 1:]
        S = (xs * xs).sum(1)
        lp_ref = -v * v / 18 - 0.5 * np.exp(-v) * S - 0.5 * (D - 1) * v
        g_ref = np.empty_like(theta)
        g_ref[:, 0] = -v / 9 + 0.5 * np.exp(-v) * S - 0.5 * (D - 1)
        g_ref[:, 1:] = -xs * np.exp(-v)[:, None]
    else:  # rw1 (models/rw1.h): r_0 = y_0, r_n = y_n - rho y_{n-1}, w_n = r_n / (1 - rho^2) (w_0 = r_0)
        rho = 0.99
        r = theta.copy()
        r[:, 1:] -= rho * theta[:, :-1]
        w = r / (1.0 - rho * rho)
        w[:, 0] = r[:, 0]
        lp_ref = -0.5 * (r * w).sum(1)
        g_ref = -w
        g_ref[:, :-1] += rho * w[:, 1:]
    assert np.allclose(lp, lp_ref, rtol=1e-12, atol=0)
    assert np.allclose(g, g_ref, rtol=1e-12, atol=1e-300 if model != wa.MODEL_RW1 else 1e-12 * np.abs(g_ref).max())
    nw = e.lanes // 64
    assert hp.error_ratio(lp, g, hp.simple_case(model, theta, params, e.dim_padded // (64 * nw), nw)) <= 1.0
    assert np.array_equal(e.positions(), before), "logp_grad must leave the chains' state alone"


def short_run(sim, model, D, N, fma=1, seed=5):
    x, y, s2 = make_data(model, D, N, seed=seed)
    e = engine(sim, model, D, 4, (x, y), s2, fused_multiply_add=fma)
    e.init_positions(seed=seed, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=seed + 1)
    for _ in range(4):
        e.warmup_step()
    e.freeze()
    draws = []
    for _ in range(4):
        e.sample_step()
        draws.append(e.positions())
    e.check()
    return dict(draws=np.array(draws), logp=e.logp(), steps=e.step_sizes(), inv_mass=e.inv_mass(),
                depths=e.depths(), grads=e.grad_evals(), failed=e.failed_extensions())


@pytest.mark.timeout(900)
@pytest.mark.parametrize("model,D,N", [(LIN, 5, 60), (LOG, 150, 200), (LOG, 1000, 50)])
def test_short_run_is_deterministic(sim, model, D, N):
    a = short_run(sim, model, D, N)
    b = short_run(sim, model, D, N)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.all(np.isfinite(a["draws"])) and np.all(np.isfinite(a["logp"]))
    assert np.all(a["grads"] > 0)


@pytest.mark.timeout(300)
def test_refusals(sim):
    x, y, s2 = make_data(LOG, 5, 20, seed=1)
    cfg = wa.default_config(sim)
    with pytest.raises(ValueError, match="conditioned on data"):
        wa.DeviceEngine(LOG, 5, 2, cfg, params=s2, lib_path=sim)
    with pytest.raises(ValueError, match="reads no data"):
        wa.DeviceEngine(wa.MODEL_STD_NORMAL, 5, 2, cfg, lib_path=sim, data=(x, y))
    with pytest.raises(ValueError, match="data x must have shape"):
        wa.DeviceEngine(LOG, 6, 2, cfg, params=np.ones(6), lib_path=sim, data=(x, y))
    with pytest.raises(ValueError, match="data y must have shape"):
        wa.DeviceEngine(LOG, 5, 2, cfg, params=s2, lib_path=sim, data=(x, y[:-1]))
    bad = x.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="must be finite"):
        wa.DeviceEngine(LOG, 5, 2, cfg, params=s2, lib_path=sim, data=(bad, y))
    yb = y.copy()
    yb[0] = np.inf
    with pytest.raises(ValueError, match="must be finite"):
        wa.DeviceEngine(LIN, 5, 2, cfg, params=s2, lib_path=sim, data=(x, yb))
    y2 = y.copy()
    y2[4] = 0.5
    with pytest.raises(ValueError, match=r"y in \{0, 1\}"):
        wa.DeviceEngine(LOG, 5, 2, cfg, params=s2, lib_path=sim, data=(x, y2))
    wa.DeviceEngine(LIN, 5, 2, cfg, params=s2, lib_path=sim, data=(x, y2)).close()  # any real y for the linear model
    with pytest.raises(ValueError, match="prior variances"):
        wa.DeviceEngine(LIN, 5, 2, cfg, params=-s2, lib_path=sim, data=(x, y))
    xl = np.zeros((3, 1100))
    with pytest.raises(ValueError, match="num_params <= 1024"):
        wa.DeviceEngine(LIN, 1100, 2, cfg, params=np.ones(1100), lib_path=sim, data=(xl, np.zeros(3)))
    with pytest.raises(ValueError, match="one wavefront per chain"):
        wa.DeviceEngine(LIN, 5, 2, wa.default_config(sim, waves_per_chain=2, elems_per_lane=2), params=s2,
                        lib_path=sim, data=(x, y))
    with pytest.raises(ValueError, match="not available with devices"):
        wa.walnuts_device(LOG, model_params=s2, num_params=5, data=(x, y), devices=[0, 0], lib_path=sim)
    with pytest.raises(ValueError, match="not available with reference_streams"):
        wa.walnuts_device(LOG, model_params=s2, num_params=5, data=(x, y), reference_streams=True, lib_path=sim)
    with pytest.raises(ValueError, match="conditioned on data"):
        wa.walnuts_device(LOG, model_params=s2, num_params=5, lib_path=sim, min_warmup_iter=2, max_warmup_iter=2,
                          min_sampling_iter=2, max_sampling_iter=2)


@pytest.mark.timeout(900)
def test_drop_in_call_with_data(sim):
    """walnutpie_sample_device_observed and _observed_resident under the emulation: same draws."""
    x, y, s2 = make_data(LOG, 5, 40, seed=2)
    kw = dict(model_params=s2, num_params=5, num_chains=3, seed=9, min_warmup_iter=6, max_warmup_iter=6,
              min_sampling_iter=5, max_sampling_iter=5, lib_path=sim, data=(x, y))
    host = wa.walnuts_device(LOG, **kw)
    kept, chains = wa.walnuts_device(LOG, keep_on_device=True, thin=1, **kw)
    for a, b in zip(host, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b))
        assert np.all(np.isfinite(np.asarray(a)))
    chains.close()


@pytest.mark.timeout(1200)
def test_runtime_compiled_copy_of_the_glm_header(sim, tmp_path):
    """A user's copy of the GLM model, compiled at run time under another name and id, gives the built-in model's bits."""
    gxx = ["g++", "-x", "c++", "-std=c++20", "-O1", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden", "-pthread",
           "-DWN_CPU_SIM", "-I", os.path.join(HERE, "cpusim")]
    header = os.path.join(os.path.dirname(HERE), "walnuts_amd", "csrc", "models", "glm.h")
    D, N = 150, 90
    so = models.build_device_model(header, "wn::LogisticRegressionModel", "user_logistic_150", 13, D,
                                   out_dir=str(tmp_path), lib_path=sim, compiler=gxx)
    mid = models.load_device_model(so, "user_logistic_150", lib_path=sim)
    assert mid == 13
    x, y, s2 = make_data(LOG, D, N, seed=4)
    theta = np.random.default_rng(1).normal(size=(4, D)) * 0.2
    ref = engine(sim, LOG, D, 4, (x, y), s2).logp_grad(theta)
    mine = engine(sim, mid, D, 4, (x, y), s2).logp_grad(theta)
    assert np.array_equal(ref[0], mine[0]) and np.array_equal(ref[1], mine[1])
    runs = []
    for m in (LOG, mid):
        e = engine(sim, m, D, 4, (x, y), s2)
        e.init_positions(seed=3, chain_offset=0, scale=0.5)
        e.init_masses_from_grad(1e-5)
        e.adapt_step(seed=4)
        for _ in range(3):
            e.warmup_step()
        runs.append((e.positions(), e.logp(), e.step_sizes()))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ---- the GLM edge matrix against the high-precision reference (tests/helpers/hp_reference.py) -----------------------
# Rows are taken in register blocks of B = 16 / 8 / 4 / 2 rows at 2 / 4 / 8 / 16 elements per lane (models/glm.h): the
# matrix puts N at 1, B - 1, B, B + 1 (and an odd N at B = 2: the last block holds one of its two rows) and D at 1 and
# at the padding boundary 64 * EPL - 1, 64 * EPL (the one-wavefront kernels take nothing larger).
SIM_GLM_GEOMETRIES = ((1, 2), (1, 4), (1, 8), (1, 16))
GLM_KINDS = {LIN: ("plain", "big_y"), LOG: ("mixed", "y0", "y1")}


def edge_ns(epl):
    B = hp.block_rows(epl)
    return sorted({1, B - 1, B, B + 1} | ({7} if B == 2 else set()))


def edge_dims(epl):
    return (1, 64 * epl - 1, 64 * epl)


def edge_data(model, D, N, kind, seed):
    """x [N, D], y [N], prior variances [D] and three chains' theta [3, D]: a moderate one, one whose largest |eta| is
    800 (exp(-|eta|) underflows past 745) and theta = 0 (eta == 0 exactly).  From N = 3 on, row 0 is all zeros
    (eta == 0 in every chain); from N = 4 on, the last row duplicates row 1.  y: linear "plain" ~ N(0, 1), "big_y" ~ 1e6 N(0, 1);
    logistic "mixed" random, "y0" all 0, "y1" all 1."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, D)) / np.sqrt(D)
    if N >= 3:
        x[0] = 0.0
    if N >= 4:
        x[N - 1] = x[1]
    if model == LIN:
        y = rng.normal(size=N) * (1e6 if kind == "big_y" else 1.0)
    else:
        y = {"y0": np.zeros(N), "y1": np.ones(N)}.get(kind, (rng.random(N) < 0.5).astype(np.float64))
    s2 = rng.uniform(0.5, 4.0, size=D)
    direction = rng.normal(size=D)
    theta = np.stack([0.3 * rng.normal(size=D), direction * (800.0 / np.abs(x @ direction).max()), np.zeros(D)])
    return x, y, s2, theta


def check_glm_edges(lib, model, epl, fma, D):
    """Every N of edge_ns(epl) and every data kind of the model at one (EPL, FMA, D): logp_grad within the bound, the
    bound at least 100 times below what dropping an observation, shifting y or swapping two columns would change, and
    the chains' positions untouched.  -> the largest error / bound seen."""
    worst = 0.0
    cfg = wa.default_config(lib, fused_multiply_add=fma, waves_per_chain=1, elems_per_lane=epl)
    for N in edge_ns(epl):
        for kind in GLM_KINDS[model]:
            x, y, s2, theta = edge_data(model, D, N, kind, seed=1000 * N + D)
            e = wa.DeviceEngine(model, D, 3, cfg, params=s2, lib_path=lib, data=(x, y))
            assert e.lanes == 64 and e.dim_padded == 64 * epl
            before = e.positions()
            lp, g = e.logp_grad(theta)
            assert np.array_equal(e.positions(), before), "logp_grad must leave the chains' state alone"
            e.close()
            ref = hp.glm_case(model, x, y, s2, theta, epl)
            ratio = hp.error_ratio(lp, g, ref)
            assert ratio <= 1.0, (N, kind, ratio)
            assert hp.sensitivity(model, x, y, s2, theta, ref) >= 100.0, (N, kind)
            worst = max(worst, ratio)
    return worst


@pytest.mark.timeout(900)
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("geometry", SIM_GLM_GEOMETRIES, ids=lambda g: f"nw{g[0]}_epl{g[1]}")
@pytest.mark.parametrize("model", [LIN, LOG], ids=["linear", "logistic"])
@pytest.mark.parametrize("dsel", [0, 1, 2], ids=["D1", "Dp-1", "Dp"])
def test_glm_edges_against_high_precision(sim, model, geometry, fma, dsel, record_property):
    epl = geometry[1]
    record_property("max_error_over_bound", check_glm_edges(sim, model, epl, fma, edge_dims(epl)[dsel]))
