"""CPU tier: hierarchical regression with varying intercepts by group (walnuts_amd/csrc/models/hier_glm.h; the group
channel of wn_model_api.h, kUsesGroups) under the workgroup emulation.

References: a float64 NumPy restatement of the four densities, an np.longdouble restatement with a per-chain error bound
in the style of tests/helpers/hp_reference.py (K * u * the absolute version of the computation), central finite
differences, the identity between the two parameterizations, and the dense one-hot workaround (a flat GLM on x widened
with the group indicators).  The device side of the same kernel source is compared bit for bit in
test_hier_models_gpu.py."""
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
from test_datasets_sim import compare_blocks, drive  # noqa: E402

HLIN, HLOG = wa.MODEL_HIER_LINEAR_REGRESSION, wa.MODEL_HIER_LOGISTIC_REGRESSION
HLIN_C, HLOG_C = wa.MODEL_HIER_LINEAR_REGRESSION_CENTERED, wa.MODEL_HIER_LOGISTIC_REGRESSION_CENTERED
HIER = (HLIN, HLOG, HLIN_C, HLOG_C)
IDS = ["linear", "logistic", "linear_c", "logistic_c"]
SIM_GEOMETRIES = ((1, 2), (1, 4), (1, 8), (1, 16))


def is_logistic(model):
    return model in (HLOG, HLOG_C)


def is_centered(model):
    return model in (HLIN_C, HLOG_C)


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def make_hier(model, P, J, N, seed, sigma_tau=1.5):
    """x [N, P], y [N], group [N] (row 0 in group J - 1; with J > 2 some groups stay empty when N is small), and
    model_params [P + J + 1]."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    group = rng.integers(0, J, size=N).astype(np.int32)
    group[0] = J - 1
    u = rng.normal(size=J)
    eta = x @ rng.normal(size=P) + u[group]
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64) if is_logistic(model) else eta + rng.normal(size=N)
    mp = np.concatenate([rng.uniform(0.5, 4.0, size=P), np.ones(J), [sigma_tau]])
    return x, y, group, mp


def split(theta, P, J):
    theta = np.atleast_2d(theta)
    return theta[:, :P], theta[:, P:P + J], theta[:, P + J]


def numpy_logp_grad(model, x, y, group, mp, theta, dtype=np.float64):
    """logp [C], grad [C, D] and their absolute versions (see hier_bound) in `dtype`."""
    X, Y, MP, TH = (np.asarray(a, dtype=dtype) for a in (x, y, mp, np.atleast_2d(theta)))
    N, P = X.shape
    J = TH.shape[1] - P - 1
    beta, u, s = split(TH, P, J)
    s2, sig2 = MP[:P], MP[-1] * MP[-1]
    tau = np.exp(s)
    v = u if is_centered(model) else tau[:, None] * u
    eta = beta @ X.T + v[:, group]  # [C, N]
    A = np.abs(beta) @ np.abs(X).T + np.abs(v[:, group])
    if is_logistic(model):
        sp = np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta)))
        r = Y - 1 / (1 + np.exp(-eta))
        ln = Y * eta - sp
        la = np.abs(Y * eta) + sp + 1
    else:
        r = Y - eta
        ln = -r * r / 2
        la = r * r / 2
    onehot = np.zeros((N, J), dtype=dtype)
    onehot[np.arange(N), group] = 1
    S, Sa = r @ onehot, (np.abs(r) + A) @ onehot  # [C, J]
    tt = tau * tau / sig2
    prior = beta * beta / (2 * s2)
    lp = ln.sum(1) - prior.sum(1) + s - tt / 2
    lpa = (la + np.abs(r) * A).sum(1) + prior.sum(1) + np.abs(s) + tt / 2
    g = np.zeros_like(TH)
    ga = np.zeros_like(TH)
    g[:, :P] = r @ X - beta / s2
    ga[:, :P] = (np.abs(r) + A) @ np.abs(X) + np.abs(beta) / s2
    if is_centered(model):
        q = (u * u).sum(1) / (tau * tau)
        lp += -J * s - q / 2
        lpa += J * np.abs(s) + q / 2
        g[:, P:P + J] = S - u / (tau * tau)[:, None]
        ga[:, P:P + J] = Sa + np.abs(u) / (tau * tau)[:, None]
        g[:, -1] = -J + q + 1 - tt
        ga[:, -1] = J + q + 1 + tt
    else:
        lp += -(u * u).sum(1) / 2
        lpa += (u * u).sum(1) / 2
        g[:, P:P + J] = tau[:, None] * S - u
        ga[:, P:P + J] = tau[:, None] * Sa + np.abs(u)
        g[:, -1] = tau * (u * S).sum(1) + 1 - tt
        ga[:, -1] = tau * (np.abs(u) * Sa).sum(1) + 1 + tt
    return lp, g, lpa, ga


# tau = wnd::dexp(s): a few ulps, squared in tau^2 and 1 / tau^2 and multiplied into every v_g
K_TAU = 12


def hier_bound(lpa, ga, N, J, epl):
    """Per-chain bounds for models/hier_glm.h: glm_bound's depths (tests/helpers/hp_reference.py) plus the group
    terms -- the add of v_g to eta, the error of tau, S_j accumulated over at most N rows, and the epilogue's cx.sum1
    (EPL lane-local multiply-adds and a 6-level butterfly) with its few operations."""
    B = hp.block_rows(epl)
    k_lp = -(-N // B) + epl + 6 + 6 + 4 + hp.C_LINK + 1 + K_TAU + epl + 6 + 6
    k_g = N + 2 + epl + 6 + hp.C_LINK + 1 + K_TAU + epl + 6 + 6
    return k_lp * hp.U * np.asarray(lpa, dtype=np.float64), k_g * hp.U * np.asarray(ga, dtype=np.float64)


def hier_case(model, x, y, group, mp, theta, epl):
    lp, g, lpa, ga = numpy_logp_grad(model, x, y, group, mp, theta, dtype=np.longdouble)
    blp, bg = hier_bound(lpa, ga, len(y), np.atleast_2d(theta).shape[1] - x.shape[1] - 1, epl)
    return lp.astype(np.float64), g.astype(np.float64), blp, bg


def engine(lib, model, D, C, data, mp, epl=0, fma=1, **kw):
    cfg = wa.default_config(lib, fused_multiply_add=fma, waves_per_chain=1 if epl else 0, elems_per_lane=epl, **kw)
    return wa.DeviceEngine(model, D, C, cfg, params=mp, lib_path=lib, data=data)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("model", HIER, ids=IDS)
@pytest.mark.parametrize("P,J,N", [(3, 4, 37), (130, 5, 20), (10, 100, 50), (1, 1, 7)])
@pytest.mark.parametrize("fma", [0, 1])
def test_logp_grad_matches_numpy_and_finite_differences(sim, model, P, J, N, fma):
    x, y, group, mp = make_hier(model, P, J, N, seed=P + J + N)
    D = P + J + 1
    e = engine(sim, model, D, 3, (x, y, group), mp, fma=fma)
    theta = np.random.default_rng(9).normal(size=(3, D)) * 0.3
    theta[:, -1] = (0.4, -0.7, 1.1)
    before = e.positions()
    lp, g = e.logp_grad(theta)
    assert np.array_equal(e.positions(), before), "logp_grad must leave the chains' state alone"
    lp_ref, g_ref, _, _ = numpy_logp_grad(model, x, y, group, mp, theta)
    assert np.all(np.abs(lp - lp_ref) <= 1e-12 * np.abs(lp_ref).max())
    for c in range(3):
        assert np.linalg.norm(g[c] - g_ref[c]) <= 1e-12 * np.linalg.norm(g_ref[c])
    # central differences of the returned log density, every coordinate (s included)
    h = 1e-5
    for i in range(D) if D <= 12 else list(range(4)) + list(range(P, P + 4)) + [D - 1]:
        plus, minus = theta.copy(), theta.copy()
        plus[:, i] += h
        minus[:, i] -= h
        fd = (e.logp_grad(plus)[0] - e.logp_grad(minus)[0]) / (2 * h)
        assert np.all(np.abs(fd - g[:, i]) <= 1e-6 * (1.0 + np.abs(lp))), (i, fd, g[:, i])


# ---- the edge matrix against the long-double reference --------------------------------------------------------------
# Rows go in blocks of B = 16 / 8 / 4 / 2 at 2 / 4 / 8 / 16 elements per lane (the one-wavefront geometries): N at
# 1, B - 1, B, B + 1.  (P, J) put P at 1, 127, 128, 129 (the narrow row stride Dx = 128 ceil(P / 128)), J at 1 and
# large (empty groups), and num_params at the padding boundaries Dp = 64 EPL and Dp +- 1 up to 1 024.  Eight per lane:
# rows of 1, 2 and 3 slot pairs out of theta's 4, tau at coordinate 256 (the first slot of a pair) and in the last slot.
EDGE_SHAPES = {
    2: [(1, 1), (1, 126), (60, 67), (100, 20)],                  # D = 3, 128, 128, 121
    4: [(127, 1), (128, 1), (129, 126), (1, 254), (127, 128)],   # D = 129, 130, 256, 256, 256
    8: [(100, 156), (200, 150), (129, 382), (300, 211), (257, 1)],  # D = 257, 351, 512, 512, 259
    16: [(129, 894), (128, 500), (1000, 23), (300, 212)],         # D = 1024, 629, 1024, 513
}


def edge_ns(epl):
    B = hp.block_rows(epl)
    return sorted({1, max(1, B - 1), B, B + 1})


def edge_thetas(x, group, P, J, rng):
    """Four chains: moderate; saturated logits (max |x beta| = 800); s = 6 (tau = 403); s = -6."""
    D = P + J + 1
    theta = 0.3 * rng.normal(size=(4, D))
    direction = rng.normal(size=P)
    theta[1, :P] = direction * (800.0 / max(np.abs(x @ direction).max(), 1e-300))
    theta[:, -1] = (0.2, 0.1, 6.0, -6.0)
    return theta


def moved(group, J):
    """(row 0 moved to another group, the labels of row 0's group and the next one swapped)"""
    a = group.copy()
    a[0] = (group[0] + 1) % J
    b = group.copy()
    g0, g1 = group[0], (group[0] + 1) % J
    b[group == g0], b[group == g1] = g1, g0
    return a, b


def check_edges(lib, model, epl, fma):
    worst = 0.0
    rng = np.random.default_rng(epl * 10 + fma)
    for (P, J) in EDGE_SHAPES[epl]:
        for N in edge_ns(epl):
            x, y, group, mp = make_hier(model, P, J, N, seed=1000 * N + P + 7 * J)
            D = P + J + 1
            e = engine(lib, model, D, 4, (x, y, group), mp, epl=epl, fma=fma)
            assert e.lanes == 64 and e.dim_padded == 64 * epl
            theta = edge_thetas(x, group, P, J, rng)
            lp, g = e.logp_grad(theta)
            e.close()
            ref = hier_case(model, x, y, group, mp, theta, epl)
            ratio = hp.error_ratio(lp, g, ref)
            assert ratio <= 1.0, (P, J, N, ratio)
            worst = max(worst, ratio)
            if J >= 2:  # the bound could not hide a misrouted row or two groups' labels swapped
                for gm in moved(group, J):
                    assert hp.error_ratio(lp, g, hier_case(model, x, y, gm, mp, theta, epl)) >= 100.0, (P, J, N)
    return worst


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("geometry", SIM_GEOMETRIES, ids=lambda g: f"nw{g[0]}_epl{g[1]}")
@pytest.mark.parametrize("model", HIER, ids=IDS)
def test_edges_against_long_double(sim, model, geometry, fma, record_property):
    record_property("max_error_over_bound", check_edges(sim, model, geometry[1], fma))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("logistic", [False, True])
def test_reparameterization_identity(sim, logistic):
    """logp_nc(beta, z, s) == logp_c(beta, exp(s) z, s) + J s, within rounding."""
    nc, c = (HLOG, HLOG_C) if logistic else (HLIN, HLIN_C)
    P, J, N = 6, 9, 40
    x, y, group, mp = make_hier(nc, P, J, N, seed=21)
    D = P + J + 1
    theta = np.random.default_rng(2).normal(size=(4, D)) * 0.5
    theta[:, -1] = (-1.0, 0.0, 0.5, 1.5)
    lp_nc, _ = engine(sim, nc, D, 4, (x, y, group), mp).logp_grad(theta)
    tc = theta.copy()
    tc[:, P:P + J] *= np.exp(theta[:, -1])[:, None]
    lp_c, _ = engine(sim, c, D, 4, (x, y, group), mp).logp_grad(tc)
    assert np.allclose(lp_nc, lp_c + J * theta[:, -1], rtol=1e-12, atol=1e-12)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("logistic", [False, True])
def test_likelihood_equals_the_one_hot_workaround(sim, logistic):
    """The likelihood part equals a flat GLM on x widened with the group indicators, at theta_flat = [beta | v]."""
    model, flat = (HLOG, wa.MODEL_LOGISTIC_REGRESSION) if logistic else (HLIN, wa.MODEL_LINEAR_REGRESSION)
    P, J, N = 5, 12, 60
    x, y, group, mp = make_hier(model, P, J, N, seed=5)
    D = P + J + 1
    theta = np.random.default_rng(3).normal(size=(3, D)) * 0.4
    lp, _ = engine(sim, model, D, 3, (x, y, group), mp).logp_grad(theta)
    beta, z, s = split(theta, P, J)
    tau = np.exp(s)
    ll = lp - (-(beta * beta / (2 * mp[:P])).sum(1) - (z * z).sum(1) / 2 + s - tau * tau / (2 * mp[-1] ** 2))
    xw = np.concatenate([x, np.eye(J)[group]], axis=1)
    s2 = np.concatenate([mp[:P], np.ones(J)])
    tf = np.concatenate([beta, tau[:, None] * z], axis=1)
    lpf, _ = wa.DeviceEngine(flat, P + J, 3, wa.default_config(sim), params=s2, lib_path=sim,
                             data=(xw, y)).logp_grad(tf)
    llf = lpf + (tf * tf / (2 * s2)).sum(1)
    assert np.allclose(ll, llf, rtol=1e-11, atol=1e-11 * np.abs(llf).max())


def make_grouped_datasets(model, P, J, sizes, seed):
    out = []
    for k, n in enumerate(sizes):
        x, y, group, mp = make_hier(model, P, J, n, seed=seed + 31 * k)
        if k == 1:
            y = 1.0 - y if is_logistic(model) else -y
        out.append((x, y, group))
    return out, mp


@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", HIER, ids=IDS)
@pytest.mark.parametrize("geometry", SIM_GEOMETRIES, ids=lambda g: f"nw{g[0]}_epl{g[1]}")
@pytest.mark.parametrize("fma", [0, 1])
def test_datasets_equal_standalone_engines(sim, model, geometry, fma):
    """Chain c of dataset g equals chain c - g k of a standalone grouped engine on dataset g seeded with chain_offset
    g k, bit for bit: positions, logp, depths, grad-evals, rng draws, step sizes, Adam state and estimator planes over
    single and fused warmup launches and sampling."""
    epl = geometry[1]
    P, J = {2: (3, 6), 4: (130, 7), 8: (200, 150), 16: (200, 40)}[epl]
    B = hp.block_rows(epl)
    k = 2
    datasets, mp = make_grouped_datasets(model, P, J, [1, B + 1, 2 * B + 3], seed=40 + epl)
    cfg = wa.default_config(sim, fused_multiply_add=fma, waves_per_chain=1, elems_per_lane=epl)
    D = P + J + 1
    e = wa.DeviceEngine(model, D, 3 * k, cfg, params=mp, lib_path=sim, datasets=datasets)
    assert e.num_datasets == 3
    batched = drive(e, 0)
    for gi, d in enumerate(datasets):
        alone = wa.DeviceEngine(model, D, k, cfg, params=mp, lib_path=sim, data=d)
        compare_blocks(batched, drive(alone, gi * k), gi, k)
        alone.close()
    e.close()


@pytest.mark.timeout(900)
def test_short_run_is_deterministic_and_finite(sim):
    def run():
        x, y, group, mp = make_hier(HLOG, 4, 8, 30, seed=8)
        e = engine(sim, HLOG, 13, 4, (x, y, group), mp)
        return drive(e, 0)
    a, b = run(), run()
    for sa, sb in zip(a, b):
        for key in sb:
            assert np.array_equal(sa[key], sb[key], equal_nan=True), key
    assert np.all(np.isfinite(a[-1]["pos"])) and np.all(np.isfinite(a[-1]["logp"]))


@pytest.mark.timeout(900)
def test_refusals(sim):
    x, y, group, mp = make_hier(HLOG, 4, 5, 20, seed=1)
    D = 10
    cfg = wa.default_config(sim)
    with pytest.raises(ValueError, match="conditioned on data"):
        wa.DeviceEngine(HLOG, D, 2, cfg, params=mp, lib_path=sim)
    with pytest.raises(ValueError, match="reads a group per observation"):
        wa.DeviceEngine(HLOG, D, 2, cfg, params=mp, lib_path=sim, data=(np.zeros((20, D)), y))
    with pytest.raises(ValueError, match="reads a group per observation"):
        wa.DeviceEngine(HLOG, D, 2, cfg, params=mp, lib_path=sim, datasets=[(np.zeros((20, D)), y)])
    with pytest.raises(ValueError, match="reads no groups"):
        wa.DeviceEngine(wa.MODEL_LOGISTIC_REGRESSION, D, 2, cfg, params=mp, lib_path=sim,
                        data=(np.zeros((20, D)), y, group))
    with pytest.raises(ValueError, match="reads no data"):
        wa.DeviceEngine(wa.MODEL_STD_NORMAL, D, 2, cfg, lib_path=sim, data=(x, y, group))
    for bad_x in (np.zeros((20, D - 1)), np.zeros((20, D)), np.zeros((20, 0))):  # J = 0, J < 0, P = 0
        with pytest.raises(ValueError, match=r"num_params == P \+ num_groups \+ 1"):
            wa.DeviceEngine(HLOG, D, 2, cfg, params=mp, lib_path=sim, data=(bad_x, y, group))
    for v in (-1, 5):
        g2 = group.copy()
        g2[3] = v
        with pytest.raises(ValueError, match=r"every group must be in \[0, num_groups\)"):
            wa.DeviceEngine(HLOG, D, 2, cfg, params=mp, lib_path=sim, data=(x, y, g2))
    with pytest.raises(ValueError, match="must hold integers"):
        wa.DeviceEngine(HLOG, D, 2, cfg, params=mp, lib_path=sim, data=(x, y, group.astype(np.float64)))
    y2 = y.copy()
    y2[4] = 0.5
    with pytest.raises(ValueError, match=r"y in \{0, 1\}"):
        wa.DeviceEngine(HLOG, D, 2, cfg, params=mp, lib_path=sim, data=(x, y2, group))
    wa.DeviceEngine(HLIN, D, 2, cfg, params=mp, lib_path=sim, data=(x, y2, group)).close()
    with pytest.raises(ValueError, match=r"dataset 1: .*y in \{0, 1\}"):
        wa.DeviceEngine(HLOG, D, 2, cfg, params=mp, lib_path=sim, datasets=[(x, y, group), (x, y2, group)])
    with pytest.raises(ValueError, match="all \\(x, y\\) pairs or all"):
        wa.DeviceEngine(HLOG, D, 2, cfg, params=mp, lib_path=sim, datasets=[(x, y, group), (x, y)])
    for bad in (-mp, np.where(np.arange(D) == D - 1, np.inf, mp), np.where(np.arange(D) == 6, 0.0, mp)):
        with pytest.raises(ValueError, match="positive and finite"):
            wa.DeviceEngine(HLOG, D, 2, cfg, params=bad, lib_path=sim, data=(x, y, group))
    with pytest.raises(ValueError, match="one wavefront per chain"):
        wa.DeviceEngine(HLOG, D, 2, wa.default_config(sim, waves_per_chain=2, elems_per_lane=2), params=mp,
                        lib_path=sim, data=(x, y, group))
    xl = np.zeros((3, 1000))
    with pytest.raises(ValueError, match="num_params <= 1024"):
        wa.DeviceEngine(HLIN, 1100, 2, cfg, params=np.ones(1100), lib_path=sim, data=(xl, np.zeros(3), np.zeros(3, int)))
    # a flat model with (x, y) is unchanged: the same bits as before the group channel existed (its own tests), and the
    # same error for a grouped model's x
    xf = np.random.default_rng(0).normal(size=(20, 5))
    with pytest.raises(ValueError, match="data x must have shape"):
        wa.DeviceEngine(wa.MODEL_LOGISTIC_REGRESSION, 6, 2, cfg, params=np.ones(6), lib_path=sim, data=(xf, y))
    with pytest.raises(ValueError, match="not available with devices"):
        wa.walnuts_device(HLOG, model_params=mp, num_params=D, data=(x, y, group), devices=[0, 0], lib_path=sim)


@pytest.mark.timeout(1200)
def test_drop_in_calls(sim):
    """walnutpie_sample_device_observed* with groups, one block and several, under the emulation: host and resident
    draws agree, and dataset g of the datasets call equals a grouped call on dataset g alone."""
    x, y, group, mp = make_hier(HLOG, 3, 4, 25, seed=2)
    D = 8
    kw = dict(model_params=mp, num_params=D, num_chains=2, seed=9, min_warmup_iter=5, max_warmup_iter=5,
              min_sampling_iter=4, max_sampling_iter=4, lib_path=sim)
    host = wa.walnuts_device(HLOG, data=(x, y, group), **kw)
    kept, chains = wa.walnuts_device(HLOG, data=(x, y, group), keep_on_device=True, thin=1, **kw)
    for a, b in zip(host, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b))
        assert np.all(np.isfinite(np.asarray(a)))
    chains.close()
    sets, _ = make_grouped_datasets(HLOG, 3, 4, [25, 9, 14], seed=3)
    kw["num_chains"] = 6
    many = wa.walnuts_device(HLOG, datasets=sets, **kw)
    kept, views = wa.walnuts_device(HLOG, datasets=sets, keep_on_device=True, thin=1, **kw)
    assert len(many) == 6 and len(views) == 3
    for a, b in zip(many, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for v in views:
        v.close()
