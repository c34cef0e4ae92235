"""CPU tier: hierarchical regression with varying intercepts and slopes by group (walnuts_amd/csrc/models/
hier_slopes_glm.h; kVaryingSlopes on top of the group channel) under the workgroup emulation.

References: a float64 NumPy restatement of the three densities, an np.longdouble restatement with a per-chain error bound
constructed as test_hier_models_sim.hier_bound (its constant, grown by a count of the operations the slopes add, times u
times the absolute version of the computation with the slope terms in it), central finite differences, the Q = 1
identity with the MODEL_HIER_* siblings (bit for bit), the dense workaround (a flat GLM on x widened with
tau_q * onehot(g) * z_q), and the pointwise / predict / replicate hooks tied to logp_grad, to each other and to the
sampler probe.  The device side of the same kernel source is compared bit for bit in test_hier_slopes_gpu.py."""
import math
import os
import sys

import mpmath as mpm
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_reference as hp  # noqa: E402
import hp_replicate_reference as hr  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from walnuts_amd import _ffi  # noqa: E402
from test_datasets_sim import compare_blocks, drive  # noqa: E402
from test_hier_models_sim import K_TAU  # noqa: E402
from test_predict_sim import download  # noqa: E402

SLIN, SLOG, SPOIS = (wa.MODEL_HIER_LINEAR_REGRESSION_SLOPES, wa.MODEL_HIER_LOGISTIC_REGRESSION_SLOPES,
                     wa.MODEL_HIER_POISSON_REGRESSION_SLOPES)
SLOPES = (SLIN, SLOG, SPOIS)
IDS = ["linear", "logistic", "poisson"]
SIBLING = {SLIN: wa.MODEL_HIER_LINEAR_REGRESSION, SLOG: wa.MODEL_HIER_LOGISTIC_REGRESSION,
           SPOIS: wa.MODEL_HIER_POISSON_REGRESSION}
FLAT = {SLIN: wa.MODEL_LINEAR_REGRESSION, SLOG: wa.MODEL_LOGISTIC_REGRESSION, SPOIS: wa.MODEL_POISSON_REGRESSION}
KIND = {SLIN: hr.NORMAL, SLOG: hr.BERNOULLI, SPOIS: hr.POISSON}
SIM_GEOMETRIES = ((1, 2), (1, 4), (1, 8), (1, 16))
# (P, J, Q, N, geometry): the only column varies, one group, N odd and below a block; empty groups, N no multiple of
# B = 16 nor of 64; u blocks across the 128-coordinate slot-pair boundary at Dx = 256; D = 882; Q at its cap with every
# column varying; eight per lane with rows of 2 slot pairs out of 4 and N = 5 B + 1
SHAPES = [(1, 1, 2, 3, (1, 16)), (3, 6, 2, 70, (1, 2)), (130, 20, 3, 9, (1, 4)), (129, 250, 3, 61, (1, 16)),
          (7, 2, 8, 20, (1, 4)), (130, 60, 3, 21, (1, 8))]
SHAPE_IDS = ["P1J1Q2", "P3J6Q2", "P130J20Q3", "P129J250Q3", "P7J2Q8", "P130J60Q3_epl8"]
SEED = 2 ** 33 + 5


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def family(model):
    return {SLIN: "identity", SLOG: "logit", SPOIS: "log"}[model]


def dim(P, J, Q):
    return P + Q * (J + 1)


def make_slopes(model, P, J, Q, N, seed, terms=False):
    """dict(x [N, P], y [N], group [N] (row 0 in group J - 1; with J > 2 some groups stay empty when N is small), mp [D],
    offset, weights).  terms: per-row offsets and weights; the weights hold zeros, and row N - 1 has weight 0 and an
    offset (1e308) at which the link's term is not finite (identity: r^2 = inf; log: exp(eta) = inf)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    group = rng.integers(0, J, size=N).astype(np.int32)
    group[0] = J - 1
    z = np.concatenate([np.ones((N, 1)), x[:, :Q - 1]], axis=1)
    u = 0.7 * rng.normal(size=(Q, J))
    eta = x @ rng.normal(size=P) + (u[:, group].T * z).sum(1)
    offset = weights = None
    if terms:
        offset = 0.3 * rng.normal(size=N)
        weights = rng.integers(0, 4, size=N).astype(np.float64) * rng.uniform(0.5, 1.5, size=N)
        weights[N // 2] = 0.0
        weights[N - 1] = 0.0
        if N > 1:
            weights[0] = 1.25
        offset[N - 1] = 1e308
    fam = family(model)
    if fam == "logit":
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    elif fam == "log":
        y = rng.poisson(np.exp(np.clip(eta, -5, 3))).astype(np.float64)
    else:
        y = eta + rng.normal(size=N)
    mp = np.concatenate([rng.uniform(0.5, 4.0, size=P), np.ones(Q * J), rng.uniform(0.8, 2.0, size=Q)])
    return dict(x=x, y=y, group=group, mp=mp, offset=offset, weights=weights, P=P, J=J, Q=Q, N=N, D=dim(P, J, Q))


def data_of(c):
    return (c["x"], c["y"], c["group"])


def thetas(c, T, seed, scale=0.3):
    rng = np.random.default_rng(seed)
    th = scale * rng.normal(size=(T, c["D"]))
    th[:, c["D"] - c["Q"]:] = rng.uniform(-0.8, 1.1, size=(T, c["Q"]))
    return th


def numpy_parts(model, c, theta, dtype=np.float64, weights="own"):
    """Everything of the density in `dtype`, rows of weight 0 removed first (the kernel discards them by select, whatever
    their eta): dict(lp [C], g [C, D], lpa, ga -- the absolute versions, see slopes_bound --, rows -- the kept rows --,
    ln, la, r, A, eta [C, kept]: the row terms (constant dropped), their absolute versions, residuals, A_n and eta_n)."""
    w = c["weights"] if weights == "own" else weights
    keep = np.arange(c["N"]) if w is None else np.flatnonzero(np.asarray(w) != 0)
    X, Y, MP, TH = (np.asarray(a, dtype=dtype) for a in (c["x"][keep], c["y"][keep], c["mp"], np.atleast_2d(theta)))
    W = np.ones(len(keep), dtype=dtype) if w is None else np.asarray(w, dtype=dtype)[keep]
    O = np.zeros(len(keep), dtype=dtype) if c["offset"] is None else np.asarray(c["offset"], dtype=dtype)[keep]
    group = c["group"][keep]
    P, J, Q, D = c["P"], c["J"], c["Q"], c["D"]
    C, N = TH.shape[0], len(keep)
    beta, u, s = TH[:, :P], TH[:, P:P + Q * J].reshape(C, Q, J), TH[:, D - Q:]
    s2, sig2 = MP[:P], MP[D - Q:] * MP[D - Q:]
    tau = np.exp(s)  # [C, Q]
    Z = np.concatenate([np.ones((N, 1), dtype=dtype), X[:, :Q - 1]], axis=1)  # [N, Q]
    vq = tau[:, :, None] * u[:, :, group] * Z.T[None]  # [C, Q, N]
    eta = beta @ X.T + vq.sum(1) + O
    A = np.abs(beta) @ np.abs(X).T + np.abs(vq).sum(1) + np.abs(O)
    fam = family(model)
    if fam == "logit":
        sp = np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta)))
        r = Y - 1 / (1 + np.exp(-eta))
        ln = Y * eta - sp
        la = np.abs(Y * eta) + sp + 1
    elif fam == "log":
        mu = np.exp(eta)
        r = Y - mu
        ln = Y * eta - mu
        la = np.abs(Y * eta) + mu
    else:
        r = Y - eta
        ln = -r * r / 2
        la = r * r / 2
    rw, ra = W * r, W * (np.abs(r) + A)
    onehot = np.zeros((N, J), dtype=dtype)
    onehot[np.arange(N), group] = 1
    S = np.stack([(rw * Z[:, q]) @ onehot for q in range(Q)], axis=1)  # [C, Q, J]
    Sa = np.stack([(ra * np.abs(Z[:, q])) @ onehot for q in range(Q)], axis=1)
    tt = tau * tau / sig2  # [C, Q]
    prior = beta * beta / (2 * s2)
    lp = (W * ln).sum(1) - prior.sum(1) - (u * u).sum((1, 2)) / 2 + (s - tt / 2).sum(1)
    lpa = (W * (la + np.abs(r) * A)).sum(1) + prior.sum(1) + (u * u).sum((1, 2)) / 2 + (np.abs(s) + tt / 2).sum(1)
    g, ga = np.zeros_like(TH), np.zeros_like(TH)
    g[:, :P] = rw @ X - beta / s2
    ga[:, :P] = ra @ np.abs(X) + np.abs(beta) / s2
    g[:, P:P + Q * J] = (tau[:, :, None] * S - u).reshape(C, Q * J)
    ga[:, P:P + Q * J] = (tau[:, :, None] * Sa + np.abs(u)).reshape(C, Q * J)
    g[:, D - Q:] = tau * (u * S).sum(2) + 1 - tt
    ga[:, D - Q:] = tau * (np.abs(u) * Sa).sum(2) + 1 + tt
    return dict(lp=lp, g=g, lpa=lpa, ga=ga, rows=keep, ln=ln, la=la, r=r, A=A, eta=eta)


# What the slopes add to an evaluation, beyond what test_hier_models_sim.hier_bound counts (its constant is kept): per
# q >= 1 the product tau_q * u_q (1 rounding) and the multiply-add into v (2 unfused), each relative to a partial sum
# that A_n bounds: 3 (Q - 1) on eta, which the link carries into every term and residual; the product r * z_q before
# the scatter: 1.  Row terms (hier_bound was written without them): the offset's add 1, w * r 1, mad(w, t, ll) 1 more
# than the add it replaces: 3.  K_TAU covers every tau_q at once, each error being relative to its own term of A_n.
def k_extra(Q, terms):
    return 3 * (Q - 1) + 1 + (3 if terms else 0)


def slopes_bound(lpa, ga, N, Q, epl, terms):
    """hier_bound's constants plus k_extra, times u times the absolute version (slope terms included: numpy_parts)."""
    B = hp.block_rows(epl)
    k_lp = -(-N // B) + epl + 6 + 6 + 4 + hp.C_LINK + 1 + K_TAU + epl + 6 + 6 + k_extra(Q, terms)
    k_g = N + 2 + epl + 6 + hp.C_LINK + 1 + K_TAU + epl + 6 + 6 + k_extra(Q, terms)
    return k_lp * hp.U * np.asarray(lpa, dtype=np.float64), k_g * hp.U * np.asarray(ga, dtype=np.float64)


def slopes_case(model, c, theta, epl):
    p = numpy_parts(model, c, theta, dtype=np.longdouble)
    blp, bg = slopes_bound(p["lpa"], p["ga"], c["N"], c["Q"], epl, c["weights"] is not None)
    return p["lp"].astype(np.float64), p["g"].astype(np.float64), blp, bg


def config(lib, geometry=None, fma=1):
    """(trees of at most 3 doublings and steps halved at most twice: the model's code is the same at every depth, and
    the emulation's time goes with the number of gradient evaluations)"""
    nw, epl = geometry if geometry else (0, 0)
    return wa.default_config(lib, fused_multiply_add=fma, waves_per_chain=nw, elems_per_lane=epl, max_trajectory_doublings=3,
                             max_step_halvings=2)


def engine(lib, model, c, C, geometry=None, fma=1, varying=None, **kw):
    kw.setdefault("offset", c["offset"])
    kw.setdefault("weights", c["weights"])
    if "datasets" not in kw and "data" not in kw:
        kw["data"] = data_of(c)
    return wa.DeviceEngine(model, c["D"], C, config(lib, geometry, fma), params=c["mp"], lib_path=lib,
                           varying=c["Q"] if varying is None else varying, **kw)


def run(lib, model, c, C, geometry, fma, warm=6, samp=6):
    """logp_grad at fixed positions, then warmup and sampling transitions: everything the device must reproduce"""
    e = engine(lib, model, c, C, geometry, fma)
    theta = thetas(c, C, seed=c["D"])
    lp, g = e.logp_grad(theta)
    e.init_positions(seed=17, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=18)
    e.warmup_step()
    e.warmup_steps(warm - 1)
    e.freeze()
    e.sample_step()
    e.sample_steps(samp - 1)
    e.check()
    out = dict(lp_eval=lp, g_eval=g, pos=e.positions(), logp=e.logp(), depth=e.depths(), grads=e.grad_evals(),
               rng=e.rng_draws(), steps=e.step_sizes(), inv_mass=e.inv_mass())
    e.close()
    return out


HOOK_LENGTHS = (3, 2)


def hooks(lib, model, c, geometry, fma):
    """The three hooks' outputs on two ragged chains: the log_lik, predict and replicate matrices, log_predictive and
    predict_fold, the generated chains block and the 12 arrays of the check (with a row mask)."""
    draws = [thetas(c, n, seed=40 + i) for i, n in enumerate(HOOK_LENGTHS)]
    ch = wa.MarkovChains.from_host(draws, lib_path=lib)
    mask = np.arange(c["N"]) % 3 != 1
    e = engine(lib, model, c, 1, geometry, fma, weights=None)
    out = dict(draws=draws)
    out["ll"] = [e.log_lik(d) for d in draws]
    out["pred"] = [e.predict(d) for d in draws]
    out["rep"] = [e.replicate(d, SEED) for d in draws]
    out["lpd"] = e.log_predictive(ch, mask)
    out["fold"] = e.predict_fold(ch)
    gen = e.replicate_chains(ch, SEED)
    out["gen"] = download(gen, max(HOOK_LENGTHS), HOOK_LENGTHS)
    gen.close()
    out["check"] = e.replicate_check(ch, SEED, mask)
    e.close()
    ch.close()
    return out


def hook_arrays(h):
    """the arrays of hooks() as one flat list (for bitwise comparisons)"""
    flat = list(h["ll"]) + [a for m in h["pred"] for a in m] + list(h["rep"]) + list(h["lpd"]) + list(h["fold"])
    return flat + list(h["gen"]) + list(h["check"])


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


# ---- values ---------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", SLOPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("terms", [False, True], ids=["plain", "terms"])
def test_logp_grad_against_long_double(sim, model, shape, terms):
    """Both arithmetic modes against the float64 restatement (1e-12 relative) and the long-double one (error / bound
    <= 1); a row moved to another group is far outside the bound."""
    P, J, Q, N, geometry = shape
    c = make_slopes(model, P, J, Q, N, seed=P + J + Q + N, terms=terms)
    theta = thetas(c, 3, seed=9)
    theta[2, c["D"] - Q:] = np.where(np.arange(Q) % 2 == 0, 3.0, -3.0)  # tau = 20 and 0.05
    p64 = numpy_parts(model, c, theta)
    ref = slopes_case(model, c, theta, geometry[1])
    for fma in (0, 1):
        e = engine(sim, model, c, 3, geometry, fma)
        assert e.lanes == 64 and e.dim_padded == 64 * geometry[1]
        before = e.positions()
        lp, g = e.logp_grad(theta)
        assert np.array_equal(e.positions(), before)
        e.close()
        assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
        assert np.all(np.abs(lp - p64["lp"]) <= 1e-12 * np.abs(p64["lpa"]))
        for ch in range(3):
            assert np.linalg.norm(g[ch] - p64["g"][ch]) <= 1e-12 * np.linalg.norm(p64["ga"][ch])
        ratio = hp.error_ratio(lp, g, ref)
        assert ratio <= 1.0, (shape, fma, ratio)
        if J >= 2 and (c["weights"] is None or c["weights"][0] != 0):
            moved = dict(c, group=c["group"].copy())
            moved["group"][0] = (c["group"][0] + 1) % J
            assert hp.error_ratio(lp, g, slopes_case(model, moved, theta, geometry[1])) >= 100.0, shape


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", SLOPES, ids=IDS)
def test_finite_differences_of_every_coordinate_class(sim, model):
    P, J, Q, N = 3, 4, 3, 37
    c = make_slopes(model, P, J, Q, N, seed=3, terms=True)
    D = c["D"]
    e = engine(sim, model, c, 3)
    theta = thetas(c, 3, seed=1)
    lp, g = e.logp_grad(theta)
    h = 1e-5
    for i in range(D):  # beta, every u_q block, every s_q
        plus, minus = theta.copy(), theta.copy()
        plus[:, i] += h
        minus[:, i] -= h
        fd = (e.logp_grad(plus)[0] - e.logp_grad(minus)[0]) / (2 * h)
        assert np.all(np.abs(fd - g[:, i]) <= 1e-6 * (1.0 + np.abs(lp))), (i, fd, g[:, i])
    e.close()


# ---- identities -----------------------------------------------------------------------------------------------------
@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", SLOPES, ids=IDS)
@pytest.mark.parametrize("geometry", SIM_GEOMETRIES, ids=lambda g: f"nw{g[0]}_epl{g[1]}")
@pytest.mark.parametrize("fma", [0, 1])
def test_one_varying_coefficient_is_the_hier_model_bit_for_bit(sim, model, geometry, fma):
    """varying=1: logp_grad and a warmup + sampling drive give the bits of MODEL_HIER_*, with and without row terms."""
    epl = geometry[1]
    P, J = {2: (3, 6), 4: (130, 7), 8: (200, 150), 16: (200, 40)}[epl]
    N = 2 * hp.block_rows(epl) + 3
    for terms in (False, True):
        c = make_slopes(model, P, J, 1, N, seed=40 + epl, terms=terms)
        theta = thetas(c, 2, seed=5)
        results = []
        for m in (model, SIBLING[model]):
            kw = dict(varying=1) if m == model else {}
            e = wa.DeviceEngine(m, c["D"], 2, config(sim, geometry, fma), params=c["mp"], lib_path=sim, data=data_of(c),
                                offset=c["offset"], weights=c["weights"], **kw)
            lp, g = e.logp_grad(theta)
            results.append([dict(lp=lp, g=g)] + drive(e, 0))
            e.close()
        for a, b in zip(*results):
            for key in b:
                assert np.array_equal(a[key], b[key], equal_nan=True), (terms, key)


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", SLOPES, ids=IDS)
def test_gradient_equals_the_dense_workaround(sim, model):
    """With s fixed, the gradient in (beta, u) is that of a flat GLM on [x | tau_q onehot(g) z_q] with unit prior
    variance on u, within the two bounds (the flat side: hp.glm_bound on the same absolute version)."""
    P, J, Q, N = 5, 6, 3, 45
    c = make_slopes(model, P, J, Q, N, seed=5)
    D, F = c["D"], P + Q * J
    theta = thetas(c, 1, seed=3)
    e = engine(sim, model, c, 1)
    epl = e.dim_padded // 64
    _, g = e.logp_grad(theta)
    e.close()
    tau = np.exp(theta[0, D - Q:])
    z = np.concatenate([np.ones((N, 1)), c["x"][:, :Q - 1]], axis=1)
    wide = np.concatenate([c["x"]] + [tau[q] * np.eye(J)[c["group"]] * z[:, q:q + 1] for q in range(Q)], axis=1)
    f = wa.DeviceEngine(FLAT[model], F, 1, config(sim), params=np.concatenate([c["mp"][:P], np.ones(Q * J)]),
                        lib_path=sim, data=(wide, c["y"]))
    epl_flat = f.dim_padded // 64
    _, gf = f.logp_grad(theta[:, :F])
    f.close()
    p = numpy_parts(model, c, theta, dtype=np.longdouble)
    ga = p["ga"].astype(np.float64)[:, :F]
    bound = slopes_bound(p["lpa"], p["ga"], N, Q, epl, False)[1][:, :F] + hp.glm_bound(p["lpa"], ga, N, epl_flat)[1]
    # (the flat model multiplies tau_q into the column on the host: one more rounding per row, inside K_TAU's slack)
    assert np.all(np.abs(g[:, :F] - gf) <= bound), np.max(np.abs(g[:, :F] - gf) / bound)
    assert np.linalg.norm(g[0, P:F]) > 0


# ---- hooks ----------------------------------------------------------------------------------------------------------
def row_const(model, y):
    if family(model) == "identity":
        with mpm.workdps(50):
            return np.full(y.shape, float(-mpm.log(2 * mpm.pi) / 2))   # fl(-1/2 log 2 pi), rounded once
    if family(model) == "log":
        return np.array([-math.lgamma(v + 1.0) for v in y])
    return np.zeros(y.shape)


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", SLOPES, ids=IDS)
@pytest.mark.parametrize("shape", [SHAPES[i] for i in (1, 2, 4, 5)], ids=[SHAPE_IDS[i] for i in (1, 2, 4, 5)])
def test_hooks(sim, model, shape):
    """pointwise(): every row term against long double, and sum_n w_n (l_n - c_n) + prior against logp_grad's logp.
    predict(): eta is pointwise()'s through an exactly vanishing residual (linear: y := eta gives l_n = c_n, bit for
    bit), mu and v are the link's of eta.  replicate(): the sampler probe fed predict()'s mu, under the matching keys."""
    P, J, Q, N, geometry = shape
    epl = geometry[1]
    c = make_slopes(model, P, J, Q, N, seed=11 + P, terms=True)
    c["offset"][N - 1] = 0.25   # (the hooks apply no weights: every row is evaluated)
    h = hooks(sim, model, c, geometry, 1)
    cn = row_const(model, c["y"])
    k_row = epl + 6 + hp.C_LINK + 1 + K_TAU + k_extra(Q, True) + 2
    lib = _ffi.load_library(sim)
    for ci, (theta, ll, (eta, mu, v), rep, gen) in enumerate(zip(h["draws"], h["ll"], h["pred"], h["rep"], h["gen"])):
        p = numpy_parts(model, c, theta, dtype=np.longdouble, weights=None)
        bound = k_row * hp.U * (p["la"] + np.abs(p["r"]) * p["A"]).astype(np.float64) + hp.U * np.abs(cn)
        assert np.all(np.abs(ll - (p["ln"] + cn).astype(np.float64)) <= bound)
        # the tie to the sampler's density, under the case's weights
        e = engine(sim, model, c, len(theta), geometry, 1)
        lp, _ = e.logp_grad(theta)
        e.close()
        pw = numpy_parts(model, c, theta, dtype=np.longdouble)
        w = np.asarray(c["weights"], dtype=np.longdouble)
        prior = pw["lp"] - (w[pw["rows"]] * pw["ln"]).sum(1)
        total = (w * (ll.astype(np.longdouble) - cn)).sum(1) + prior
        slack = 2 * slopes_bound(pw["lpa"], pw["ga"], N, Q, epl, True)[0] + (c["weights"] * bound).sum(1)
        assert np.all(np.abs((total - lp).astype(np.float64)) <= slack)
        # predict: mu, v of eta; replicate: the probe
        if family(model) == "identity":
            assert np.array_equal(mu, eta) and np.all(v == 1.0)
            for t in range(len(theta)):
                e = engine(sim, model, dict(c, y=eta[t]), 1, geometry, 1, weights=None)
                assert np.array_equal(e.log_lik(theta[t:t + 1])[0], cn), "predict()'s eta is not pointwise()'s"
                e.close()
        else:
            ref_mu = np.exp(eta) if family(model) == "log" else 1 / (1 + np.exp(-eta))
            assert np.allclose(mu, ref_mu, rtol=1e-13, atol=0)
            assert np.allclose(v, ref_mu if family(model) == "log" else ref_mu * (1 - ref_mu), rtol=1e-12, atol=0)
        k_eta = epl + 6 + 1 + K_TAU + k_extra(Q, True)
        assert np.all(np.abs(eta - p["eta"].astype(np.float64)) <= k_eta * hp.U * p["A"].astype(np.float64))
        for t in range(len(theta)):
            ones = np.ones(N)
            assert np.array_equal(rep[t], hr.sampler_probe(lib, KIND[model], mu[t], ones, SEED, t, 0, 0, hr.GATHER)[0])
            assert np.array_equal(gen[t], hr.sampler_probe(lib, KIND[model], mu[t], ones, SEED, ci, t, 0, hr.GATHER)[0])


@pytest.mark.timeout(1800)
def test_hooks_invariance(sim, monkeypatch):
    """Another grid: identical bits everywhere.  Another row order: the per-row outputs permute, bit for bit."""
    P, J, Q, N, geometry = SHAPES[1]
    c = make_slopes(SPOIS, P, J, Q, N, seed=8, terms=True)
    c["offset"][N - 1] = 0.25
    base = hooks(sim, SPOIS, c, geometry, 1)
    monkeypatch.setenv("WALNUTS_AMD_POINTWISE_GRID", "1")
    other = hooks(sim, SPOIS, c, geometry, 1)
    monkeypatch.delenv("WALNUTS_AMD_POINTWISE_GRID")
    assert same(hook_arrays(base), hook_arrays(other))
    perm = np.random.default_rng(4).permutation(N)
    cp = dict(c, x=c["x"][perm], y=c["y"][perm], group=c["group"][perm], offset=c["offset"][perm])
    e = engine(sim, SPOIS, cp, 1, geometry, 1, weights=None)
    for d, ll, (eta, mu, v) in zip(base["draws"], base["ll"], base["pred"]):
        assert np.array_equal(e.log_lik(d), ll[:, perm])
        assert same(e.predict(d), (eta[:, perm], mu[:, perm], v[:, perm]))
    e.close()
    # a row mask: the masked rows are not evaluated, the others keep their bits
    lpd, mean, var, count = base["lpd"]
    off = np.arange(N) % 3 == 1
    assert np.all(count[off] == 0) and np.all(np.isnan(lpd[off])) and np.all(count[~off] == sum(HOOK_LENGTHS))
    ch = wa.MarkovChains.from_host(base["draws"], lib_path=sim)
    e = engine(sim, SPOIS, c, 1, geometry, 1, weights=None)
    full = e.log_predictive(ch)
    e.close()
    ch.close()
    assert all(np.array_equal(a[~off], b[~off]) for a, b in zip(full, base["lpd"]))


# ---- runs -----------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", SLOPES, ids=IDS)
def test_datasets_and_weight_sets_equal_standalone_engines(sim, model):
    P, J, Q, geometry, k = 3, 4, 2, (1, 2), 2
    B = hp.block_rows(2)
    cases = [make_slopes(model, P, J, Q, n, seed=60 + 7 * i) for i, n in enumerate((1, B + 1, 2 * B + 3))]
    mp = cases[0]["mp"]
    cfg = config(sim, geometry, 1)
    D = cases[0]["D"]
    e = wa.DeviceEngine(model, D, 3 * k, cfg, params=mp, lib_path=sim, datasets=[data_of(c) for c in cases], varying=Q)
    assert e.num_datasets == 3
    batched = drive(e, 0)
    e.close()
    for gi, c in enumerate(cases):
        alone = wa.DeviceEngine(model, D, k, cfg, params=mp, lib_path=sim, data=data_of(c), varying=Q)
        compare_blocks(batched, drive(alone, gi * k), gi, k)
        alone.close()
    c = cases[2]
    rng = np.random.default_rng(2)
    sets = rng.integers(0, 3, size=(2, c["N"])).astype(np.float64)
    e = wa.DeviceEngine(model, D, 2 * k, cfg, params=mp, lib_path=sim, data=data_of(c), weight_sets=sets, varying=Q)
    batched = drive(e, 0)
    e.close()
    for gi in range(2):
        alone = wa.DeviceEngine(model, D, k, cfg, params=mp, lib_path=sim, data=data_of(c), weights=sets[gi], varying=Q)
        compare_blocks(batched, drive(alone, gi * k), gi, k)
        alone.close()


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", SLOPES, ids=IDS)
def test_non_finite_tau(sim, model):
    """Chains placed at s_q = +-800: IEEE results, the other chains stay finite, check() is clean."""
    c = make_slopes(model, 4, 3, 3, 30, seed=4)
    D, Q = c["D"], c["Q"]
    e = engine(sim, model, c, 5, (1, 2), 1)
    e.init_positions(seed=1, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=2)
    pos = e.positions()
    pos[0, D - 1], pos[1, D - 1], pos[2, D - Q] = 800.0, -800.0, 800.0
    lp, g = e.logp_grad(pos)
    assert np.all(np.isfinite(lp[3:])) and np.all(np.isfinite(g[3:]))
    assert not np.isfinite(lp[0]) or not np.all(np.isfinite(g[0]))
    assert not np.isfinite(lp[2]) or not np.all(np.isfinite(g[2]))
    e.set_positions(pos)
    e.warmup_steps(4)
    e.freeze()
    e.sample_steps(4)
    e.check()
    assert np.all(np.isfinite(e.positions()[3:])) and np.all(np.isfinite(e.logp()[3:]))
    e.close()


@pytest.mark.timeout(1800)
def test_drop_in_calls_and_wrappers(sim):
    """walnuts_device with data=(x, y, group), varying=2 and with datasets=; host draws equal kept-on-device draws; the
    scoring, predicting and replicating wrappers take the fit."""
    c = make_slopes(SLOG, 3, 4, 2, 25, seed=2)
    D = c["D"]
    kw = dict(model_params=c["mp"], num_params=D, num_chains=2, seed=9, min_warmup_iter=5, max_warmup_iter=5,
              min_sampling_iter=4, max_sampling_iter=4, lib_path=sim, varying=2)
    host = wa.walnuts_device(SLOG, data=data_of(c), **kw)
    kept, chains = wa.walnuts_device(SLOG, data=data_of(c), keep_on_device=True, thin=1, **kw)
    for a, b in zip(host, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.all(np.isfinite(np.asarray(a)))
    common = dict(num_params=D, data=data_of(c), lib_path=sim, varying=2)
    res = wa.log_predictive(SLOG, chains, **common)
    assert res.lpd.shape == (25,) and np.all(np.isfinite(res.lpd))
    pr = wa.predict(SLOG, chains, **common)
    assert pr.mean.shape == (25,) and np.all((pr.mean > 0) & (pr.mean < 1))
    pd = wa.predict_draws(SLOG, chains, **common)
    assert pd.dims() == 25
    pd.close()
    rd = wa.replicate_draws(SLOG, chains, seed=3, **common)
    assert rd.dims() == 25
    rd.close()
    ppc = wa.posterior_predictive_check(SLOG, chains, seed=3, **common)
    assert np.all((ppc.p_value["mean"] >= 0) & (ppc.p_value["mean"] <= 1))
    chains.close()
    folds = np.ones((2, 25))
    folds[0, ::2], folds[1, 1::2] = 0.0, 0.0
    kw4 = dict(kw, num_chains=4)
    _, views = wa.walnuts_device(SLOG, data=data_of(c), weight_sets=folds, keep_on_device=True, **kw4)
    kf = wa.kfold_elpd(SLOG, views, num_params=D, data=data_of(c), weight_sets=folds, lib_path=sim, varying=2)
    assert kf.lpd.shape == (25,) and np.isfinite(kf.elpd)
    for v in views:
        v.close()
    sets = [data_of(make_slopes(SLOG, 3, 4, 2, n, seed=3 + n)) for n in (25, 9, 14)]
    kw["num_chains"] = 6
    many = wa.walnuts_device(SLOG, datasets=sets, **kw)
    kept, views = wa.walnuts_device(SLOG, datasets=sets, keep_on_device=True, thin=1, **kw)
    assert len(many) == 6 and len(views) == 3
    for a, b in zip(many, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for v in views:
        v.close()


# ---- refusals -------------------------------------------------------------------------------------------------------
def c_abi_error(lib_path, model, D, x, y, group, J, Q, mp=None):
    """wn_engine_create_observed with a hand-filled wn_observations -> the error message ('' if it succeeds)"""
    import ctypes as C
    lib = _ffi.load_library(lib_path)
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    group = np.ascontiguousarray(group, dtype=np.int32)
    mp = np.ones(D) if mp is None else np.ascontiguousarray(mp, dtype=np.float64)
    obs = _ffi.Observations()
    obs.x, obs.y, obs.num_obs = x.ctypes.data_as(_ffi._dp), y.ctypes.data_as(_ffi._dp), y.size
    obs.group, obs.num_groups, obs.num_varying = group.ctypes.data_as(_ffi._i32p), J, Q
    cfg = wa.default_config(lib_path)
    h, err = C.c_void_p(), C.c_void_p()
    rc = lib.wn_engine_create_observed(C.byref(h), model, D, mp.ctypes.data_as(_ffi._dp), C.byref(obs), 2, C.byref(cfg),
                                       C.byref(err))
    if rc == 0:
        lib.wn_engine_destroy(h)
        return ""
    try:
        _ffi.check(lib, rc, err)
    except ValueError as ex:
        return str(ex)
    raise AssertionError("not a config error")


@pytest.mark.timeout(900)
def test_refusals(sim):
    lib = _ffi.load_library(sim)
    N = 6
    y, g = np.zeros(N), np.zeros(N, dtype=np.int32)
    cfg = wa.default_config(sim)

    def py(model, D, P, Q, match, group=g):
        with pytest.raises(ValueError, match=match):
            wa.DeviceEngine(model, D, 2, cfg, params=np.ones(D), lib_path=sim, data=(np.zeros((N, P)), y, group), varying=Q)

    # Q outside [1, 8]
    assert "1 <= num_varying <= 8, got 9" in c_abi_error(sim, SLIN, 9 + 9 * 2, np.zeros((N, 9)), y, g, 1, 9)
    assert "1 <= num_varying <= 8, got -1" in c_abi_error(sim, SLIN, 5, np.zeros((N, 3)), y, g, 1, -1)
    py(SLIN, 9 + 9 * 2, 9, 9, "1 <= num_varying <= 8, got 9")
    py(SLIN, 5, 3, 0, "varying must be at least 1")
    assert lib.wn_model_data_columns_varying(SLIN, 27, 1, 9) == -1
    # Q - 1 <= P
    assert "num_varying - 1 <= P, got num_varying 3, P 1" in c_abi_error(sim, SLOG, 1 + 3 * 2, np.zeros((N, 1)), y, g, 1, 3)
    py(SLOG, 7, 1, 3, "num_varying - 1 <= P, got num_varying 3, P 1")
    assert lib.wn_model_data_columns_varying(SLOG, 7, 1, 3) == -1
    # P >= 1, J >= 1, num_params == P + Q (J + 1)
    msg = r"num_params == P \+ num_varying \* \(num_groups \+ 1\)"
    assert "got num_params 4, num_groups 1, num_varying 2" in c_abi_error(sim, SPOIS, 4, np.zeros((N, 1)), y, g, 1, 2)  # P = 0
    assert "got num_params 6, num_groups 0, num_varying 2" in c_abi_error(sim, SPOIS, 6, np.zeros((N, 4)), y, g, 0, 2)  # J = 0
    py(SPOIS, 6, 4, 2, msg)   # J = 0
    py(SPOIS, 4, 4, 2, msg)   # J = -1
    py(SPOIS, 7, 2, 2, "must be a multiple of varying .*num_params 7, P 2, varying 2")
    assert lib.wn_model_data_columns_varying(SPOIS, 4, 1, 2) == -1 and lib.wn_model_data_columns_varying(SPOIS, 6, 0, 2) == -1
    # D <= 1024
    py(SLIN, 1100, 1000, 2, "num_params <= 1024")
    assert "num_params <= 1024" in c_abi_error(sim, SLIN, 1100, np.zeros((N, 1000)), y, g, 49, 2)
    # num_varying > 1 for a model without the trait
    for m in (wa.MODEL_HIER_LINEAR_REGRESSION, wa.MODEL_HIER_POISSON_REGRESSION_CENTERED):
        assert "has no varying slopes" in c_abi_error(sim, m, 7, np.zeros((N, 3)), y, g, 1, 2)
        py(m, 7, 3, 2, "has no varying slopes")
    with pytest.raises(ValueError, match="has no varying slopes"):
        wa.DeviceEngine(wa.MODEL_LINEAR_REGRESSION, 3, 2, cfg, params=np.ones(3), lib_path=sim, data=(np.zeros((N, 3)), y),
                        varying=2)
    # what is accepted, and the columns the library reports
    assert c_abi_error(sim, SLIN, 7, np.zeros((N, 3)), y, g, 1, 2) == ""
    assert c_abi_error(sim, SLIN, 5, np.zeros((N, 3)), y, g, 1, 0) == ""   # 0: the intercept alone
    assert lib.wn_model_data_columns_varying(SLIN, 7, 1, 2) == 3
    assert lib.wn_model_data_columns_varying(SLIN, 5, 1, 0) == 3 == lib.wn_model_data_columns(SLIN, 5, 1)
    for m, D, J in ((wa.MODEL_HIER_LINEAR_REGRESSION, 9, 3), (wa.MODEL_LINEAR_REGRESSION, 9, 0),
                    (wa.MODEL_NEG_BINOMIAL_REGRESSION, 9, 0), (wa.MODEL_STD_NORMAL, 9, 0)):
        assert lib.wn_model_data_columns_varying(m, D, J, 1) == lib.wn_model_data_columns(m, D, J)
        assert lib.wn_model_data_columns_varying(m, D, J, 2) == -1
    # the model's own checks: sigma_q, y, groups
    bad = np.ones(7)
    bad[5] = -1.0
    assert "positive and finite" in c_abi_error(sim, SLIN, 7, np.zeros((N, 3)), y, g, 1, 2, mp=bad)
    assert "every y to be a count" in c_abi_error(sim, SPOIS, 7, np.zeros((N, 3)), y + 0.5, g, 1, 2)
    py(SLOG, 7, 3, 2, r"every group must be in \[0, num_groups\)", group=g + 1)
    with pytest.raises(ValueError, match="reads a group per observation"):
        wa.DeviceEngine(SLOG, 7, 2, cfg, params=np.ones(7), lib_path=sim, data=(np.zeros((N, 7)), y), varying=2)
