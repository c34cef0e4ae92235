"""CPU tier: varying intercepts and slopes by group with an estimated noise level (walnuts_amd/csrc/models/
hier_slopes_scale_glm.h: hier_linear_regression_slopes_sigma, kVaryingSlopes + kScaleParam) under the workgroup emulation.

References: tests/helpers/hp_hier_slopes_scale_reference.py (np.longdouble dot products, mpmath row terms, an error bound
per chain of the form K * u * the absolute version of the computation, K being hp_hier_scale_reference's constants plus a
count of the operations the slopes add), a float64 NumPy restatement, central finite differences, the two anchors (Q = 1
is hier_linear_regression_sigma bit for bit; s = 0 is hier_linear_regression_slopes), the dense workaround (the flat
linear_regression_sigma on x widened with the indicator-times-covariate columns), the pointwise / predict / replicate hooks
against the hp_* references and the sampler probe, datasets and weight sets against stand-alone engines, the refusals by
their messages, the front-end queries and the convergence of the exact posterior's quadrature.  The device side of the same
kernel source is compared bit for bit in test_hier_slopes_scale_gpu.py.

The worst error / bound over this file's references is printed per test and recorded in DESIGN.md 3.8.12."""
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
import hp_math_reference as hm  # noqa: E402
import hp_pointwise_reference as hpw  # noqa: E402
import hp_predict_reference as hpp  # noqa: E402
import hp_reference as hp  # noqa: E402
import test_hier_scale_sim as scale_sim  # noqa: E402
import test_hier_slopes_sim as slopes_sim  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from walnuts_amd import _ffi  # noqa: E402
from test_datasets_sim import compare_blocks, drive  # noqa: E402
from test_predict_sim import download  # noqa: E402

MODEL = wa.MODEL_HIER_LINEAR_REGRESSION_SLOPES_SIGMA
assert MODEL == hss.MODEL == 40
HSIG, SLIN = wa.MODEL_HIER_LINEAR_REGRESSION_SIGMA, wa.MODEL_HIER_LINEAR_REGRESSION_SLOPES
NAME = "hier_linear_regression_slopes_sigma"
SIM_GEOMETRIES = ((1, 2), (1, 4), (1, 8), (1, 16))
# (P, J, Q, N, geometry): the minimum; five blocks of 16 rows, the last partial; D = 128, s_{Q-1} and s share lane 63;
# D = 129, s_{Q-1} at coordinate 127 and s at 128: the scales straddle a slot pair; two slot pairs of x and a partial
# block; Q at its cap; eight per lane; sixteen per lane; D = 1024, s in the last slot of lane 63
SHAPES = [(1, 1, 2, 3, (1, 16)), (3, 6, 2, 70, (1, 2)), (3, 61, 2, 5, (1, 2)), (4, 61, 2, 5, (1, 4)),
          (130, 20, 3, 9, (1, 4)), (7, 2, 8, 20, (1, 4)), (130, 60, 3, 21, (1, 8)), (129, 250, 3, 61, (1, 16)),
          (1, 510, 2, 5, (1, 16))]
SHAPE_IDS = ["P1J1Q2N3", "P3J6Q2N70", "P3J61Q2N5", "P4J61Q2N5", "P130J20Q3N9", "P7J2Q8N20", "P130J60Q3N21",
             "P129J250Q3N61", "P1J510Q2N5"]
assert [hss.dim(P, J, Q) for P, J, Q, _, _ in SHAPES] == [6, 18, 128, 129, 194, 32, 314, 883, 1024]
SEED = 2 ** 33 + 5
HOOK_LENGTHS = (3, 2)


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def make_case(P, J, Q, N, seed, terms=False):
    """dict(x [N, P], y [N], group [N] (row 0 in group J - 1; with J > 2 some groups stay empty when N is small), mp [D],
    offset, weights).  terms: per-row offsets and weights; the weights hold zeros, and row N - 1 has weight 0 and an
    offset (1e308) at which the residual is huge and the family's term is not finite."""
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
    y = eta + 0.8 * rng.normal(size=N)
    mp = np.concatenate([rng.uniform(0.5, 4.0, size=P), np.ones(Q * J), rng.uniform(0.8, 2.0, size=Q + 1)])
    return dict(x=x, y=y, group=group, mp=mp, offset=offset, weights=weights, P=P, J=J, Q=Q, N=N, D=hss.dim(P, J, Q))


def data_of(c):
    return (c["x"], c["y"], c["group"])


def thetas(c, T, seed, scale=0.3):
    rng = np.random.default_rng(seed)
    th = scale * rng.normal(size=(T, c["D"]))
    th[:, c["D"] - c["Q"] - 1:] = rng.uniform(-0.8, 1.1, size=(T, c["Q"] + 1))
    return th


def numpy_logp_grad(c, theta):
    """float64 NumPy restatement (rows of weight 0 removed first)."""
    w = c["weights"]
    keep = np.arange(c["N"]) if w is None else np.flatnonzero(w != 0)
    X, Y, group = c["x"][keep], c["y"][keep], c["group"][keep]
    n = len(keep)
    W = np.ones(n) if w is None else w[keep]
    O = np.zeros(n) if c["offset"] is None else c["offset"][keep]
    P, J, Q, D, MP = c["P"], c["J"], c["Q"], c["D"], c["mp"]
    TH = np.atleast_2d(theta)
    C = TH.shape[0]
    beta, u, sq, s = TH[:, :P], TH[:, P:P + Q * J].reshape(C, Q, J), TH[:, D - 1 - Q:D - 1], TH[:, D - 1]
    tau = np.exp(sq)
    Z = np.concatenate([np.ones((n, 1)), X[:, :Q - 1]], axis=1)
    eta = beta @ X.T + (tau[:, :, None] * u[:, :, group] * Z.T[None]).sum(1) + O
    isig2 = np.exp(-2 * s)[:, None]
    d = Y - eta
    rw = W * d * isig2
    ll = -0.5 * d * d * isig2 - s[:, None]
    ds = d * d * isig2 - 1
    onehot = np.zeros((n, J))
    onehot[np.arange(n), group] = 1
    S = np.stack([(rw * Z[:, q]) @ onehot for q in range(Q)], axis=1)
    tt = tau * tau / MP[D - 1 - Q:D - 1] ** 2
    ss = np.exp(2 * s) / MP[D - 1] ** 2
    lp = ((W * ll).sum(1) - (beta * beta / (2 * MP[:P])).sum(1) - (u * u).sum((1, 2)) / 2 + (sq - tt / 2).sum(1)
          + (s - ss / 2))
    g = np.zeros_like(TH)
    g[:, :P] = rw @ X - beta / MP[:P]
    g[:, P:P + Q * J] = (tau[:, :, None] * S - u).reshape(C, Q * J)
    g[:, D - 1 - Q:D - 1] = tau * (u * S).sum(2) + 1 - tt
    g[:, D - 1] = (W * ds).sum(1) + 1 - ss
    return lp, g


def config(lib, geometry=None, fma=1):
    """(trees of at most 3 doublings and steps halved at most twice: the model's code is the same at every depth, and
    the emulation's time goes with the number of gradient evaluations)"""
    nw, epl = geometry if geometry else (0, 0)
    return wa.default_config(lib, fused_multiply_add=fma, waves_per_chain=nw, elems_per_lane=epl, max_trajectory_doublings=3,
                             max_step_halvings=2)


def engine(lib, c, num_chains, geometry=None, fma=1, model=MODEL, **kw):
    kw.setdefault("offset", c["offset"])
    kw.setdefault("weights", c["weights"])
    if "datasets" not in kw and "data" not in kw:
        kw["data"] = data_of(c)
    return wa.DeviceEngine(model, c["D"], num_chains, config(lib, geometry, fma), params=c["mp"], lib_path=lib,
                           varying=c["Q"], **kw)


def run(lib, c, num_chains, geometry, fma, warm=6, samp=6, model=MODEL):
    """logp_grad at fixed positions, then warmup and sampling transitions: everything the device must reproduce (the nine
    arrays of test_hier_scale_sim.run)"""
    e = engine(lib, c, num_chains, geometry, fma, model=model)
    theta = thetas(c, num_chains, seed=c["D"])
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


def hook_case(P, J, Q, N, seed):
    """a case for the hooks: offsets everywhere (the last row's non-zero and finite), no weights applied"""
    c = make_case(P, J, Q, N, seed=seed, terms=True)
    c["offset"][N - 1] = 0.25
    return c


def hook_mask(N):
    """rows n % 3 == 1 masked; row N - 1, whose offset is non-zero, live whenever N % 3 != 2"""
    return np.arange(N) % 3 != 1


def hooks(lib, c, geometry, fma, model=MODEL):
    """The three hooks' outputs on two ragged chains: the log_lik, predict and replicate matrices, log_predictive,
    predict_fold and replicate_check under a row mask, and the generated chains block."""
    draws = [thetas(c, n, seed=40 + i) for i, n in enumerate(HOOK_LENGTHS)]
    ch = wa.MarkovChains.from_host(draws, lib_path=lib)
    mask = hook_mask(c["N"])
    e = engine(lib, c, 1, geometry, fma, model=model, weights=None)
    out = dict(draws=draws, mask=mask)
    out["ll"] = [e.log_lik(d) for d in draws]
    out["pred"] = [e.predict(d) for d in draws]
    out["rep"] = [e.replicate(d, SEED) for d in draws]
    out["lpd"] = e.log_predictive(ch, mask)
    out["fold"] = e.predict_fold(ch, mask)
    gen = e.replicate_chains(ch, SEED)
    out["gen"] = download(gen, max(HOOK_LENGTHS), HOOK_LENGTHS)
    gen.close()
    out["check"] = e.replicate_check(ch, SEED, mask)
    e.close()
    ch.close()
    return out


hook_arrays, same = scale_sim.hook_arrays, scale_sim.same


# ---- values ---------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(3600)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("terms", [False, True], ids=["plain", "terms"])
def test_logp_grad_against_high_precision(sim, shape, terms, record_property):
    """Both arithmetic modes, on every emulated geometry that holds the shape (its own first), against the float64
    restatement (1e-12 of the absolute version) and the high-precision one (error / bound <= 1); a row moved to another
    group is far outside the bound."""
    P, J, Q, N, own = shape
    c = make_case(P, J, Q, N, seed=P + J + Q + N, terms=terms)
    D = c["D"]
    theta = thetas(c, 3, seed=9)
    theta[2, D - 1 - Q:] = np.where(np.arange(Q + 1) % 2 == 0, 3.0, -3.0)  # tau_q, scale = 20 and 0.05 in turn
    lp64, g64 = numpy_logp_grad(c, theta)
    lp_ref, g_ref, lpa, ga = hss.reference(c["x"], c["y"], c["mp"], theta, Q, c["offset"], c["weights"], c["group"])
    moved_ref = None
    if J >= 2 and (c["weights"] is None or c["weights"][0] != 0):
        gm = c["group"].copy()
        gm[0] = (gm[0] + 1) % J
        moved_ref = hss.reference(c["x"], c["y"], c["mp"], theta, Q, c["offset"], c["weights"], gm)
    worst = 0.0
    for geometry in SIM_GEOMETRIES:
        epl = geometry[1]
        if epl < own[1]:
            continue
        blp, bg = hss.bound(lpa, ga, N, Q, epl, terms)
        for fma in (0, 1):
            e = engine(sim, c, 3, geometry, fma)
            assert e.lanes == 64 and e.dim_padded == 64 * epl
            before = e.positions()
            lp, g = e.logp_grad(theta)
            assert np.array_equal(e.positions(), before), "logp_grad must leave the chains' state alone"
            e.close()
            assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
            assert np.all(np.abs(lp - lp64) <= 1e-12 * lpa)
            for ch in range(3):
                assert np.linalg.norm(g[ch] - g64[ch]) <= 1e-12 * np.linalg.norm(ga[ch])
            ratio = hss.error_ratio(lp, g, (lp_ref, g_ref, blp, bg))
            print(f"shape {shape} geometry {geometry} terms {terms} fma {fma}: error / bound = {ratio:.3f}")
            assert ratio <= 1.0, (shape, geometry, fma, ratio)
            worst = max(worst, ratio)
            if moved_ref is not None:
                mb = hss.bound(moved_ref[2], moved_ref[3], N, Q, epl, terms)
                assert hss.error_ratio(lp, g, (moved_ref[0], moved_ref[1]) + mb) >= 100.0, shape
    record_property("max_error_over_bound", worst)


@pytest.mark.timeout(1800)
def test_finite_differences_of_every_coordinate_class(sim):
    """beta, u_q for q = 0 and the last q, s_0, s_{Q-1}, s"""
    P, J, Q, N = 3, 4, 3, 37
    c = make_case(P, J, Q, N, seed=3, terms=True)
    D = c["D"]
    e = engine(sim, c, 3)
    theta = thetas(c, 3, seed=1)
    lp, g = e.logp_grad(theta)
    h = 1e-5
    for i in (1, P + 2, P + (Q - 1) * J + 1, D - 1 - Q, D - 2, D - 1):
        plus, minus = theta.copy(), theta.copy()
        plus[:, i] += h
        minus[:, i] -= h
        fd = (e.logp_grad(plus)[0] - e.logp_grad(minus)[0]) / (2 * h)
        assert np.all(np.abs(fd - g[:, i]) <= 1e-6 * (1.0 + np.abs(lp))), (i, fd, g[:, i])
        assert np.all(g[:, i] != 0), i
    e.close()


# ---- the two anchors ------------------------------------------------------------------------------------------------
@pytest.mark.timeout(3600)
@pytest.mark.parametrize("geometry", SIM_GEOMETRIES, ids=lambda g: f"nw{g[0]}_epl{g[1]}")
@pytest.mark.parametrize("fma", [0, 1])
def test_one_varying_coefficient_is_hier_linear_regression_sigma_bit_for_bit(sim, geometry, fma):
    """varying=1: logp_grad and six warmup and six sampling transitions of four chains (positions, depths, gradient
    counts, check()) give the bits of MODEL_HIER_LINEAR_REGRESSION_SIGMA, with and without row terms."""
    epl = geometry[1]
    P, J = {2: (3, 6), 4: (130, 7), 8: (200, 150), 16: (200, 40)}[epl]
    N = 2 * hp.block_rows(epl) + 3
    for terms in (False, True):
        c = make_case(P, J, 1, N, seed=40 + epl, terms=terms)
        assert c["D"] == P + J + 2
        a, b = run(sim, c, 4, geometry, fma, model=MODEL), run(sim, c, 4, geometry, fma, model=HSIG)
        assert len(a) == 9
        for key in a:
            assert np.array_equal(a[key], b[key], equal_nan=True), (terms, key)
        assert np.all(a["grads"] > 0)


@pytest.mark.timeout(1800)
def test_one_varying_coefficient_gives_the_sibling_hooks_bit_for_bit(sim):
    """the hook matrices and folds at varying=1"""
    P, J, N, geometry = 3, 6, 70, (1, 2)
    c = hook_case(P, J, 1, N, seed=8)
    for fma in (0, 1):
        assert same(hook_arrays(hooks(sim, c, geometry, fma)), hook_arrays(hooks(sim, c, geometry, fma, model=HSIG))), fma


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("terms", [False, True], ids=["plain", "terms"])
def test_unit_noise_is_the_fixed_noise_sibling(sim, terms):
    """At s = 0 the model equals hier_linear_regression_slopes on the same data and theta without its last coordinate:
    logp minus the prior on s (-1 / (2 sigma_0^2); the likelihood's -N * 0 vanishes) and every shared gradient coordinate,
    with test_hier_scale_sim.test_unit_noise_is_the_fixed_noise_sibling's comparison and tolerance.  BIT-IDENTICAL at
    s = 0: scale = dexp(0) = 1 and 1 / (1 * 1) = 1 exactly, so every residual d * 1, every row term mad(-0.5 d, r, ll)
    - 0 and with them every shared gradient coordinate (asserted); logp is not, since the prior term of s enters one
    lane's partial before the lanes are summed."""
    P, J, Q, N = 4, 7, 3, 45
    c = make_case(P, J, Q, N, seed=13, terms=terms)   # (both references remove the rows of weight 0 first)
    D = c["D"]
    theta = thetas(c, 3, seed=4)
    theta[:, D - 1] = 0.0
    e = engine(sim, c, 3)
    epl = e.dim_padded // 64
    lp, g = e.logp_grad(theta)
    e.close()
    cs = dict(c, mp=c["mp"][:D - 1], D=D - 1)
    sib = engine(sim, cs, 3, model=SLIN)
    assert sib.dim_padded // 64 == epl
    lps, gs = sib.logp_grad(theta[:, :D - 1])
    sib.close()
    ref = hss.case(c["x"], c["y"], c["mp"], theta, Q, epl, c["offset"], c["weights"], c["group"])
    ref_s = slopes_sim.slopes_case(SLIN, cs, theta[:, :D - 1], epl)
    prior_s = -1.0 / (2 * c["mp"][D - 1] ** 2)
    assert np.all(np.abs((lp - prior_s) - lps) <= ref[2] + ref_s[2] + 2 * hp.U * np.abs(lp))
    assert np.all(np.abs(g[:, :D - 1] - gs) <= ref[3][:, :D - 1] + ref_s[3])
    assert np.array_equal(g[:, :D - 1], gs)
    assert np.linalg.norm(g[:, :D - 1]) > 0


@pytest.mark.timeout(1800)
def test_likelihood_equals_the_dense_workaround(sim):
    """The likelihood part equals the flat linear_regression_sigma's on x widened with the Q J indicator-times-covariate
    columns, at theta_flat = [beta | tau_q u_q | s] (test_hier_scale_sim.test_likelihood_equals_the_one_hot_workaround's
    construction and bound): the grouped logp minus its priors against the flat logp minus its own."""
    import hp_count_reference as hc
    P, J, Q, N = 5, 6, 3, 45
    c = make_case(P, J, Q, N, seed=5)
    D, F = c["D"], P + Q * J
    theta = thetas(c, 3, seed=3, scale=0.4)
    e = engine(sim, c, 3)
    epl = e.dim_padded // 64
    lp, _ = e.logp_grad(theta)
    e.close()
    beta, u, sq, s = theta[:, :P], theta[:, P:F].reshape(3, Q, J), theta[:, D - 1 - Q:D - 1], theta[:, D - 1]
    tau = np.exp(sq)
    mp = c["mp"]
    own = [-(beta * beta / (2 * mp[:P])).sum(1), -(u * u).sum((1, 2)) / 2,
           (sq - tau * tau / (2 * mp[D - 1 - Q:D - 1] ** 2)).sum(1), s - np.exp(2 * s) / (2 * mp[D - 1] ** 2)]
    ll = lp - sum(own)
    z = np.concatenate([np.ones((N, 1)), c["x"][:, :Q - 1]], axis=1)
    xw = np.concatenate([c["x"]] + [np.eye(J)[c["group"]] * z[:, q:q + 1] for q in range(Q)], axis=1)
    s2 = np.concatenate([mp[:P], np.ones(Q * J), [mp[D - 1]]])
    tf = np.concatenate([beta, (tau[:, :, None] * u).reshape(3, Q * J), s[:, None]], axis=1)
    f = wa.DeviceEngine(wa.MODEL_LINEAR_REGRESSION_SIGMA, F + 1, 3, config(sim), params=s2, lib_path=sim, data=(xw, c["y"]))
    epl_flat = f.dim_padded // 64
    lpf, _ = f.logp_grad(tf)
    f.close()
    flat_priors = [-(tf[:, :F] ** 2 / (2 * s2[:F])).sum(1), s - np.exp(2 * s) / (2 * mp[D - 1] ** 2)]
    llf = lpf - sum(flat_priors)
    _, _, lpa, ga = hss.reference(c["x"], c["y"], mp, theta, Q, None, None, c["group"])
    bound = hss.bound(lpa, ga, N, Q, epl, False)[0] + hc.count_bound(lpa, ga[:, :F + 1], N, epl_flat)[0]
    bound = bound + 8 * hp.U * (np.abs(lp) + np.abs(lpf) + sum(np.abs(a) for a in own + flat_priors))
    print("dense workaround error / bound", np.abs(ll - llf) / bound)
    assert np.all(np.abs(ll - llf) <= bound), np.abs(ll - llf) / bound
    assert np.all(np.abs(ll) > 1.0)


# ---- hooks ----------------------------------------------------------------------------------------------------------
HOOK_SHAPES = [SHAPES[i] for i in (1, 3, 4, 5, 6)]
HOOK_SHAPE_IDS = [SHAPE_IDS[i] for i in (1, 3, 4, 5, 6)]


@pytest.mark.timeout(3600)
@pytest.mark.parametrize("shape", HOOK_SHAPES, ids=HOOK_SHAPE_IDS)
def test_hooks(sim, shape, record_property):
    """log_lik against the pointwise reference, predict against the predict reference (v = exp(2 s)), replicate against
    the sampler probe fed predict()'s mu and the device's scale (fmad(scale, z, mu)); the folds (log_predictive,
    predict_fold, replicate_check) with a masked row and a live row whose offset is non-zero against the references' folds
    and the Python-float replays."""
    import hp_replicate_reference as hr
    P, J, Q, N, geometry = shape
    epl = geometry[1]
    c = hook_case(P, J, Q, N, seed=11 + P)
    lib = _ffi.load_library(sim)
    worst = 0.0
    for fma in (0, 1):
        h = hooks(sim, c, geometry, fma)
        mask = h["mask"]
        assert not mask[1] and mask[0] and c["offset"][0] != 0
        L_rows, b_rows = [], []
        for ci, (theta, ll, (eta, mu, v), rep, gen) in enumerate(zip(h["draws"], h["ll"], h["pred"], h["rep"], h["gen"])):
            ref_ll = hss.pointwise_reference(c["x"], c["y"], theta, Q, epl, c["offset"], c["group"])
            ref_pr = hss.predict_reference(c["x"], theta, Q, epl, c["offset"], c["group"])
            ratios = hpw.error_ratio(ll, ref_ll), hpp.error_ratio((eta, mu, v), ref_pr)
            print(f"shape {shape} fma {fma} chain {ci}: error / bound = {ratios[0]:.3f} (log_lik), {ratios[1]:.3f} (eta, mu, v)")
            assert max(ratios) <= 1.0, (fma, ci, ratios)
            worst = max(worst, *ratios)
            assert np.array_equal(mu, eta)
            assert np.allclose(v, np.exp(2 * theta[:, -1])[:, None] * np.ones(N), rtol=1e-14, atol=0)
            # the offset dropped, the constant omitted, the neighbouring group's effects: far outside the bounds
            no_off = hss.pointwise_reference(c["x"], c["y"], theta, Q, epl, None, c["group"])["ll"]
            no_const = hss.pointwise_reference(c["x"], c["y"], theta, Q, epl, c["offset"], c["group"], constant=False)["ll"]
            assert (np.abs(no_off - ref_ll["ll"]) / ref_ll["bound"]).max() > 10.0
            assert (np.abs(no_const - ref_ll["ll"]) / ref_ll["bound"]).max() > 10.0
            other = hss.predict_reference(c["x"], theta, Q, epl, c["offset"], (c["group"] + 1) % J)
            assert (np.abs(other["eta"] - ref_pr["eta"]) / ref_pr["eta_bound"]).max() > 10.0
            L_rows += ref_ll["L"]
            b_rows.append(ref_ll["bound"])
            for t in range(len(theta)):
                s = theta[t, c["D"] - 1]
                assert hm.same_bits(rep[t], hss.replicate_probe(lib, mu[t], s, SEED, t, 0)), (ci, t)
                assert hm.same_bits(gen[t], hss.replicate_probe(lib, mu[t], s, SEED, ci, t)), (ci, t)
            assert not np.isnan(rep).any() and not np.isnan(gen).any()
        # the folds: masked rows are not evaluated; live rows against the exact fold and the replays
        T = sum(HOOK_LENGTHS)
        lpd, mean, var, count = h["lpd"]
        assert np.all(count[~mask] == 0) and np.all(np.isnan(lpd[~mask])) and np.all(count[mask] == T)
        fold = hpw.fold(L_rows, np.concatenate(b_rows), len(HOOK_LENGTHS))
        for name, got in (("lpd", lpd), ("mean", mean), ("var", var)):
            assert np.all(np.abs(got[mask] - fold[name][mask]) <= fold[name + "_bound"][mask]), name
        want = hpp.replay_fold([p[0] for p in h["pred"]], [p[1] for p in h["pred"]], [p[2] for p in h["pred"]])
        for got, exp in zip(h["fold"], want):
            assert np.array_equal(np.asarray(got)[mask], np.asarray(exp)[mask], equal_nan=True)
        assert np.all(h["fold"][5][~mask] == 0) and np.all(np.isnan(h["fold"][0][~mask]))
        stat_rep, stat_obs = h["check"]
        for ci, n in enumerate(HOOK_LENGTHS):
            eta, mu, v = h["pred"][ci]
            for i in range(n):
                assert hm.same_bits(stat_rep[:, ci, i], hr.check_statistics(h["gen"][ci][i], mu[i], v[i], mask))
                assert hm.same_bits(stat_obs[:, ci, i], hr.check_statistics(c["y"], mu[i], v[i], mask))
            assert np.all(np.isnan(stat_rep[:, ci, n:]))
    record_property("max_error_over_bound", worst)


@pytest.mark.timeout(1800)
def test_hooks_invariance_and_psis(sim, monkeypatch):
    """Another grid: identical bits everywhere.  Another row order: the per-row outputs permute, bit for bit.  A row mask:
    the other rows keep their bits.  psis_loo: finite, and its matrix is the emulation's own log_lik columns."""
    P, J, Q, N, geometry = SHAPES[1]
    c = hook_case(P, J, Q, N, seed=8)
    base = hooks(sim, c, geometry, 1)
    monkeypatch.setenv("WALNUTS_AMD_POINTWISE_GRID", "1")
    other = hooks(sim, c, geometry, 1)
    monkeypatch.delenv("WALNUTS_AMD_POINTWISE_GRID")
    assert same(hook_arrays(base), hook_arrays(other))
    perm = np.random.default_rng(4).permutation(N)
    cp = dict(c, x=c["x"][perm], y=c["y"][perm], group=c["group"][perm], offset=c["offset"][perm])
    e = engine(sim, cp, 1, geometry, 1, weights=None)
    for d, ll, (eta, mu, v) in zip(base["draws"], base["ll"], base["pred"]):
        assert np.array_equal(e.log_lik(d), ll[:, perm])
        assert same(e.predict(d), (eta[:, perm], mu[:, perm], v[:, perm]))
    e.close()
    mask = base["mask"]
    ch = wa.MarkovChains.from_host(base["draws"], lib_path=sim)
    # y and the weights are never read by predict and replicate
    e = engine(sim, dict(c, y=np.zeros(N)), 1, geometry, 1, weights=np.full(N, 7.0))
    assert same([e.replicate(d, SEED) for d in base["draws"]], base["rep"])
    assert same([a for d in base["draws"] for a in e.predict(d)], [a for m in base["pred"] for a in m])
    e.close()
    e = engine(sim, c, 1, geometry, 1, weights=None)
    full = e.log_predictive(ch)
    assert all(np.array_equal(a[mask], b[mask]) for a, b in zip(full, base["lpd"]))
    ch.close()
    S = 16
    draws = [thetas(c, S, seed=70 + i, scale=0.1) for i in range(2)]
    ch = wa.MarkovChains.from_host(draws, lib_path=sim)
    elpd, k, ess, lpd, count = e.psis_loo(ch)
    assert np.all(np.isfinite(elpd)) and np.all(np.isfinite(lpd)) and np.all(np.isfinite(ess)) and np.all(count == 2 * S)
    assert not np.isnan(k).any() and np.all(elpd <= lpd + 1e-9 * np.abs(lpd))
    matrix = e._psis_matrix(ch, 2 * S)
    assert matrix.shape == (N, 2 * S) and np.array_equal(matrix.T, e.log_lik(np.concatenate(draws)))
    e.close()
    ch.close()


# ---- runs -----------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(3600)
@pytest.mark.parametrize("geometry", [(1, 2), (1, 8)], ids=["nw1_epl2", "nw1_epl8"])
def test_datasets_and_weight_sets_equal_standalone_engines(sim, geometry):
    """datasets= with three grouped datasets of sizes [1, B + 1, 2 B + 3] equals three stand-alone engines bit for bit;
    the same for weight_sets= with W = 3."""
    epl = geometry[1]
    P, J, Q = {2: (3, 4, 2), 8: (130, 70, 3)}[epl]
    B, k = hp.block_rows(epl), 2
    cases = [make_case(P, J, Q, n, seed=60 + 7 * i) for i, n in enumerate((1, B + 1, 2 * B + 3))]
    mp, D = cases[0]["mp"], cases[0]["D"]
    cfg = config(sim, geometry, 1)
    kw = dict(params=mp, lib_path=sim, varying=Q)
    e = wa.DeviceEngine(MODEL, D, 3 * k, cfg, datasets=[data_of(c) for c in cases], **kw)
    assert e.num_datasets == 3 and e.dim_padded == 64 * epl
    batched = drive(e, 0)
    e.close()
    for gi, c in enumerate(cases):
        alone = wa.DeviceEngine(MODEL, D, k, cfg, data=data_of(c), **kw)
        compare_blocks(batched, drive(alone, gi * k), gi, k)
        alone.close()
    c = cases[2]
    sets = np.random.default_rng(2).integers(0, 3, size=(3, c["N"])).astype(np.float64)
    e = wa.DeviceEngine(MODEL, D, 3 * k, cfg, data=data_of(c), weight_sets=sets, **kw)
    assert e.num_datasets == 3
    batched = drive(e, 0)
    e.close()
    for gi in range(3):
        alone = wa.DeviceEngine(MODEL, D, k, cfg, data=data_of(c), weights=sets[gi], **kw)
        compare_blocks(batched, drive(alone, gi * k), gi, k)
        alone.close()


@pytest.mark.timeout(1800)
def test_non_finite_scales(sim):
    """Chains placed at s = +-800 or s_q = +-800 (q = 0 and the last): IEEE results, the other chains stay finite, check()
    is clean."""
    c = make_case(4, 3, 3, 30, seed=4)
    D, Q = c["D"], c["Q"]
    e = engine(sim, c, 8, (1, 2), 1)
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
    assert np.all(np.isfinite(e.positions()[6:])) and np.all(np.isfinite(e.logp()[6:]))
    e.close()


@pytest.mark.timeout(1800)
def test_drop_in_calls_and_wrappers(sim):
    """walnuts_device with data=(x, y, group), varying=2, offset=, weights= and with datasets=; host draws equal
    kept-on-device draws; the scoring, predicting and replicating wrappers take the fit: none needed new code."""
    c = make_case(3, 4, 2, 25, seed=2, terms=True)
    c["offset"][24] = 0.1
    D = c["D"]
    kw = dict(model_params=c["mp"], num_params=D, num_chains=2, seed=9, min_warmup_iter=5, max_warmup_iter=5,
              min_sampling_iter=4, max_sampling_iter=4, lib_path=sim, varying=2)
    rows = dict(data=data_of(c), offset=c["offset"])
    host = wa.walnuts_device(MODEL, weights=c["weights"], **rows, **kw)
    kept, chains = wa.walnuts_device(MODEL, weights=c["weights"], keep_on_device=True, thin=1, **rows, **kw)
    for a, b in zip(host, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.all(np.isfinite(np.asarray(a)))
    common = dict(num_params=D, lib_path=sim, varying=2, **rows)
    res = wa.log_predictive(MODEL, chains, **common)
    assert res.lpd.shape == (25,) and np.all(np.isfinite(res.lpd))
    loo = wa.psis_loo(MODEL, chains, **common)
    assert np.all(np.isfinite(loo.lpd))
    new = (c["x"][:7], c["group"][:7])
    pr = wa.predict(MODEL, chains, num_params=D, data=new, offset=c["offset"][:7], lib_path=sim, varying=2)
    assert pr.mean.shape == (7,) and np.all(np.isfinite(pr.mean)) and np.all(pr.noise_var > 0)   # sigma^2, estimated
    ppc = wa.posterior_predictive_check(MODEL, chains, seed=3, **common)
    assert np.all((ppc.p_value["mean"] >= 0) & (ppc.p_value["mean"] <= 1))
    chains.close()
    sets = [data_of(make_case(3, 4, 2, n, seed=3 + n)) for n in (25, 9, 14)]
    kw["num_chains"] = 6
    many = wa.walnuts_device(MODEL, datasets=sets, **kw)
    kept, views = wa.walnuts_device(MODEL, datasets=sets, keep_on_device=True, thin=1, **kw)
    assert len(many) == 6 and len(views) == 3
    for a, b in zip(many, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for v in views:
        v.close()


def test_exact_posterior_quadrature_has_converged():
    """The reference of test_hier_slopes_scale_gpu.test_against_exact_posterior: halving the grid's step moves nothing at
    the tolerance (asserted inside), and halving it once more moves nothing either."""
    x, y, group, mp, P, J, Q = hss.exact_case()
    assert (P, J, Q, len(y)) == (2, 4, 2, 40) and np.bincount(group, minlength=J).min() >= 4
    mean, var = hss.exact_posterior(x, y, group, mp, J)
    mean3, var3, edge = hss.exact_moments(x, y, group, mp, J, 0.03125)
    assert edge <= 1e-12
    assert np.all(np.abs(mean3 - mean) <= 1e-6 * np.sqrt(var)) and np.all(np.abs(var3 - var) <= 1e-6 * var)
    assert 0.3 < mean[P + Q * J + 2] < 1.5 and np.all(var > 0)   # sigma, simulated at 0.7


# ---- refusals and front-end results ---------------------------------------------------------------------------------
c_abi_error = slopes_sim.c_abi_error


@pytest.mark.timeout(900)
def test_refusals(sim):
    lib = _ffi.load_library(sim)
    N = 6
    y, g = np.zeros(N), np.zeros(N, dtype=np.int32)
    cfg = wa.default_config(sim)

    def py(D, P, Q, match, group=g, model=MODEL, mp=None):
        with pytest.raises(ValueError, match=match):
            wa.DeviceEngine(model, D, 2, cfg, params=np.ones(D) if mp is None else mp, lib_path=sim,
                            data=(np.zeros((N, P)), y) if group is None else (np.zeros((N, P)), y, group), varying=Q)

    # Q = 0, Q = 9
    py(6, 3, 0, "varying must be at least 1")
    assert "1 <= num_varying <= 8, got -1" in c_abi_error(sim, MODEL, 6, np.zeros((N, 3)), y, g, 1, -1)
    assert "1 <= num_varying <= 8, got 9" in c_abi_error(sim, MODEL, 9 + 9 * 2 + 1, np.zeros((N, 9)), y, g, 1, 9)
    py(9 + 9 * 2 + 1, 9, 9, "1 <= num_varying <= 8, got 9")
    # Q - 1 > P
    assert "num_varying - 1 <= P, got num_varying 3, P 1" in c_abi_error(sim, MODEL, 1 + 3 * 2 + 1, np.zeros((N, 1)), y, g, 1, 3)
    py(8, 1, 3, "num_varying - 1 <= P, got num_varying 3, P 1")
    # P < 1, J < 1: the identity is named with its + 1
    msg = r"num_params == P \+ num_varying \* \(num_groups \+ 1\) \+ 1 with P >= 1 and num_groups >= 1"
    assert "(num_groups + 1) + 1 with" in c_abi_error(sim, MODEL, 5, np.zeros((N, 1)), y, g, 1, 2)
    assert "got num_params 5, num_groups 1, num_varying 2" in c_abi_error(sim, MODEL, 5, np.zeros((N, 1)), y, g, 1, 2)  # P = 0
    assert "got num_params 7, num_groups 0, num_varying 2" in c_abi_error(sim, MODEL, 7, np.zeros((N, 4)), y, g, 0, 2)  # J = 0
    py(7, 4, 2, msg)   # J = 0
    py(5, 4, 2, msg)   # J = -1
    # a remainder in (D - P - 1) / Q
    py(8, 2, 2, r"num_params - P - 1 must be a multiple of varying \(num_params == P \+ varying \* \(J \+ 1\) \+ 1\), "
                "got num_params 8, P 2, varying 2")
    # a pair (x, y) without groups: the message names this model's column count
    pair = NAME + r" model reads a group per observation: .*x \[num_obs\]\[num_params - num_varying \* \(num_groups \+ 1\) - 1\]"
    py(8, 8, 2, pair, group=None)
    # varying=2 on id 35 is still refused
    py(8, 3, 2, "has no varying slopes", model=HSIG)
    assert "has no varying slopes" in c_abi_error(sim, HSIG, 8, np.zeros((N, 3)), y, g, 1, 2)
    # sigma_q and sigma_0
    for i in (5, 6, 7):
        for bad in (0.0, -1.0, np.inf):
            py(8, 3, 2, "sigma_q, sigma_0.* must be positive and finite", mp=np.where(np.arange(8) == i, bad, 1.0))
    bad = np.ones(8)
    bad[7] = -1.0
    assert "positive and finite" in c_abi_error(sim, MODEL, 8, np.zeros((N, 3)), y, g, 1, 2, mp=bad)
    # one wavefront per chain; groups in range
    py(1101, 1000, 2, "num_params <= 1024")
    py(8, 3, 2, r"every group must be in \[0, num_groups\)", group=g + 1)
    # what is accepted
    assert c_abi_error(sim, MODEL, 8, np.zeros((N, 3)), y, g, 1, 2) == ""
    assert c_abi_error(sim, MODEL, 6, np.zeros((N, 3)), y, g, 1, 0) == ""   # 0: the intercept alone
    assert c_abi_error(sim, MODEL, 6, np.zeros((N, 1)), y, g, 1, 2) == ""
    assert c_abi_error(sim, MODEL, 1024, np.zeros((N, 1)), y, g, 510, 2) == ""
    assert lib.wn_model_data_columns_varying(MODEL, 8, 1, 3) == -1 and lib.wn_model_data_columns_varying(MODEL, 5, 1, 2) == -1


def test_front_end_results(sim):
    lib = _ffi.load_library(sim)
    assert lib.wn_model_num_scale_params(MODEL) == 1
    assert lib.wn_model_data_columns(MODEL, 20, 5) == 13
    assert lib.wn_model_data_columns(MODEL, 20, 0) == -1
    assert lib.wn_model_data_columns_varying(MODEL, 20, 5, 1) == 13
    assert lib.wn_model_data_columns_varying(MODEL, 20, 5, 0) == 13
    assert lib.wn_model_data_columns_varying(MODEL, 21, 4, 2) == 10
    assert lib.wn_model_data_columns_varying(MODEL, 20, 5, 9) == -1
    assert wa.model_id(NAME, sim) == MODEL == 40
    # the siblings' answers stand
    assert lib.wn_model_data_columns_varying(SLIN, 20, 4, 2) == 10 and lib.wn_model_data_columns_varying(HSIG, 20, 5, 2) == -1
    for free in (37, 38, 39):
        assert lib.wn_model_num_scale_params(free) == -1
