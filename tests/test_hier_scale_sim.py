"""CPU tier: hierarchical linear regression with an estimated noise level (walnuts_amd/csrc/models/hier_scale_glm.h;
kScaleParam on top of the group channel) under the workgroup emulation.

References: tests/helpers/hp_hier_scale_reference.py (np.longdouble accumulation, mpmath for exp, an error bound per
chain of the form K * u * the absolute version of the computation, with the constants of hp_reference.glm_bound, K_TAU
and C_COUNT, none grown), a float64 NumPy restatement, central finite differences, the
identities with the siblings (centered = non-centered up to the Jacobian; the flat scale models on one-hot columns; the
fixed-noise hier_linear_regression* at s = 0), the pointwise / predict / replicate hooks against the hp_* references and
the sampler probe, datasets and weight sets against stand-alone engines, the refusals by their messages, the front-end
queries, and a short run.  The device side of the same kernel source is compared bit for bit in test_hier_scale_gpu.py.

The worst error / bound over this file's references is printed per test and recorded in DESIGN.md 3.8.10."""
import ctypes as C
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
import hp_math_reference as hm  # noqa: E402
import hp_pointwise_reference as hpw  # noqa: E402
import hp_predict_reference as hpp  # noqa: E402
import hp_reference as hp  # noqa: E402
import hp_weighted_reference as hw  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from walnuts_amd import _ffi  # noqa: E402
from test_datasets_sim import compare_blocks, drive  # noqa: E402
from test_predict_sim import download  # noqa: E402

HSIG, HSIG_C = wa.MODEL_HIER_LINEAR_REGRESSION_SIGMA, wa.MODEL_HIER_LINEAR_REGRESSION_SIGMA_CENTERED
MODELS = (HSIG, HSIG_C)
IDS = ["linear_sigma", "linear_sigma_c"]
assert MODELS == hs.MODELS
CENTERED = (HSIG_C,)
FLAT = {HSIG: wa.MODEL_LINEAR_REGRESSION_SIGMA, HSIG_C: wa.MODEL_LINEAR_REGRESSION_SIGMA}
FIXED_NOISE = {HSIG: wa.MODEL_HIER_LINEAR_REGRESSION, HSIG_C: wa.MODEL_HIER_LINEAR_REGRESSION_CENTERED}
SIM_GEOMETRIES = ((1, 2), (1, 4), (1, 8), (1, 16))
# (P, J, N, geometry): D = 4, everything in lanes 0 and 1; N no multiple of B = 16, more than four blocks; D = 129, s_tau
# at coordinate 127 (lane 63, second slot), s at 128 (lane 0 of the next slot pair), the effects across the pair boundary;
# rows narrower than theta, nx = 2, N = B + 1; the same at eight per lane; D = 512, s in the very last slot; sixteen per
# lane; D = 1024, the limit; N = 1 with five groups that no row belongs to
SHAPES = [(1, 1, 3, (1, 2)), (3, 6, 70, (1, 2)), (3, 124, 9, (1, 4)), (130, 20, 9, (1, 4)), (200, 150, 50, (1, 8)),
          (300, 210, 13, (1, 8)), (129, 500, 61, (1, 16)), (1, 1021, 5, (1, 16)), (3, 6, 1, (1, 2))]
SHAPE_IDS = ["P1J1N3", "P3J6N70", "P3J124N9", "P130J20N9", "P200J150N50", "P300J210N13", "P129J500N61", "P1J1021N5",
             "P3J6N1"]
SEED = 2 ** 33 + 5


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def make_case(model, P, J, N, seed, terms=False):
    """dict(x [N, P], y [N], group [N] (row 0 in group J - 1; with J > 2 some groups stay empty when N is small), mp [D],
    offset, weights).  terms: per-row offsets and weights; the weights hold zeros, and row N - 1 has weight 0 and an
    offset (1e308) at which the family's term is not finite."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    group = rng.integers(0, J, size=N).astype(np.int32)
    group[0] = J - 1
    eta = x @ rng.normal(size=P) + 0.7 * rng.normal(size=J)[group]
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
    mp = np.concatenate([rng.uniform(0.5, 4.0, size=P), np.ones(J), rng.uniform(0.8, 2.0, size=2)])
    return dict(x=x, y=y, group=group, mp=mp, offset=offset, weights=weights, P=P, J=J, N=N, D=P + J + 2)


def data_of(c):
    return (c["x"], c["y"], c["group"])


def thetas(c, T, seed, scale=0.3):
    rng = np.random.default_rng(seed)
    th = scale * rng.normal(size=(T, c["D"]))
    th[:, c["D"] - 2:] = rng.uniform(-0.8, 1.1, size=(T, 2))
    return th


def numpy_logp_grad(model, c, theta):
    """float64 NumPy restatement (rows of weight 0 removed first)."""
    w = c["weights"]
    keep = np.arange(c["N"]) if w is None else np.flatnonzero(w != 0)
    X, Y, group = c["x"][keep], c["y"][keep], c["group"][keep]
    W = np.ones(len(keep)) if w is None else w[keep]
    O = np.zeros(len(keep)) if c["offset"] is None else c["offset"][keep]
    P, J, D, MP = c["P"], c["J"], c["D"], c["mp"]
    TH = np.atleast_2d(theta)
    beta, u, st, s = TH[:, :P], TH[:, P:P + J], TH[:, D - 2], TH[:, D - 1]
    tau = np.exp(st)
    v = u if model in CENTERED else tau[:, None] * u
    eta = beta @ X.T + v[:, group] + O
    isig2 = np.exp(-2 * s)[:, None]
    d = Y - eta
    r = d * isig2
    ll = -0.5 * d * d * isig2 - s[:, None]
    ds = d * d * isig2 - 1
    rw = W * r
    S = rw @ np.eye(J)[group].reshape(len(keep), J)
    tt = tau * tau / MP[D - 2] ** 2
    ss = np.exp(2 * s) / MP[D - 1] ** 2
    lp = (W * ll).sum(1) - (beta * beta / (2 * MP[:P])).sum(1) + (st - tt / 2) + (s - ss / 2)
    g = np.zeros_like(TH)
    g[:, :P] = rw @ X - beta / MP[:P]
    if model in CENTERED:
        q = (u * u).sum(1) / (tau * tau)
        lp += -J * st - q / 2
        g[:, P:P + J] = S - u / (tau * tau)[:, None]
        g[:, D - 2] = -J + q + 1 - tt
    else:
        lp += -(u * u).sum(1) / 2
        g[:, P:P + J] = tau[:, None] * S - u
        g[:, D - 2] = tau * (u * S).sum(1) + 1 - tt
    g[:, D - 1] = (W * ds).sum(1) + 1 - ss
    return lp, g


def hs_case(model, c, theta, epl):
    return hs.case(model, c["x"], c["y"], c["mp"], theta, epl, c["offset"], c["weights"], c["group"])


def config(lib, geometry=None, fma=1):
    """(trees of at most 3 doublings and steps halved at most twice: the model's code is the same at every depth, and
    the emulation's time goes with the number of gradient evaluations)"""
    nw, epl = geometry if geometry else (0, 0)
    return wa.default_config(lib, fused_multiply_add=fma, waves_per_chain=nw, elems_per_lane=epl, max_trajectory_doublings=3,
                             max_step_halvings=2)


def engine(lib, model, c, num_chains, geometry=None, fma=1, **kw):
    kw.setdefault("offset", c["offset"])
    kw.setdefault("weights", c["weights"])
    if "datasets" not in kw and "data" not in kw:
        kw["data"] = data_of(c)
    return wa.DeviceEngine(model, c["D"], num_chains, config(lib, geometry, fma), params=c["mp"], lib_path=lib, **kw)


def run(lib, model, c, num_chains, geometry, fma, warm=6, samp=6):
    """logp_grad at fixed positions, then warmup and sampling transitions: everything the device must reproduce (the nine
    arrays of test_hier_models_gpu.run)"""
    e = engine(lib, model, c, num_chains, geometry, fma)
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


HOOK_LENGTHS = (3, 2)


def hook_case(model, P, J, N, seed):
    """a case for the hooks: offsets everywhere (the last row's non-zero and finite), no weights applied"""
    c = make_case(model, P, J, N, seed=seed, terms=True)
    c["offset"][N - 1] = 0.25
    return c


def hook_mask(N):
    """rows n % 3 == 1 masked; row N - 1, whose offset is non-zero, live whenever N % 3 != 2"""
    return np.arange(N) % 3 != 1


def hooks(lib, model, c, geometry, fma):
    """The three hooks' outputs on two ragged chains: the log_lik, predict and replicate matrices, log_predictive,
    predict_fold and replicate_check under a row mask, and the generated chains block."""
    draws = [thetas(c, n, seed=40 + i) for i, n in enumerate(HOOK_LENGTHS)]
    ch = wa.MarkovChains.from_host(draws, lib_path=lib)
    mask = hook_mask(c["N"])
    e = engine(lib, model, c, 1, geometry, fma, weights=None)
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


def hook_arrays(h):
    """the arrays of hooks() as one flat list (for bitwise comparisons)"""
    flat = list(h["ll"]) + [a for m in h["pred"] for a in m] + list(h["rep"]) + list(h["lpd"]) + list(h["fold"])
    return flat + list(h["gen"]) + list(h["check"])


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


# ---- values ---------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", MODELS, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("terms", [False, True], ids=["plain", "terms"])
def test_logp_grad_against_high_precision(sim, model, shape, terms, record_property):
    """Both arithmetic modes, on every emulated geometry that holds the shape (its own first), against the float64
    restatement (1e-12 of the absolute version) and the high-precision one (error / bound <= 1); a row moved to another
    group is far outside the bound."""
    P, J, N, own = shape
    c = make_case(model, P, J, N, seed=P + J + N, terms=terms)
    D = c["D"]
    theta = thetas(c, 3, seed=9)
    theta[2, D - 2:] = (3.0, -3.0)  # tau = 20, scale = 0.05
    lp64, g64 = numpy_logp_grad(model, c, theta)
    lp_ref, g_ref, lpa, ga = hs.reference(model, c["x"], c["y"], c["mp"], theta, c["offset"], c["weights"], c["group"])
    moved_ref = None
    if J >= 2 and (c["weights"] is None or c["weights"][0] != 0):
        gm = c["group"].copy()
        gm[0] = (gm[0] + 1) % J
        moved_ref = hs.reference(model, c["x"], c["y"], c["mp"], theta, c["offset"], c["weights"], gm)
    worst = 0.0
    for geometry in SIM_GEOMETRIES:
        epl = geometry[1]
        if 64 * epl < D or (geometry != own and epl < own[1]):
            continue
        blp, bg = hs.bound(lpa, ga, N, epl, terms)
        for fma in (0, 1):
            e = engine(sim, model, c, 3, geometry, fma)
            assert e.lanes == 64 and e.dim_padded == 64 * epl
            before = e.positions()
            lp, g = e.logp_grad(theta)
            assert np.array_equal(e.positions(), before), "logp_grad must leave the chains' state alone"
            e.close()
            assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
            assert np.all(np.abs(lp - lp64) <= 1e-12 * lpa)
            for ch in range(3):
                assert np.linalg.norm(g[ch] - g64[ch]) <= 1e-12 * np.linalg.norm(ga[ch])
            ratio = hs.error_ratio(lp, g, (lp_ref, g_ref, blp, bg))
            print(f"model {model} shape {shape} geometry {geometry} terms {terms} fma {fma}: error / bound = {ratio:.3f}")
            assert ratio <= 1.0, (shape, geometry, fma, ratio)
            worst = max(worst, ratio)
            if moved_ref is not None:
                mb = hs.bound(moved_ref[2], moved_ref[3], N, epl, terms)
                assert hs.error_ratio(lp, g, (moved_ref[0], moved_ref[1]) + mb) >= 100.0, shape
    record_property("max_error_over_bound", worst)


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", MODELS, ids=IDS)
def test_finite_differences_of_every_coordinate_class(sim, model):
    P, J, N = 3, 4, 37
    c = make_case(model, P, J, N, seed=3, terms=True)
    D = c["D"]
    e = engine(sim, model, c, 3)
    theta = thetas(c, 3, seed=1)
    lp, g = e.logp_grad(theta)
    h = 1e-5
    for i in range(D):  # every beta, every effect, s_tau, s
        plus, minus = theta.copy(), theta.copy()
        plus[:, i] += h
        minus[:, i] -= h
        fd = (e.logp_grad(plus)[0] - e.logp_grad(minus)[0]) / (2 * h)
        assert np.all(np.abs(fd - g[:, i]) <= 1e-6 * (1.0 + np.abs(lp))), (i, fd, g[:, i])
    assert np.all(g[:, D - 2] != 0) and np.all(g[:, D - 1] != 0)
    e.close()


# ---- identities: each within the sum of the two sides' reference bounds ---------------------------------------------
@pytest.mark.timeout(1800)
@pytest.mark.parametrize("nc,ce", [(HSIG, HSIG_C)], ids=["linear_sigma"])
@pytest.mark.parametrize("terms", [False, True], ids=["plain", "terms"])
def test_reparameterization_identity(sim, nc, ce, terms):
    """logp_nc(beta, z, s_tau, s) == logp_c(beta, exp(s_tau) z, s_tau, s) + J s_tau.  a = fl(tau z) is not the exact
    product: the centered side's reference is evaluated at the a the engine is given, and the difference of the two exact
    values, at most u |a_j| |d logp / d a_j| per effect, is added to the bound."""
    P, J, N = 6, 9, 40
    c = make_case(nc, P, J, N, seed=21, terms=terms)
    D = c["D"]
    theta = thetas(c, 4, seed=2, scale=0.5)
    theta[:, D - 2] = (-1.0, 0.0, 0.5, 1.5)
    tc = theta.copy()
    tc[:, P:P + J] *= np.exp(theta[:, D - 2])[:, None]
    e = engine(sim, nc, c, 4)
    epl = e.dim_padded // 64
    lp_nc, _ = e.logp_grad(theta)
    e.close()
    e = engine(sim, ce, c, 4)
    lp_c, g_c = e.logp_grad(tc)
    e.close()
    b_nc = hs_case(nc, c, theta, epl)[2]
    b_c = hs_case(ce, c, tc, epl)[2]
    moved = 2 * hp.U * (np.abs(tc[:, P:P + J]) * np.abs(g_c[:, P:P + J])).sum(1)   # a = fl(tau z), tau = fl(exp(s_tau))
    jac = J * theta[:, D - 2]
    err = np.abs(lp_nc - (lp_c + jac))
    bound = b_nc + b_c + moved + 2 * hp.U * (np.abs(lp_c) + np.abs(jac))
    print("identity error / bound", err / bound)
    assert np.all(err <= bound), err / bound


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [HSIG], ids=["linear_sigma"])
def test_likelihood_equals_the_one_hot_workaround(sim, model):
    """The likelihood part equals the flat scale model's on x widened with the group indicators, at theta_flat =
    [beta | v | s] (test_hier_models_sim.test_likelihood_equals_the_one_hot_workaround's construction): the grouped logp
    minus its priors against the flat logp minus its own, within the two sides' reference bounds (the flat side:
    hp_count_reference.count_bound on the same absolute version) and the roundings of taking the priors off."""
    import hp_count_reference as hc
    P, J, N = 5, 12, 60
    c = make_case(model, P, J, N, seed=5)
    D = c["D"]
    theta = thetas(c, 3, seed=3, scale=0.4)
    e = engine(sim, model, c, 3)
    epl = e.dim_padded // 64
    lp, _ = e.logp_grad(theta)
    e.close()
    beta, z, st, s = theta[:, :P], theta[:, P:P + J], theta[:, D - 2], theta[:, D - 1]
    tau = np.exp(st)
    mp = c["mp"]
    own = [-(beta * beta / (2 * mp[:P])).sum(1), -(z * z).sum(1) / 2, st - tau * tau / (2 * mp[D - 2] ** 2),
           s - np.exp(2 * s) / (2 * mp[D - 1] ** 2)]
    ll = lp - sum(own)
    xw = np.concatenate([c["x"], np.eye(J)[c["group"]]], axis=1)
    s2 = np.concatenate([mp[:P], np.ones(J), [mp[D - 1]]])
    tf = np.concatenate([beta, tau[:, None] * z, s[:, None]], axis=1)
    f = wa.DeviceEngine(FLAT[model], P + J + 1, 3, config(sim), params=s2, lib_path=sim, data=(xw, c["y"]))
    epl_flat = f.dim_padded // 64
    lpf, _ = f.logp_grad(tf)
    f.close()
    flat_priors = [-(tf[:, :P + J] ** 2 / (2 * s2[:P + J])).sum(1), s - np.exp(2 * s) / (2 * mp[D - 1] ** 2)]
    llf = lpf - sum(flat_priors)
    _, _, lpa, ga = hs.reference(model, c["x"], c["y"], mp, theta, None, None, c["group"])
    bound = hs.bound(lpa, ga, N, epl, False)[0] + hc.count_bound(lpa, ga[:, :P + J + 1], N, epl_flat)[0]
    bound = bound + 8 * hp.U * (np.abs(lp) + np.abs(lpf) + sum(np.abs(a) for a in own + flat_priors))
    print("one-hot error / bound", np.abs(ll - llf) / bound)
    assert np.all(np.abs(ll - llf) <= bound), np.abs(ll - llf) / bound


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [HSIG, HSIG_C], ids=["noncentered", "centered"])
@pytest.mark.parametrize("terms", [False, True], ids=["plain", "terms"])
def test_unit_noise_is_the_fixed_noise_sibling(sim, model, terms):
    """At s = 0, hier_linear_regression_sigma* equals hier_linear_regression* in logp minus the prior on s
    (-1 / (2 sigma_0^2)) and in every gradient coordinate but s."""
    P, J, N = 4, 7, 45
    c = make_case(model, P, J, N, seed=13, terms=terms)
    if terms:
        c["offset"][N - 1] = 0.25   # (hp_weighted_reference keeps the rows of weight 0: their terms must be finite)
    D = c["D"]
    theta = thetas(c, 3, seed=4)
    theta[:, D - 1] = 0.0
    e = engine(sim, model, c, 3)
    epl = e.dim_padded // 64
    lp, g = e.logp_grad(theta)
    e.close()
    sib = wa.DeviceEngine(FIXED_NOISE[model], D - 1, 3, config(sim), params=c["mp"][:D - 1], lib_path=sim, data=data_of(c),
                          offset=c["offset"], weights=c["weights"])
    assert sib.dim_padded // 64 == epl
    lps, gs = sib.logp_grad(theta[:, :D - 1])
    sib.close()
    ref = hs_case(model, c, theta, epl)
    sm = FIXED_NOISE[model]
    ref_s = hw.case(sm, c["x"], c["y"], c["mp"][:D - 1], theta[:, :D - 1], epl, c["offset"], c["weights"], c["group"])
    prior_s = -1.0 / (2 * c["mp"][D - 1] ** 2)
    assert np.all(np.abs((lp - prior_s) - lps) <= ref[2] + ref_s[2] + 2 * hp.U * np.abs(lp))
    assert np.all(np.abs(g[:, :D - 1] - gs) <= ref[3][:, :D - 1] + ref_s[3])
    assert np.linalg.norm(g[:, :D - 1]) > 0


# ---- hooks ----------------------------------------------------------------------------------------------------------
HOOK_SHAPES = [SHAPES[i] for i in (1, 2, 3, 4, 6)]
HOOK_SHAPE_IDS = [SHAPE_IDS[i] for i in (1, 2, 3, 4, 6)]


@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", MODELS, ids=IDS)
@pytest.mark.parametrize("shape", HOOK_SHAPES, ids=HOOK_SHAPE_IDS)
def test_hooks(sim, model, shape, record_property):
    """log_lik against the pointwise reference, predict against the predict reference, replicate against the sampler probe
    fed predict()'s mu and the device's scale; the folds (log_predictive, predict_fold, replicate_check) with a masked row
    and a live row whose offset is non-zero against the references' folds and the Python-float replays."""
    import hp_replicate_reference as hr
    P, J, N, geometry = shape
    epl = geometry[1]
    c = hook_case(model, P, J, N, seed=11 + P)
    lib = _ffi.load_library(sim)
    worst = 0.0
    for fma in (0, 1):
        h = hooks(sim, model, c, geometry, fma)
        mask = h["mask"]
        assert not mask[1] and mask[0] and c["offset"][0] != 0
        L_rows, b_rows = [], []
        for ci, (theta, ll, (eta, mu, v), rep, gen) in enumerate(zip(h["draws"], h["ll"], h["pred"], h["rep"], h["gen"])):
            ref_ll = hs.pointwise_reference(model, c["x"], c["y"], theta, epl, c["offset"], c["group"])
            ref_pr = hs.predict_reference(model, c["x"], theta, epl, c["offset"], c["group"])
            ratios = hpw.error_ratio(ll, ref_ll), hpp.error_ratio((eta, mu, v), ref_pr)
            print(f"model {model} shape {shape} fma {fma} chain {ci}: error / bound = {ratios[0]:.3f} (log_lik), "
                  f"{ratios[1]:.3f} (eta, mu, v)")
            assert max(ratios) <= 1.0, (fma, ci, ratios)
            worst = max(worst, *ratios)
            # the offset dropped, the constant omitted, the neighbouring group's effect: far outside the bounds
            no_off = hs.pointwise_reference(model, c["x"], c["y"], theta, epl, None, c["group"])["ll"]
            no_const = hs.pointwise_reference(model, c["x"], c["y"], theta, epl, c["offset"], c["group"], constant=False)["ll"]
            assert (np.abs(no_off - ref_ll["ll"]) / ref_ll["bound"]).max() > 10.0
            assert (np.abs(no_const - ref_ll["ll"]) / ref_ll["bound"]).max() > 10.0
            if J >= 2:
                other = hs.predict_reference(model, c["x"], theta, epl, c["offset"], (c["group"] + 1) % J)
                assert (np.abs(other["eta"] - ref_pr["eta"]) / ref_pr["eta_bound"]).max() > 10.0
            L_rows += ref_ll["L"]
            b_rows.append(ref_ll["bound"])
            for t in range(len(theta)):
                s = theta[t, c["D"] - 1]
                assert hm.same_bits(rep[t], hs.replicate_probe(lib, model, mu[t], s, SEED, t, 0)), (ci, t)
                assert hm.same_bits(gen[t], hs.replicate_probe(lib, model, mu[t], s, SEED, ci, t)), (ci, t)
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
@pytest.mark.parametrize("model", [HSIG_C, HSIG], ids=["linear_sigma_c", "linear_sigma"])
def test_replicates_do_not_change_with_the_mask_or_the_launch_size(sim, model, monkeypatch):
    P, J, N, geometry = SHAPES[1]
    c = hook_case(model, P, J, N, seed=8)
    base = hooks(sim, model, c, geometry, 1)
    monkeypatch.setenv("WALNUTS_AMD_POINTWISE_GRID", "1")
    other = hooks(sim, model, c, geometry, 1)
    monkeypatch.delenv("WALNUTS_AMD_POINTWISE_GRID")
    assert same(hook_arrays(base), hook_arrays(other))
    # the check's replicates are the chains block's rows whatever the mask; y and the weights are never read
    ch = wa.MarkovChains.from_host(base["draws"], lib_path=sim)
    e = engine(sim, model, dict(c, y=np.zeros(N)), 1, geometry, 1, weights=np.full(N, 7.0))
    assert same([e.replicate(d, SEED) for d in base["draws"]], base["rep"])
    assert same([a for d in base["draws"] for a in e.predict(d)], [a for m in base["pred"] for a in m])
    full_rep, _ = e.replicate_check(ch, SEED)
    e.close()
    ch.close()
    import hp_replicate_reference as hr
    for ci, n in enumerate(HOOK_LENGTHS):
        eta, mu, v = base["pred"][ci]
        for i in range(n):
            assert hm.same_bits(full_rep[:, ci, i], hr.check_statistics(base["gen"][ci][i], mu[i], v[i], np.ones(N, dtype=bool)))


# ---- runs -----------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", MODELS, ids=IDS)
@pytest.mark.parametrize("geometry", [(1, 2), (1, 8)], ids=["nw1_epl2", "nw1_epl8"])
def test_datasets_and_weight_sets_equal_standalone_engines(sim, model, geometry):
    """datasets= with three grouped datasets of sizes [1, B + 1, 2 B + 3] equals three stand-alone engines bit for bit;
    the same for weight_sets= with W = 3."""
    epl = geometry[1]
    P, J = {2: (3, 4), 8: (130, 140)}[epl]
    B, k = hp.block_rows(epl), 2
    cases = [make_case(model, P, J, n, seed=60 + 7 * i) for i, n in enumerate((1, B + 1, 2 * B + 3))]
    mp, D = cases[0]["mp"], cases[0]["D"]
    cfg = config(sim, geometry, 1)
    e = wa.DeviceEngine(model, D, 3 * k, cfg, params=mp, lib_path=sim, datasets=[data_of(c) for c in cases])
    assert e.num_datasets == 3 and e.dim_padded == 64 * epl
    batched = drive(e, 0)
    e.close()
    for gi, c in enumerate(cases):
        alone = wa.DeviceEngine(model, D, k, cfg, params=mp, lib_path=sim, data=data_of(c))
        compare_blocks(batched, drive(alone, gi * k), gi, k)
        alone.close()
    c = cases[2]
    sets = np.random.default_rng(2).integers(0, 3, size=(3, c["N"])).astype(np.float64)
    e = wa.DeviceEngine(model, D, 3 * k, cfg, params=mp, lib_path=sim, data=data_of(c), weight_sets=sets)
    assert e.num_datasets == 3
    batched = drive(e, 0)
    e.close()
    for gi in range(3):
        alone = wa.DeviceEngine(model, D, k, cfg, params=mp, lib_path=sim, data=data_of(c), weights=sets[gi])
        compare_blocks(batched, drive(alone, gi * k), gi, k)
        alone.close()


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", MODELS, ids=IDS)
def test_non_finite_tau_or_scale(sim, model):
    """Chains placed at s_tau = +-800 or s = +-800: IEEE results, the other chains stay finite, check() is clean."""
    c = make_case(model, 4, 3, 30, seed=4)
    D = c["D"]
    e = engine(sim, model, c, 6, (1, 2), 1)
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
    assert np.all(np.isfinite(e.positions()[4:])) and np.all(np.isfinite(e.logp()[4:]))
    e.close()


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [HSIG, HSIG_C], ids=["linear_sigma", "linear_sigma_c"])
def test_short_run_is_deterministic_and_finite(sim, model):
    def once():
        c = make_case(model, 4, 8, 30, seed=8)
        e = wa.DeviceEngine(model, c["D"], 8, wa.default_config(sim), params=c["mp"], lib_path=sim, data=data_of(c))
        out = drive(e, 0)
        e.close()
        return out
    a, b = once(), once()
    for sa, sb in zip(a, b):
        for key in sb:
            assert np.array_equal(sa[key], sb[key], equal_nan=True), key
    assert np.all(np.isfinite(a[-1]["pos"])) and np.all(np.isfinite(a[-1]["logp"]))


@pytest.mark.timeout(1800)
def test_drop_in_calls_and_wrappers(sim):
    """walnuts_device with data=(x, y, group), offset=, weights=, weight_sets= and datasets=; host draws equal
    kept-on-device draws; the scoring, predicting and replicating wrappers take the fit.  None of these calls needed new
    code: each goes through observations()."""
    model = HSIG
    c = make_case(model, 3, 4, 25, seed=2, terms=True)
    c["offset"][24] = 0.1
    D = c["D"]
    kw = dict(model_params=c["mp"], num_params=D, num_chains=2, seed=9, min_warmup_iter=5, max_warmup_iter=5,
              min_sampling_iter=4, max_sampling_iter=4, lib_path=sim)
    rows = dict(data=data_of(c), offset=c["offset"])
    host = wa.walnuts_device(model, weights=c["weights"], **rows, **kw)
    kept, chains = wa.walnuts_device(model, weights=c["weights"], keep_on_device=True, thin=1, **rows, **kw)
    for a, b in zip(host, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.all(np.isfinite(np.asarray(a)))
    common = dict(num_params=D, lib_path=sim, **rows)
    res = wa.log_predictive(model, chains, **common)
    assert res.lpd.shape == (25,) and np.all(np.isfinite(res.lpd))
    new = (c["x"][:7], c["group"][:7])
    pr = wa.predict(model, chains, num_params=D, data=new, offset=c["offset"][:7], lib_path=sim)
    assert pr.mean.shape == (7,) and np.all(np.isfinite(pr.mean)) and np.all(pr.noise_var > 0)   # sigma^2, estimated
    pd = wa.predict_draws(model, chains, num_params=D, data=new, offset=c["offset"][:7], lib_path=sim)
    assert pd.dims() == 7
    pd.close()
    rd = wa.replicate_draws(model, chains, seed=3, **common)
    assert rd.dims() == 25
    rd.close()
    ppc = wa.posterior_predictive_check(model, chains, seed=3, **common)
    assert np.all((ppc.p_value["mean"] >= 0) & (ppc.p_value["mean"] <= 1))
    chains.close()
    folds = np.ones((2, 25))
    folds[0, ::2], folds[1, 1::2] = 0.0, 0.0
    _, views = wa.walnuts_device(model, weight_sets=folds, keep_on_device=True, **rows, **dict(kw, num_chains=4))
    kf = wa.kfold_elpd(model, views, num_params=D, weight_sets=folds, lib_path=sim, **rows)
    assert kf.lpd.shape == (25,) and np.isfinite(kf.elpd)
    for v in views:
        v.close()
    sets = [data_of(make_case(model, 3, 4, n, seed=3 + n)) for n in (25, 9, 14)]
    kw["num_chains"] = 6
    many = wa.walnuts_device(model, datasets=sets, **kw)
    kept, views = wa.walnuts_device(model, datasets=sets, keep_on_device=True, thin=1, **kw)
    assert len(many) == 6 and len(views) == 3
    for a, b in zip(many, kept):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for v in views:
        v.close()


def test_exact_posterior_quadrature_has_converged():
    """The reference of test_hier_scale_gpu.test_linear_sigma_against_exact_posterior: halving the grid's step moves
    nothing at the tolerance (asserted inside), and halving it once more moves nothing either."""
    x, y, group, mp, P, J = hs.exact_case()
    assert np.bincount(group, minlength=J).min() >= 4
    mean, var = hs.exact_posterior(x, y, group, mp, J)
    mean3, var3, edge = hs.exact_moments(x, y, group, mp, J, 0.03125)
    assert edge <= 1e-12
    assert np.all(np.abs(mean3 - mean) <= 1e-6 * np.sqrt(var)) and np.all(np.abs(var3 - var) <= 1e-6 * var)
    assert 0.3 < mean[P + J + 1] < 1.5 and np.all(var > 0)   # sigma, simulated at 0.7


# ---- refusals and front-end results ---------------------------------------------------------------------------------
def c_abi_error(lib_path, model, D, x, y, group, J, mp=None):
    """wn_engine_create_observed with a hand-filled wn_observations -> the error message ('' if it succeeds)"""
    lib = _ffi.load_library(lib_path)
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    mp = np.ones(D) if mp is None else np.ascontiguousarray(mp, dtype=np.float64)
    obs = _ffi.Observations()
    obs.x, obs.y, obs.num_obs = x.ctypes.data_as(_ffi._dp), y.ctypes.data_as(_ffi._dp), y.size
    if group is not None:
        group = np.ascontiguousarray(group, dtype=np.int32)
        obs.group, obs.num_groups = group.ctypes.data_as(_ffi._i32p), J
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
@pytest.mark.parametrize("model", MODELS, ids=IDS)
def test_refusals(sim, model):
    N = 6
    y, g = np.zeros(N), np.zeros(N, dtype=np.int32)
    cfg = wa.default_config(sim)
    name = {HSIG: "hier_linear_regression_sigma", HSIG_C: "hier_linear_regression_sigma_centered"}[model]

    def py(D, x, match, y=y, group=g, mp=None, **kw):
        with pytest.raises(ValueError, match=match):
            wa.DeviceEngine(model, D, 2, cfg, params=np.ones(D) if mp is None else mp, lib_path=sim,
                            data=(x, y) if group is None else (x, y, group), **kw)

    # a pair instead of a triple: the message names this model's column count
    pair = name + r" model reads a group per observation: .*x \[num_obs\]\[num_params - num_groups - 2\]"
    py(7, np.zeros((N, 7)), pair, group=None)
    assert "num_params - num_groups - 2]" in c_abi_error(sim, model, 7, np.zeros((N, 7)), y, None, 0)
    with pytest.raises(ValueError, match="conditioned on data"):
        wa.DeviceEngine(model, 7, 2, cfg, params=np.ones(7), lib_path=sim)
    # num_params that does not split into P + J + 2; J = 0; P = 0
    split = r"a grouped model with a scale parameter needs num_params == P \+ num_groups \+ 2 with P >= 1 and num_groups >= 1"
    assert "got num_params 7, num_groups 5" in c_abi_error(sim, model, 7, np.zeros((N, 3)), y, g, 5)    # P = 0 from 3 + 5 + 2 = 10
    assert "got num_params 7, num_groups 0" in c_abi_error(sim, model, 7, np.zeros((N, 5)), y, g, 0)    # J = 0
    assert "got num_params 3, num_groups 1" in c_abi_error(sim, model, 3, np.zeros((N, 1)), y, g, 1)    # P = 0
    py(7, np.zeros((N, 5)), split)    # J = 0
    py(7, np.zeros((N, 6)), split)    # J = -1
    py(7, np.zeros((N, 0)), split)    # P = 0
    # varying=2
    py(8, np.zeros((N, 3)), "has no varying slopes", varying=2)
    # sigma_tau and sigma_0
    for i in (5, 6):
        for bad in (0.0, -1.0, np.inf):
            py(7, np.zeros((N, 3)), "sigma_tau, sigma_0.* must be positive and finite", mp=np.where(np.arange(7) == i, bad, 1.0))
    # any finite y is taken
    wa.DeviceEngine(model, 7, 2, cfg, params=np.ones(7), lib_path=sim, data=(np.zeros((N, 3)), y - 0.5, g)).close()
    # one wavefront per chain
    py(1025, np.zeros((N, 1000)), "num_params <= 1024", group=g)
    assert "num_params <= 1024" in c_abi_error(sim, model, 1025, np.zeros((N, 1000)), y, g, 23)
    py(7, np.zeros((N, 3)), r"every group must be in \[0, num_groups\)", group=g + 2)
    # what is accepted
    assert c_abi_error(sim, model, 7, np.zeros((N, 3)), y, g, 2) == ""
    assert c_abi_error(sim, model, 4, np.zeros((N, 1)), y, g, 1) == ""
    assert c_abi_error(sim, model, 1024, np.zeros((N, 1)), y, g, 1021) == ""


def test_front_end_results(sim):
    """wn_model_num_scale_params and wn_model_data_columns for one old model of each kind and the two new ones"""
    lib = _ffi.load_library(sim)
    old = [(wa.MODEL_STD_NORMAL, 0, -1, -1), (wa.MODEL_LINEAR_REGRESSION, 0, 20, 20),
           (wa.MODEL_NEG_BINOMIAL_REGRESSION, 1, 19, 19), (wa.MODEL_LINEAR_REGRESSION_SIGMA, 1, 19, 19),
           (wa.MODEL_HIER_LOGISTIC_REGRESSION, 0, -1, 14), (wa.MODEL_HIER_POISSON_REGRESSION_CENTERED, 0, -1, 14),
           (wa.MODEL_HIER_LINEAR_REGRESSION_SLOPES, 0, -1, 14)]
    for model, scales, flat_cols, grouped_cols in old:
        assert lib.wn_model_num_scale_params(model) == scales, model
        assert lib.wn_model_data_columns(model, 20, 0) == flat_cols, model
        assert lib.wn_model_data_columns(model, 20, 5) == grouped_cols, model
    for model in MODELS:
        assert lib.wn_model_num_scale_params(model) == 1
        assert lib.wn_model_data_columns(model, 20, 0) == -1
        assert lib.wn_model_data_columns(model, 20, 5) == 13
        assert lib.wn_model_data_columns_varying(model, 20, 5, 1) == 13
        assert lib.wn_model_data_columns_varying(model, 20, 5, 2) == -1
    for free in (-1, 37, 38, 39, 63, 64, 1000):
        assert lib.wn_model_num_scale_params(free) == -1
    for tag, model in zip(("hier_linear_regression_sigma", "hier_linear_regression_sigma_centered"), MODELS):
        assert wa.model_id(tag, sim) == model
