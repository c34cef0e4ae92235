"""CPU tier: the data models across elements per lane, under the workgroup emulation.

  * Narrow grouped rows through the hooks: a grouped model's rows hold nx = ceil(P / 128) slot pairs out of the EPL / 2
    that theta has.  At (1, 8) with P = 130 and 300 (nx = 2 and 3 of 4) and at (1, 16) with P = 300 (nx = 3 of 8) the
    pointwise, predict and replicate hooks run the cases 1 < nx < EPL / 2 of load_row and pointwise_eta: log_lik against
    hp_pointwise_reference, predict against hp_predict_reference, replicate against the sampler probe fed predict()'s mu.
    The slopes model enters at varying=1 only: there it is held to its MODEL_HIER_* sibling bit for bit (the two headers
    state the same order of operations), and so to the sibling's reference and bound.  The Q > 1 gather and scatter
    with narrow rows are not run here: test_hier_slopes_sim.py's shape (130, 60, 3, 21, (1, 8)) runs them.
  * One problem at all four one-wavefront geometries: one case per family with offsets and weights (P = 100, N = 65)
    forced onto (1, 2), (1, 4), (1, 8) and (1, 16).  logp, grad, log_lik, eta, mu and v stay within each geometry's own
    counted bound of ONE high-precision reference; the integer-valued outputs and the replicates of the count families
    are identical.

Nothing here was tuned to an observed error: the bounds are hp_weighted_reference.bound, hp_pointwise_reference.k_entry
and hp_predict_reference.k_eta / link_depth.  The device side runs the same checks in test_lane_widths_gpu.py."""
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
import hp_pointwise_reference as hpw  # noqa: E402
import hp_predict_reference as hpp  # noqa: E402
import hp_replicate_reference as hr  # noqa: E402
import hp_weighted_reference as hw  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from walnuts_amd import _ffi  # noqa: E402
from test_pointwise_sim import case_for, overflowing_theta, thetas_for  # noqa: E402
from test_replicate_sim import scales_of  # noqa: E402
from test_weights_sim import engine  # noqa: E402

LOG, POIS, NB, LSIG, HLOG, HPOIS_C = hw.LOG, hw.POIS, hw.NB, hw.LSIG, hw.HLOG, hw.HPOIS_C
SLOG = wa.MODEL_HIER_LOGISTIC_REGRESSION_SLOPES
REFERENCE_MODEL = {SLOG: HLOG}   # varying=1: the sibling's order of operations, parameters and layout
KIND = {"logit": hr.BERNOULLI, "log": hr.POISSON, "negbin": hr.NEGBIN, "sigma": hr.NORMAL}
SEED = 2 ** 33 + 77
N = 65


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def ref_model(model):
    return REFERENCE_MODEL.get(model, model)


def extra(model):
    return dict(varying=1) if model in REFERENCE_MODEL else {}


def replicate_against_probe(lib, model, theta, mu, rep):
    """position t's replicate is the sampler probe under chain t, draw 0, fed predict()'s mu and the family's scale"""
    kind = KIND[hw.family(ref_model(model))]
    scale = scales_of(lib, ref_model(model), theta)
    ffi = _ffi.load_library(lib)
    for t in range(len(theta)):
        want = hr.sampler_probe(ffi, kind, mu[t], np.full(mu[t].shape, scale[t]), SEED, t, 0, 0, hr.GATHER)[0]
        assert hm.same_bits(rep[t], want), t


# ---- narrow grouped rows through the hooks --------------------------------------------------------------------------
NARROW = [((1, 8), 130), ((1, 8), 300), ((1, 16), 300)]   # nx = 2 and 3 of 4; 3 of 8
NARROW_IDS = ["epl8_P130", "epl8_P300", "epl16_P300"]
NARROW_MODELS = (HLOG, HPOIS_C, SLOG)
NARROW_MODEL_IDS = ["hier_logistic", "hier_poisson_centered", "slopes_logistic_q1"]
GROUPS = 40


def narrow_case(model, P, seed):
    """P columns, GROUPS groups (some of them empty at N = 65, row 0 in the last one), offsets; the Poisson case scaled
    as test_replicate_sim.rep_case_data scales it, so that mu straddles the threshold between the two Poisson samplers"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    offset = 0.5 * rng.normal(size=N)
    group = rng.integers(0, GROUPS, size=N).astype(np.int32)
    group[0] = GROUPS - 1
    fam = hw.family(ref_model(model))
    if fam == "log":
        x, offset = 4.0 * x, offset + 1.5
    eta = x @ rng.normal(size=P) * (0.3 if fam == "log" else 1.0) + 0.7 * rng.normal(size=GROUPS)[group] + offset
    y = (rng.poisson(np.exp(np.clip(eta, -5, 4))) if fam == "log" else rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    D = P + GROUPS + 1
    params = rng.uniform(0.5, 4.0, size=D)
    params[P:P + GROUPS] = 1.0
    params[-1] = 1.5
    return dict(data=(x, y, group), params=params, D=D, offset=offset)


def check_narrow_rows(lib, model, geometry, P):
    """-> the worst error / bound over log_lik, eta, mu and v, both arithmetic modes"""
    epl = geometry[1]
    c = narrow_case(model, P, seed=3 * P + epl + ref_model(model))
    x, y, group = c["data"]
    assert 1 < -(-P // 128) < epl // 2
    theta = thetas_for(HLOG, c["D"], 3, seed=P)
    ref_ll = hpw.reference(ref_model(model), x, y, theta, epl, c["offset"], group)
    ref_pr = hpp.reference(ref_model(model), x, theta, epl, c["offset"], group)
    worst = 0.0
    for fma in (0, 1):
        got = {}
        for m in {model, ref_model(model)}:   # (the slopes model: its sibling too, whose reference it borrows)
            e = engine(lib, m, c, 1, geometry, fma, offset=c["offset"], **extra(m))
            assert e.lanes == 64 and e.dim_padded == 64 * epl
            got[m] = (e.log_lik(theta),) + tuple(e.predict(theta)) + (e.replicate(theta, SEED),)
            e.close()
        ll, eta, mu, v, rep = got[model]
        if model in REFERENCE_MODEL:
            assert all(hm.same_bits(a, b) for a, b in zip(got[model], got[ref_model(model)])), fma
        ratios = hpw.error_ratio(ll, ref_ll), hpp.error_ratio((eta, mu, v), ref_pr)
        print(f"model {model} geometry {geometry} P {P} fma {fma}: error / bound = {ratios[0]:.3f} (log_lik), "
              f"{ratios[1]:.3f} (predict)")
        assert max(ratios) <= 1.0, (fma, ratios)
        worst = max(worst, *ratios)
        assert not np.isnan(rep).any()
        replicate_against_probe(lib, model, theta, mu, rep)
        if hw.family(ref_model(model)) == "log":
            assert (mu < 10).any() and (mu >= 10).any()
    o = narrow_case(model, P, seed=977 + P)
    far = hpw.sensitivity(ref_model(model), x, y, theta, epl, ref_ll, c["offset"], group, None,
                          (o["data"][0], o["data"][1], o["offset"], o["data"][2]), np.arange(N) % 3 == 0)
    assert far > 10.0, far
    far = hpp.sensitivity(ref_model(model), x, theta, epl, ref_pr, c["offset"], group, None, GROUPS)
    assert far > 10.0, far
    return worst


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", NARROW_MODELS, ids=NARROW_MODEL_IDS)
@pytest.mark.parametrize("geometry,P", NARROW, ids=NARROW_IDS)
def test_narrow_grouped_rows_through_the_hooks(sim, model, geometry, P, record_property):
    record_property("max_error_over_bound", check_narrow_rows(sim, model, geometry, P))


# ---- one problem at all four geometries -----------------------------------------------------------------------------
WIDTHS = ((1, 2), (1, 4), (1, 8), (1, 16))
FAMILIES = (LOG, POIS, NB, LSIG, HLOG, SLOG)
FAMILY_IDS = ["logistic", "poisson", "negbin", "linear_sigma", "hier_logistic", "slopes_logistic_q1"]
COLUMNS = 100
LENGTHS = (2, 1)


def replay_near_ties(lib, model, theta, mu):
    """-> (the restated samplers' values [T, N], near [T, N]): hp_replicate_reference.replay under chain t, draw 0, on
    predict()'s mu -- and, for the Bernoulli draw u < mu, which the restatement does not mark, |u - mu| within its TIE"""
    kind = KIND[hw.family(ref_model(model))]
    scale = scales_of(lib, ref_model(model), theta)
    ffi = _ffi.load_library(lib)
    values, near = np.empty(mu.shape), np.zeros(mu.shape, dtype=bool)
    for t in range(len(theta)):
        served = np.isfinite(mu[t])
        out, _, nr, _, st = hr.replay(ffi, kind, np.where(served, mu[t], 1.0), scale[t], SEED, t, 0, 0)
        values[t], near[t] = np.where(served, out, np.nan), nr & served
        if kind == hr.BERNOULLI:
            u = st.uniforms(0)[0]
            near[t] |= np.abs(u - mu[t]) <= hr.TIE * np.maximum(np.abs(u), np.abs(mu[t]))
    return values, near


def check_all_widths(lib, model, fmas=(0, 1)):
    """-> {epl: the worst error / bound over logp, grad, log_lik, eta, mu and v}.

    The replicates of a count family are a function of the row's mu through comparisons alone, so two geometries, whose
    mu differ by rounding, give different replicates only where a comparison is a near tie in the sense of
    hp_replicate_reference (within 1e-9 relative; the geometries' mu agree to within their bounds, some 1e-14).  SEED
    was checked under the emulation to give NO near tie on any of these cases (the replay alone reports none, and this
    check asserts it again on every run), so no row is set aside and the replicates are compared for equality.  The
    normal family's replicate sd * z + mu is continuous in mu: it is held to the probe fed its own geometry's mu."""
    rm = ref_model(model)
    fam = hw.family(rm)
    c = case_for(rm, COLUMNS, N, seed=500 + rm)
    x, y = c["data"][:2]
    group = c["data"][2] if rm in hw.HIER else None
    theta = thetas_for(rm, c["D"], 3, seed=6)
    hook_theta = overflowing_theta(rm, c, theta) if rm == POIS else theta   # (the last draw's replicate is invalid)
    mask = np.arange(N) % 3 != 1
    lp_ref, g_ref, lpa, ga = hw.reference(rm, x, y, c["params"], theta, c["offset"], c["weights"], group)
    worst, exact, reps, shared = {}, [], [], None
    for geometry in WIDTHS:
        epl = geometry[1]
        ref_ll = hpw.reference(rm, x, y, hook_theta, epl, c["offset"], group)
        ref_pr = hpp.reference(rm, x, hook_theta, epl, c["offset"], group)
        values = (ref_ll["ll"], ref_pr["eta"], ref_pr["mu"], ref_pr["v"])
        shared = values if shared is None else shared
        assert all(np.array_equal(a, b) for a, b in zip(values, shared))   # one reference: only the bounds differ
        blp, bg = hw.bound(rm, lpa, ga, N, epl)
        worst[epl] = 0.0
        for fma in fmas:
            e = engine(lib, model, c, 3, geometry, fma, offset=c["offset"], weights=c["weights"], **extra(model))
            assert e.lanes == 64 and e.dim_padded == 64 * epl
            lp, g = e.logp_grad(theta)
            e.close()
            ch = wa.MarkovChains.from_host([hook_theta[:LENGTHS[0]], hook_theta[LENGTHS[0]:]], lib_path=lib)
            e = engine(lib, model, c, 1, geometry, fma, offset=c["offset"], weights=c["weights"], **extra(model))
            ll, (eta, mu, v), rep = e.log_lik(hook_theta), e.predict(hook_theta), e.replicate(hook_theta, SEED)
            count = e.log_predictive(ch, mask)[3]
            fold_count = e.predict_fold(ch, mask)[5]
            stat_rep, stat_obs = e.replicate_check(ch, SEED, mask)
            e.close()
            ch.close()
            ratios = (hw.error_ratio(lp, g, (lp_ref, g_ref, blp, bg)), hpw.error_ratio(ll, ref_ll),
                      hpp.error_ratio((eta, mu, v), ref_pr))
            print(f"model {model} geometry {geometry} fma {fma}: error / bound = {ratios[0]:.3f} (logp, grad), "
                  f"{ratios[1]:.3f} (log_lik), {ratios[2]:.3f} (eta, mu, v)")
            assert max(ratios) <= 1.0, (geometry, fma, ratios)
            worst[epl] = max(worst[epl], *ratios)
            invalid = (np.isnan(stat_rep[0]) & ~np.isnan(stat_obs[0])).sum(axis=1)   # (per chain, as the wrapper counts)
            exact.append([count, fold_count, invalid, stat_obs[[0, 1, 2, 3, 4]]])
            if fam == "sigma":
                replicate_against_probe(lib, model, hook_theta, mu, rep)
            else:
                want, near = replay_near_ties(lib, model, hook_theta, mu)
                assert not near.any(), (geometry, fma, np.argwhere(near))
                assert hm.same_bits(rep, want), (geometry, fma)
                reps.append([rep, stat_rep[[0, 1, 2, 3, 4]]])   # sums of integers are exact: only Pearson's moves
    for group_of_outputs in (exact, reps):
        for other in group_of_outputs[1:]:
            assert all(hm.same_bits(a, b) for a, b in zip(group_of_outputs[0], other))
    assert exact[0][0][mask].min() == sum(LENGTHS) and np.all(exact[0][0][~mask] == 0)
    assert exact[0][2].tolist() == ([0, 1] if rm == POIS else [0, 0])
    return worst


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", FAMILIES, ids=FAMILY_IDS)
def test_one_problem_at_every_width(sim, model, record_property):
    for epl, ratio in check_all_widths(sim, model).items():
        record_property(f"max_error_over_bound_epl{epl}", ratio)
