"""CPU tier: the count models' maths (wn_devmath.h: dlog1p, dsoftplus, dlgamma_diff = lgamma(y + phi) - lgamma(phi),
ddigamma_diff = psi(y + phi) - psi(phi)) against mpmath, within the bounds stated in DESIGN 3.8.3 and
tests/helpers/hp_count_reference.py.  The functions are evaluated by the host build of the same source, through
wn_internal_count_math_probe of the emulation library; test_count_models_gpu.py compares the device with it bit for
bit."""
import ctypes as C
import math
import os
import sys

import mpmath as mp
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_count_reference as hc  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from walnuts_amd import _ffi  # noqa: E402

U = 2.0 ** -53
Y_DOMAIN = [0.0, 1.0, 2.0, 3.0, 7.0, 30.0, 1e3, 1e6, 2.0 ** 40]
S_DOMAIN = np.linspace(-36.8, 27.6, 47)  # phi = exp(-s) in [1e-12, 1e16]


@pytest.fixture(scope="module")
def lib():
    return _ffi.load_library(simbuild.build())


def probe(lib, fn, x, phi=None):
    x = np.ascontiguousarray(x, dtype=np.float64)
    phi = np.ascontiguousarray(np.zeros_like(x) if phi is None else phi, dtype=np.float64)
    out = np.empty_like(x)
    assert lib.wn_internal_count_math_probe(x.ctypes.data_as(_ffi._dp), phi.ctypes.data_as(_ffi._dp),
                                            out.ctypes.data_as(_ffi._dp), x.size, fn) == 0
    return out


def domain():
    yy, pp = np.meshgrid(np.array(Y_DOMAIN), np.exp(-S_DOMAIN))
    return yy.ravel(), pp.ravel()


def test_log1p_and_softplus_relative_accuracy(lib):
    rng = np.random.default_rng(3)
    x = np.concatenate([-np.exp(rng.uniform(-745, 0, 1500)) * 0.999, np.exp(rng.uniform(-745, 700, 1500)),
                        rng.uniform(-1, 1, 1500), [0.0, -0.0, 5e-324, -5e-324, 1e-300]])
    got = probe(lib, 0, x)
    with mp.workdps(40):
        ref = np.array([float(mp.log1p(mp.mpf(float(v)))) for v in x])
    nz = ref != 0
    assert np.all(got[~nz] == ref[~nz])
    assert np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])) <= hc.C_REL * U
    t = np.concatenate([rng.uniform(-708, 745, 1500), rng.uniform(-40, 40, 1500), [-700.0, -36.0, 0.0, 36.0, 709.0]])
    got = probe(lib, 1, t)
    with mp.workdps(40):
        ref = np.array([float(mp.log1p(mp.exp(mp.mpf(float(v))))) for v in t])
    assert np.max(np.abs(got - ref) / ref) <= hc.C_REL * U
    # the old form max(t, 0) + log(1 + exp(-|t|)) is off by ~u / exp(t) relative as t -> -inf; this one is not
    assert probe(lib, 1, [-40.0])[0] == pytest.approx(math.exp(-40.0), rel=4 * U)
    # special values
    sp = probe(lib, 0, [-1.0, -2.0, np.inf, np.nan, -np.inf])
    assert sp[0] == -np.inf and np.isnan(sp[1]) and sp[2] == np.inf and np.isnan(sp[3]) and np.isnan(sp[4])
    sp = probe(lib, 1, [np.inf, -np.inf, np.nan, -800.0])
    assert sp[0] == np.inf and sp[1] == 0.0 and np.isnan(sp[2]) and sp[3] == 0.0


def test_gamma_differences_against_mpmath(lib):
    y, phi = domain()
    lg = probe(lib, 2, y, phi)
    dg = probe(lib, 3, y, phi)
    worst = 0.0
    for i in range(y.size):
        if y[i] == 0:
            continue
        el = hc.lgamma_diff(y[i], phi[i])
        ed = hc.digamma_diff(y[i], phi[i])
        rl = abs(lg[i] - el) / (hc.abs_lgamma_diff(y[i], phi[i]) * U)
        rd = abs(dg[i] - ed) / (hc.abs_digamma_diff(float(ed), phi[i]) * U)
        assert rl <= hc.C_GAMMA and rd <= hc.C_GAMMA, (y[i], phi[i], float(rl), float(rd))
        worst = max(worst, float(rl), float(rd))
    assert worst > 0.5  # (the comparison is not vacuous)


def test_gamma_differences_vanish_at_zero(lib):
    phi = np.exp(-np.linspace(-40.0, 40.0, 201))
    assert np.all(probe(lib, 2, np.zeros_like(phi), phi) == 0.0)
    assert np.all(probe(lib, 3, np.zeros_like(phi), phi) == 0.0)
    assert np.all(np.signbit(probe(lib, 2, np.zeros_like(phi), phi)) == 0)


def test_recurrences(lib):
    """f(y + 1, phi) = f(y, phi) + log(phi + y),  g(y + 1, phi) = g(y, phi) + 1 / (phi + y), within the two bounds"""
    y, phi = domain()
    keep = y < 2.0 ** 40
    y, phi = y[keep], phi[keep]
    l0, l1 = probe(lib, 2, y, phi), probe(lib, 2, y + 1, phi)
    d0, d1 = probe(lib, 3, y, phi), probe(lib, 3, y + 1, phi)
    for i in range(y.size):
        with mp.workdps(40):
            step_l = mp.log(mp.mpf(float(phi[i])) + mp.mpf(float(y[i])))
            step_d = 1 / (mp.mpf(float(phi[i])) + mp.mpf(float(y[i])))
        bl = hc.C_GAMMA * U * (hc.abs_lgamma_diff(y[i], phi[i]) + hc.abs_lgamma_diff(y[i] + 1, phi[i]))
        ed0, ed1 = hc.digamma_diff(y[i], phi[i]), hc.digamma_diff(y[i] + 1, phi[i])
        bd = hc.C_GAMMA * U * (hc.abs_digamma_diff(float(ed0), phi[i]) + hc.abs_digamma_diff(float(ed1), phi[i]))
        assert abs(l1[i] - (l0[i] + step_l)) <= bl + U * abs(float(step_l)), (y[i], phi[i])
        assert abs(d1[i] - (d0[i] + step_d)) <= bd + U * float(step_d), (y[i], phi[i])


def test_outside_the_domain_within_bound_or_non_finite(lib):
    rng = np.random.default_rng(5)
    phi = np.exp(np.concatenate([rng.uniform(-700, -27.7, 60), rng.uniform(36.9, 700, 60)]))
    y = np.floor(np.exp(rng.uniform(0, 44, phi.size)))
    y = np.concatenate([y, 2.0 ** rng.uniform(40, 62, 40).round()])
    phi = np.concatenate([phi, np.exp(rng.uniform(-27, 36, 40))])
    lg, dg = probe(lib, 2, y, phi), probe(lib, 3, y, phi)
    for i in range(y.size):
        if np.isfinite(lg[i]):
            el = hc.lgamma_diff(y[i], phi[i])
            assert abs(lg[i] - el) <= hc.C_GAMMA * U * hc.abs_lgamma_diff(y[i], phi[i]), (y[i], phi[i])
        if np.isfinite(dg[i]):
            ed = hc.digamma_diff(y[i], phi[i])
            assert abs(dg[i] - ed) <= hc.C_GAMMA * U * hc.abs_digamma_diff(float(ed), phi[i]), (y[i], phi[i])


def test_model_ids_and_columns():
    sim = simbuild.build()
    lib = _ffi.load_library(sim)
    for name, mid in [("poisson_regression", wa.MODEL_POISSON_REGRESSION),
                      ("neg_binomial_regression", wa.MODEL_NEG_BINOMIAL_REGRESSION),
                      ("linear_regression_sigma", wa.MODEL_LINEAR_REGRESSION_SIGMA),
                      ("hier_poisson_regression", wa.MODEL_HIER_POISSON_REGRESSION),
                      ("hier_poisson_regression_centered", wa.MODEL_HIER_POISSON_REGRESSION_CENTERED)]:
        assert wa.model_id(name, sim) == mid
    assert lib.wn_model_data_columns(wa.MODEL_POISSON_REGRESSION, 7, 0) == 7
    assert lib.wn_model_data_columns(wa.MODEL_NEG_BINOMIAL_REGRESSION, 7, 0) == 6
    assert lib.wn_model_data_columns(wa.MODEL_LINEAR_REGRESSION_SIGMA, 7, 0) == 6
    assert lib.wn_model_data_columns(wa.MODEL_LINEAR_REGRESSION, 7, 0) == 7
    assert lib.wn_model_data_columns(wa.MODEL_HIER_POISSON_REGRESSION, 10, 3) == 6
    assert lib.wn_model_data_columns(wa.MODEL_HIER_POISSON_REGRESSION, 10, 0) == -1
    assert lib.wn_model_data_columns(wa.MODEL_STD_NORMAL, 7, 0) == -1
    assert lib.wn_model_data_columns(63, 7, 0) == -1
