"""GPU tier: PSIS-LOO on the device (walnuts_amd/csrc/wn_psis.h) -- bit for bit against the workgroup emulation of the
same source over the CPU tier's cases, against the closed-form leave-one-out density of a linear regression, and end to
end behind walnuts_device(keep_on_device=True)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_psis_reference as hps  # noqa: E402
import hp_weighted_reference as hw  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from test_pointwise_sim import SMALL, case_for  # noqa: E402
from test_psis_sim import (BOUND, CASES, KEYS, chains_for, check_truth, constant_column, every_draw_twice,  # noqa: E402
                           invariance, nan_draw, ragged, run_case, worst_error)
from test_weights_sim import engine, make_case  # noqa: E402

pytestmark = pytest.mark.gpu
LOG, LSIG, HLOG = hw.LOG, hw.LSIG, hw.HLOG


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True), np.nanmax(np.abs(x - y))


@pytest.mark.parametrize("case", CASES, ids=[f"S{c[0]}-N{c[1]}" for c in CASES])
def test_cases_equal_emulation(gpu, sim, case):
    dev, _, _ = run_case(None, case, with_log_lik=False)
    emu, _, _ = run_case(sim, case, with_log_lik=False)
    same_bits(dev, emu)
    assert np.all(dev[4][~np.isnan(dev[0])] == case[0])


@pytest.mark.parametrize("model", [HLOG, LSIG], ids=["hier_logistic", "linear_sigma"])
@pytest.mark.parametrize("geometry", [(1, 4), (1, 8)])
def test_other_models_equal_emulation(gpu, sim, model, geometry):
    """a hierarchical and a scale model at four and eight elements per lane, both arithmetic modes"""
    S, N = 120, 65
    c = case_for(model, SMALL[geometry[1]], N, seed=31 + model)
    for fma in (0, 1):
        got = []
        for lib in (None, sim):
            _, ch = chains_for(model, c["D"], ragged(S), 3, lib)
            e = engine(lib, model, c, 1, geometry, fma, offset=c["offset"])
            got.append(e.psis_loo(ch))
            e.close()
        same_bits(*got)
        assert np.all(np.isfinite(got[0][0])) and np.all(got[0][4] == S)


def test_ties_and_degenerate_columns(gpu, sim):
    for dev, emu in zip(constant_column(None), constant_column(sim)):
        same_bits(dev, emu)
    for half in (13, 103):
        same_bits(every_draw_twice(None, half), every_draw_twice(sim, half))
    dev, emu = nan_draw(None), nan_draw(sim)
    same_bits([getattr(dev, k) for k in KEYS + ("count",)], [getattr(emu, k) for k in KEYS + ("count",)])


def test_invariance(gpu, sim, monkeypatch):
    dev = invariance(None, monkeypatch)
    c = case_for(LOG, 5, 130, seed=21)
    _, ch = chains_for(LOG, c["D"], ragged(200), 9, sim)
    e = engine(sim, LOG, c, 1, (1, 2), 1, offset=c["offset"])
    emu = e.psis_loo(ch)
    e.close()
    same_bits(dev, emu)


@pytest.mark.parametrize("seed", [2, 4])
def test_exact_loo_of_linear_regression(gpu, seed):
    res = check_truth(None, seed)
    if seed == 4:
        assert res.num_bad >= 1 and res.pareto_k[0] > 0.7
    else:
        assert res.num_bad == 0


def test_end_to_end(gpu):
    """Logistic regression, 64 chains x 32 draws resident on the device, N = 130, P = 5: wa.psis_loo equals the float64
    reference applied to DeviceEngine.log_lik of the same draws (taken from the host results) within the CPU tier's
    bound, and p_loo lies between 0 and P + 1."""
    C, T, N, P = 64, 32, 130, 5
    c = make_case(LOG, P, N, seed=12)
    results, chains = wa.walnuts_device(LOG, keep_on_device=True, thin=1, model_params=c["params"], num_params=c["D"],
                                        num_chains=C, seed=3, id=1, init_radius=0.5, min_warmup_iter=60,
                                        max_warmup_iter=60, min_sampling_iter=T, max_sampling_iter=T, data=c["data"],
                                        offset=c["offset"])
    host = np.array([np.asarray(r) for r in results])
    assert host.shape == (C, T, c["D"])
    res = wa.psis_loo(LOG, chains, num_params=c["D"], data=c["data"], offset=c["offset"])
    assert np.all(res.count == C * T)
    e = wa.DeviceEngine(LOG, c["D"], 1, params=np.ones(c["D"]), data=c["data"], offset=c["offset"])
    ll = e.log_lik(host.reshape(C * T, c["D"]))
    e.close()
    ref = hps.numpy_rows(ll)
    worst = worst_error([getattr(res, k) for k in KEYS], np.arange(N), ref)
    print(f"worst |device - float64 reference| {worst:.3g}; p_loo {res.p_loo:.3f}, worst khat {res.pareto_k.max():.3f}")
    assert worst <= BOUND
    assert 0.0 < res.p_loo < P + 1
