"""CPU tier: predictions of the data models (walnuts_amd/csrc/wn_predict.h; wn_engine_predict, wn_engine_predict_fold,
wn_engine_predict_chains, wa.predict, wa.predict_draws) under the workgroup emulation.

References: mpmath with an exact eta and entry bounds counted from the order of operations
(tests/helpers/hp_predict_reference.py); the fold replayed exactly in Python floats.  The device side of the same kernel
source is compared bit for bit in test_predict_gpu.py."""
import math
import os
import sys

import mpmath as mp
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_predict_reference as hpp  # noqa: E402
import hp_weighted_reference as hw  # noqa: E402
import walnuts_amd as wa  # noqa: E402
import wnso  # noqa: E402
from walnuts_amd import models  # noqa: E402
from test_pointwise_sim import (GEOMETRIES, GROUPS, MAIN, MAIN_IDS, OTHER_IDS, OTHERS, SMALL, WIDE, case_for,  # noqa: E402
                                group_of, overflowing_theta, ragged_chains, thetas_for)
from test_weights_sim import config, engine, make_case  # noqa: E402

LIN, LOG, POIS, NB, LSIG, HLOG = hw.LIN, hw.LOG, hw.POIS, hw.NB, hw.LSIG, hw.HLOG
LENGTHS = (5, 3, 4, 1)


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def check_predict(lib, model, geometry, N, fmas=(0, 1), sensitivity=False):
    """eta, mu and v of T = 3 positions against the high-precision reference, error / bound <= 1 in both arithmetic
    modes; a Poisson theta whose row 0 overflows the link: device and reference agree on what is not finite."""
    epl = geometry[1]
    c = case_for(model, WIDE[epl], N, seed=7 * N + epl + model)
    theta = thetas_for(model, c["D"], 3, seed=N)
    if model == POIS:
        theta = overflowing_theta(model, c, theta)
    x = c["data"][0]
    ref = hpp.reference(model, x, theta, epl, c["offset"], group_of(model, c))
    if model == POIS:
        assert ref["mu"][-1, 0] == math.inf and ref["v"][-1, 0] == math.inf and np.isfinite(ref["mu"][:-1]).all()
    worst = 0.0
    for fma in fmas:
        e = engine(lib, model, c, 1, geometry, fma, offset=c["offset"], weights=c["weights"])
        assert e.lanes == 64 and e.dim_padded == 64 * epl
        got = e.predict(theta)
        e.close()
        assert all(a.shape == (3, N) for a in got)
        ratio = hpp.error_ratio(got, ref)
        print(f"model {model} geometry {geometry} fma {fma} N {N}: error / bound = {ratio:.3f}")
        assert ratio <= 1.0, (N, fma, ratio)
        worst = max(worst, ratio)
    if sensitivity:
        far = hpp.sensitivity(model, x, theta, epl, ref, c["offset"], group_of(model, c), c["weights"], GROUPS)
        print(f"model {model} geometry {geometry}: the nearest mistake lies {far:.3g} bounds away")
        assert far > 10.0
    return worst


@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", MAIN, ids=MAIN_IDS)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_values_against_high_precision(sim, model, geometry, record_property):
    """N at the 64-row pack boundaries (129 at two elements per lane only)."""
    record_property("max_error_over_bound", max(check_predict(sim, model, geometry, N, sensitivity=N == 65)
                                                for N in (1, 63, 64, 65) + ((129,) if geometry[1] == 2 else ())))


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", OTHERS, ids=OTHER_IDS)
def test_values_of_the_other_models(sim, model):
    check_predict(sim, model, (1, 2), 65, sensitivity=True)


def check_eta_is_pointwise_eta(lib, model, geometry=(1, 2), N=65):
    """y := the eta predict() returns makes the identity link's residual y - eta vanish exactly when -- and only when --
    pointwise() forms the same eta bit for bit: every l is then fl(-1/2 log 2 pi), in both arithmetic modes."""
    epl = geometry[1]
    c = case_for(model, SMALL[epl], N, seed=31 + model)
    theta = thetas_for(model, c["D"], 2, seed=8)
    with mp.workdps(50):
        const = float(-mp.log(2 * mp.pi) / 2)   # fl(-1/2 log 2 pi), rounded once
    for fma in (0, 1):
        e = engine(lib, model, c, 1, geometry, fma, offset=c["offset"])
        eta, mu, v = e.predict(theta)
        e.close()
        assert np.array_equal(eta, mu) and np.all(v == 1.0)
        for t in range(2):
            data = (c["data"][0], eta[t]) + tuple(c["data"][2:])
            e = engine(lib, model, c, 1, geometry, fma, offset=c["offset"], data=data)
            ll = e.log_lik(theta[t:t + 1])
            e.close()
            assert np.all(ll == const), (fma, t, np.abs(ll - const).max())


@pytest.mark.parametrize("model", [LIN, hw.HLIN, hw.HLIN_C], ids=["linear", "hier_linear", "hier_linear_centered"])
def test_eta_is_the_pointwise_eta(sim, model):
    check_eta_is_pointwise_eta(sim, model)


def fold_case(lib, model, geometry, fma, N=65, seed=17):
    """4 ragged chains in W = 2 blocks over shared rows with the mask n % 3 == 0: the six outputs of predict_fold, the
    per-chain matrices of predict on the same draws taken from the host, and one generated block"""
    epl = geometry[1]
    c = case_for(model, SMALL[epl], N, seed=3 * N + model)
    sets = np.ones((2, N))
    mask = np.tile(np.arange(N) % 3 == 0, (2, 1))
    draws, ch = ragged_chains(model, c["D"], LENGTHS, seed, lib)
    e = engine(lib, model, c, 2, geometry, fma, offset=c["offset"], weight_sets=sets)
    assert e.num_datasets == 2
    fold = e.predict_fold(ch, mask)
    matrices = [e.predict(d) for d in draws]
    gen = e.predict_chains(ch, block=1, what="mean")
    e.close()
    return dict(c=c, draws=draws, chains=ch, fold=fold, matrices=matrices, gen=gen, mask=mask)


def download(chains, max_len, lengths):
    """The [k][max_len][dims] block of generated chains -> list of [len, dims] arrays, read through
    wn_chains_device_draws draw by draw: a view of ONE chain of ONE draw, whose summary mean is that draw itself (x / 1)."""
    lib, dims = chains.lib, chains.dims()
    base, device = lib.wn_chains_device_draws(chains._h), int(lib.wn_chains_device(chains._h))
    out = []
    for c, n in enumerate(lengths):
        rows = []
        for i in range(n):
            one = wa.MarkovChains.from_device(base + (c * max_len + i) * dims * 8, 1, 1, dims, device=device, lib_path=lib._name)
            rows.append(one.mean())
            one.close()
        out.append(np.stack(rows))
    return out


def check_fold_is_the_stated_fold(f):
    """all five outputs and count against the replay of wn_predict.h's fold on predict()'s matrices, exactly"""
    on = f["mask"][0]
    for g in range(2):
        parts = f["matrices"][2 * g:2 * g + 2]
        want = hpp.replay_fold(*([p[i] for p in parts] for i in range(3)))
        for name, got, w in zip(("eta_mean", "eta_var", "mean", "mean_var", "noise_var", "count"), f["fold"], want):
            w = np.where(on, w, 0 if name == "count" else np.nan)
            assert np.array_equal(got[g], w, equal_nan=True), (g, name)
    assert np.array_equal(f["fold"][5], np.where(f["mask"], np.array([[8], [5]]), 0))
    assert np.all(np.isnan(f["fold"][0][~f["mask"]]))


def check_generated_chains(f):
    """block 1's generated chains equal predict()'s matrix bit for bit, lengths respected; their summary mean agrees
    with the fold's mean within the Welford bound"""
    gen, lengths = f["gen"], LENGTHS[2:]
    N = f["matrices"][0][0].shape[1]
    assert gen.num_chains() == 2 and gen.dims() == N and gen.num_draws() == sum(lengths)
    assert gen.min_chain_size() == min(lengths)
    host = download(gen, max(lengths), lengths)
    for c, got in enumerate(host):
        assert np.array_equal(got, f["matrices"][2 + c][1]), c
    T, C = sum(lengths), len(lengths)
    on = f["mask"][1]
    bound = hpp.welford_mean_bound(T, C, np.concatenate(host))
    assert np.all(np.abs(gen.mean() - f["fold"][2][1])[on] <= bound[on])
    return host


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [LOG, NB, HLOG], ids=["logistic", "negbin", "hier_logistic"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("fma", [0, 1])
def test_fold_and_generated_chains(sim, model, geometry, fma):
    f = fold_case(sim, model, geometry, fma)
    check_fold_is_the_stated_fold(f)
    check_generated_chains(f)
    # eta as well, and what= is checked
    c = f["c"]
    e = engine(sim, model, c, 2, geometry, fma, offset=c["offset"], weight_sets=np.ones((2, 65)))
    eta = e.predict_chains(f["chains"], block=0, what="eta")
    for k, got in enumerate(download(eta, max(LENGTHS[:2]), LENGTHS[:2])):
        assert np.array_equal(got, f["matrices"][k][0]), k
    e.close()


def check_fold_invariance(lib, monkeypatch):
    """the same case with a workspace that holds one chain per slab, and with one workgroup: identical bits (the
    library reads both variables at every call)"""
    base = fold_case(lib, LOG, (1, 2), 1)["fold"]
    for name in ("WALNUTS_AMD_POINTWISE_WORKSPACE", "WALNUTS_AMD_POINTWISE_GRID"):
        monkeypatch.setenv(name, "1")
        other = fold_case(lib, LOG, (1, 2), 1)["fold"]
        monkeypatch.delenv(name)
        for a, b in zip(base, other):
            assert np.array_equal(a, b, equal_nan=True), name


def test_fold_is_independent_of_workspace_and_grid(sim, monkeypatch):
    check_fold_invariance(sim, monkeypatch)


def check_wrappers(sim):
    """wa.predict on x alone equals DeviceEngine.predict_fold on the fit's (x, y); wa.predict_draws' quantiles equal the
    summary oracle's on the same values (the comparison of test_summary_gpu.py)."""
    model, geometry, N = HLOG, (1, 2), 65
    c = case_for(model, SMALL[2], N, seed=5)
    cfg = config(sim, geometry, 1)
    draws, ch = ragged_chains(model, c["D"], LENGTHS, 3, sim)
    x, _, group = c["data"]
    e = engine(sim, model, c, 1, geometry, 1, offset=c["offset"])
    want = e.predict_fold(ch)
    matrices = [e.predict(d)[1] for d in draws]
    e.close()
    args = dict(num_params=c["D"], offset=c["offset"], cfg=cfg, lib_path=sim)
    res = wa.predict(model, ch, data=(x, group), **args)
    for name, w in zip(("eta_mean", "eta_var", "mean", "mean_var", "noise_var", "count"), want):
        assert np.array_equal(getattr(res, name), w), name
    assert np.array_equal(res.var, res.noise_var + res.mean_var) and np.array_equal(res.sd, np.sqrt(res.var))
    assert res.evaluated.all() and np.all(res.count == sum(LENGTHS))
    # the fit's own triple, a mask, and blocks given as a sequence of views
    rows = np.arange(N) % 3 == 0
    masked = wa.predict(model, ch, data=c["data"], rows=rows, **args)
    assert np.array_equal(masked.mean[rows], res.mean[rows]) and np.all(np.isnan(masked.mean[~rows]))
    assert np.array_equal(masked.evaluated, rows)
    halves = [wa.MarkovChains.from_host(draws[:2], lib_path=sim), wa.MarkovChains.from_host(draws[2:], lib_path=sim)]
    by_set = wa.predict(model, halves, data=(x, group), weight_sets=np.ones((2, N)), **args)
    whole = wa.predict(model, ch, data=(x, group), weight_sets=np.ones((2, N)), **args)
    assert by_set.mean.shape == (2, N) and np.array_equal(by_set.mean, whole.mean) and np.array_equal(by_set.count, whole.count)
    # a flat model takes x as it is
    cl = make_case(LOG, 5, 9, seed=1)
    dl, chl = ragged_chains(LOG, cl["D"], (2, 2), 1, sim)
    flat = wa.predict(LOG, chl, num_params=cl["D"], data=cl["data"][0], cfg=cfg, lib_path=sim)
    pair = wa.predict(LOG, chl, num_params=cl["D"], data=cl["data"], cfg=cfg, lib_path=sim)
    assert np.array_equal(flat.mean, pair.mean) and np.all((flat.mean > 0) & (flat.mean < 1))
    # predict_draws: MarkovChains of one dimension per row
    gen = wa.predict_draws(model, ch, data=(x, group), what="mean", **args)
    assert gen.num_chains() == len(LENGTHS) and gen.dims() == N and gen.num_draws() == sum(LENGTHS)
    probs = [0.05, 0.5, 0.95]
    q = gen.quantiles(probs)
    assert np.array_equal(q, wnso.quantiles(matrices, probs))
    assert np.array_equal(gen.mean(), wnso.mean(matrices))
    with pytest.raises(ValueError, match="what"):
        wa.predict_draws(model, ch, data=(x, group), what="variance", **args)


@pytest.mark.timeout(1800)
def test_wrappers(sim):
    check_wrappers(sim)


def test_refusals(sim, tmp_path):
    cfg = config(sim, (1, 2), 1)
    c = make_case(LOG, 5, 9, seed=1)
    _, ch = ragged_chains(LOG, c["D"], (2, 2, 2), 1, sim)
    # a model without data
    e = wa.DeviceEngine(wa.MODEL_STD_NORMAL, 5, 2, cfg, lib_path=sim)
    for call in (lambda: e.predict(np.zeros((1, 5))), lambda: e.predict_fold(ch), lambda: e.predict_chains(ch)):
        with pytest.raises(ValueError, match="std_normal model: this engine holds no data"):
            call()
    e.close()
    # dims mismatch, chain count not a multiple of G, dataset / block out of range, what, every output NULL
    e = engine(sim, LOG, c, 2, (1, 2), 1, datasets=[c["data"], c["data"]], data=None)
    _, wrong = ragged_chains(LOG, c["D"] + 1, (2, 2), 1, sim)
    _, even = ragged_chains(LOG, c["D"], (2, 2), 1, sim)
    for call in (e.predict_fold, e.predict_chains):
        with pytest.raises(ValueError, match="dimensions"):
            call(wrong)
        with pytest.raises(ValueError, match="multiple"):
            call(ch)
    with pytest.raises(ValueError, match="dataset must be in"):
        e.predict(np.zeros((1, c["D"])), dataset=2)
    for block in (-1, 2):
        with pytest.raises(ValueError, match="block must be in"):
            e.predict_chains(even, block=block)
    import ctypes as C
    err, out = C.c_void_p(), C.c_void_p()
    assert e.lib.wn_engine_predict_chains(e.h, even._h, 0, 2, C.byref(out), C.byref(err)) != 0
    assert e.lib.walnutpie_get_error_type(err) == 1 and b"what must be 0" in e.lib.walnutpie_get_error_message(err)
    e.lib.walnutpie_destroy_error(err)
    err = C.c_void_p()
    th = np.zeros((1, c["D"]))
    assert e.lib.wn_engine_predict(e.h, th.ctypes.data_as(C.POINTER(C.c_double)), 1, 0, None, None, None, C.byref(err)) != 0
    assert e.lib.walnutpie_get_error_type(err) == 1 and b"every output is NULL" in e.lib.walnutpie_get_error_message(err)
    e.lib.walnutpie_destroy_error(err)
    # one output alone is fine, and equals the full call's
    mean_only = np.empty((1, 9))
    err = C.c_void_p()
    assert e.lib.wn_engine_predict(e.h, th.ctypes.data_as(C.POINTER(C.c_double)), 1, 1, None,
                                   mean_only.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(err)) == 0
    assert np.array_equal(mean_only, e.predict(th, dataset=1)[1]) and np.all(mean_only == 0.5)
    e.close()
    # weight sets share one block of rows
    e = engine(sim, LOG, c, 2, (1, 2), 1, weight_sets=np.ones((2, 9)))
    with pytest.raises(ValueError, match="weight sets share one block"):
        e.predict(th, dataset=1)
    # a mask that turns every row off: nothing is evaluated, all NaN, zero counts
    out = e.predict_fold(even, np.zeros((2, 9)))
    assert all(np.all(np.isnan(a)) for a in out[:5]) and np.all(out[5] == 0)
    e.close()
    # a run-time model without the hook, built as in test_runtime_model.py
    gxx = ["g++", "-x", "c++", "-std=c++20", "-O1", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden", "-pthread",
           "-DWN_CPU_SIM", "-I", os.path.join(HERE, "cpusim")]
    header = os.path.join(HERE, "helpers", "user_diag_model.h")
    so = models.build_device_model(header, "user::MyDiagNormal", "user_diag_pr", 29, 130, out_dir=str(tmp_path),
                                   elems_per_lane=4, lib_path=sim, compiler=gxx)
    mid = models.load_device_model(so, "user_diag_pr", lib_path=sim)
    e = wa.DeviceEngine(mid, 130, 2, wa.default_config(sim, elems_per_lane=4), params=np.ones(130), lib_path=sim)
    _, ch130 = ragged_chains(LOG, 130, (2, 2), 1, sim)
    with pytest.raises(ValueError, match="user_diag_pr"):
        e.predict_fold(ch130)
    e.close()
