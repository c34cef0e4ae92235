"""CPU tier: the pointwise log-likelihood and the predictive fold (walnuts_amd/csrc/wn_pointwise.h; wn_engine_log_lik,
wn_engine_log_predictive, wa.log_predictive, wa.kfold_elpd) under the workgroup emulation.

References: mpmath with an exact eta and entry / fold bounds counted from the order of operations
(tests/helpers/hp_pointwise_reference.py).  The device side of the same kernel source is compared bit for bit in
test_pointwise_gpu.py."""
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
import hp_pointwise_reference as hpw  # noqa: E402
import hp_weighted_reference as hw  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from walnuts_amd import models  # noqa: E402
from test_weights_sim import config, engine, fold_weights, make_case, thetas  # noqa: E402

LIN, LOG, POIS, NB, LSIG, HLOG = hw.LIN, hw.LOG, hw.POIS, hw.NB, hw.LSIG, hw.HLOG
HPOIS_C = hw.HPOIS_C
GROUPS = 3
MAIN = (LOG, POIS, NB, LSIG, HLOG, HPOIS_C)
MAIN_IDS = ["logistic", "poisson", "negbin", "linear_sigma", "hier_logistic", "hier_poisson_centered"]
OTHERS = (LIN, hw.HLIN, hw.HLIN_C, hw.HLOG_C, hw.HPOIS)
OTHER_IDS = ["linear", "hier_linear", "hier_linear_centered", "hier_logistic_centered", "hier_poisson"]
GEOMETRIES = ((1, 2), (1, 4), (1, 8), (1, 16))
WIDE = {2: 100, 4: 200, 8: 400, 16: 1000}   # columns of x of the l-against-reference cases
SMALL = {2: 5, 4: 70, 8: 150, 16: 40}     # ... of the fold / invariance cases
U = 2.0 ** -53


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def case_for(model, P, N, seed):
    """test_weights_sim.make_case for every built-in data model (the hierarchical ones reuse HLOG's layout)"""
    if model in hw.HIER and model != HLOG:
        c = make_case(HLOG, P, N, seed)
        x, _, group = c["data"]
        rng = np.random.default_rng(seed + 1)
        eta = x @ rng.normal(size=P) + c["offset"]
        fam = hw.family(model)
        y = rng.poisson(np.exp(eta)).astype(np.float64) if fam == "log" else (
            eta + 0.7 * rng.normal(size=N) if fam == "identity" else c["data"][1])
        c["data"] = (x, y, group)
        return c
    return make_case(model, P, N, seed)


def thetas_for(model, D, T, seed):
    return thetas(HLOG if model in hw.HIER else model, D, T, seed)


def group_of(model, c):
    return c["data"][2] if model in hw.HIER else None


def overflowing_theta(model, c, theta):
    """theta[-1] such that row 0's eta is about 900: the Poisson link overflows there (exp(eta) = inf, l = -inf)"""
    x = c["data"][0]
    P = x.shape[1]
    theta = theta.copy()
    theta[-1, :] = 0.0
    theta[-1, :P] = 900.0 * x[0] / float(x[0] @ x[0])
    return theta


def check_log_lik(lib, model, geometry, N, fmas=(0, 1), sensitivity=False):
    epl = geometry[1]
    c = case_for(model, WIDE[epl], N, seed=7 * N + epl + model)
    theta = thetas_for(model, c["D"], 3, seed=N)
    if model == POIS:
        theta = overflowing_theta(model, c, theta)
    x, y = c["data"][:2]
    ref = hpw.reference(model, x, y, theta, epl, c["offset"], group_of(model, c))
    if model == POIS:
        assert ref["ll"][-1, 0] == -math.inf and np.isfinite(ref["ll"][:-1]).all()
    worst = 0.0
    for fma in fmas:
        e = engine(lib, model, c, 1, geometry, fma, offset=c["offset"], weights=c["weights"])
        assert e.lanes == 64 and e.dim_padded == 64 * epl
        ll = e.log_lik(theta)
        e.close()
        assert ll.shape == (3, N)
        ratio = hpw.error_ratio(ll, ref)
        print(f"model {model} geometry {geometry} fma {fma} N {N}: error / bound = {ratio:.3f}")
        assert ratio <= 1.0, (N, fma, ratio)
        worst = max(worst, ratio)
    if sensitivity:
        o = case_for(model, WIDE[epl], N, seed=1234 + model)
        mask = np.arange(N) % 3 == 0
        far = hpw.sensitivity(model, x, y, theta, epl, ref, c["offset"], group_of(model, c), c["weights"],
                              (o["data"][0], o["data"][1], o["offset"], group_of(model, o)), mask)
        print(f"model {model} geometry {geometry}: the nearest mistake lies {far:.3g} bounds away")
        assert far > 10.0
    return worst


@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", MAIN, ids=MAIN_IDS)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_log_lik_against_high_precision(sim, model, geometry, record_property):
    """T = 3; N at the 64-row pack boundaries (129 at P = 100 only); both arithmetic modes; a theta that overflows the
    Poisson link: reference and device agree on non-finiteness there."""
    record_property("max_error_over_bound", max(check_log_lik(sim, model, geometry, N, sensitivity=N == 65)
                                                for N in (1, 63, 64, 65) + ((129,) if geometry[1] == 2 else ())))


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", OTHERS, ids=OTHER_IDS)
def test_log_lik_of_the_other_models(sim, model):
    check_log_lik(sim, model, (1, 2), 65, sensitivity=True)


def ulp(v):
    return math.ulp(abs(float(v))) if v != 0 else 0.0


def test_host_constants_within_one_ulp(sim):
    """c_n read back through l at theta = 0.  Poisson: eta = 0, the term is 0 * y - dexp(0) = -1 exactly, l = fl(c - 1);
    where c and c - 1 share a binade that add is exact and l + 1 IS the uploaded constant; elsewhere the add rounds once
    (half an ulp of l).  Linear regression with y = 0: the term is 0, l is the constant itself."""
    ys = np.array(list(range(0, 200)) + [1e3, 12345.0, 1e6, 1e9, 2.0 ** 40, 1e15])
    x = np.zeros((ys.size, 5))
    e = wa.DeviceEngine(POIS, 5, 1, config(sim, (1, 2), 0), params=np.ones(5), data=(x, ys), lib_path=sim)
    ll = e.log_lik(np.zeros((1, 5)))[0]
    e.close()
    exact = 0
    with mp.workdps(60):
        for y, l in zip(ys, ll):
            c = -mp.loggamma(mp.mpf(float(y)) + 1)
            cf = float(c)
            if cf == 0.0 or math.frexp(cf)[1] == math.frexp(cf - 1.0)[1]:
                exact += 1
                assert abs(mp.mpf(float(l + 1.0)) - c) <= ulp(cf), y
            else:
                assert abs(mp.mpf(float(l)) - (c - 1)) <= ulp(cf) + 0.5 * ulp(l), y
        assert exact > ys.size // 2
        e = wa.DeviceEngine(LIN, 5, 1, config(sim, (1, 2), 0), params=np.ones(5), data=(x[:3], np.zeros(3)), lib_path=sim)
        l0 = e.log_lik(np.zeros((1, 5)))[0]
        e.close()
        c = -mp.log(2 * mp.pi) / 2
        assert np.all(l0 == l0[0]) and abs(mp.mpf(float(l0[0])) - c) <= ulp(float(c))


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [LOG, NB, LSIG, HLOG], ids=["logistic", "negbin", "linear_sigma", "hier_logistic"])
@pytest.mark.parametrize("weighted", [False, True])
def test_tie_to_the_samplers_density(sim, model, weighted):
    """sum_n w_n (l_n - c_n) + prior(theta) against logp_grad's logp, within the sum of the two bounds (l_n - c_n is the
    row term the models' densities sum: they drop exactly c_n).  The prior: hp_weighted_reference (mpmath) with every
    weight 0."""
    geometry, epl, N = (1, 2), 2, 65
    c = make_case(model, SMALL[epl], N, seed=50 + model)
    theta = thetas(model, c["D"], 2, seed=5)
    x, y = c["data"][:2]
    group = group_of(model, c)
    w = c["weights"] if weighted else None
    e = engine(sim, model, c, 2, geometry, 1, offset=c["offset"], weights=w)
    lp, _ = e.logp_grad(theta)
    ll = e.log_lik(theta)
    e.close()
    ref = hpw.reference(model, x, y, theta, epl, c["offset"], group)
    lp_ref, _, lp_bound, _ = hw.case(model, x, y, c["params"], theta, epl, c["offset"], w, group)
    prior = hw.reference(model, x, y, c["params"], theta, c["offset"], np.zeros(N), group)[0]
    wts = np.ones(N) if w is None else w
    with mp.workdps(60):
        for t in range(2):
            cn = [hpw.row_const(hw.family(model), mp.mpf(float(v))) for v in y]
            total = mp.fsum(mp.mpf(float(wts[n])) * (mp.mpf(float(ll[t, n])) - cn[n]) for n in range(N)) + mp.mpf(float(prior[t]))
            slack = float(np.sum(wts * ref["bound"][t])) + lp_bound[t] + U * abs(prior[t])
            assert abs(float(total - mp.mpf(float(lp[t])))) <= slack, (t, float(total), lp[t], slack)


def ragged_chains(model, D, lengths, seed, lib):
    """host draws per chain and their MarkovChains (from_host, ragged)"""
    draws = [thetas_for(model, D, n, seed + i) for i, n in enumerate(lengths)]
    return draws, wa.MarkovChains.from_host(draws, lib_path=lib)


def check_block(out, sl, ref_rows, bound_rows, chains, mask=None):
    """lpd / mean / var / count of one block (slice sl of the outputs) against the reference fold"""
    lpd, mean, var, count = (a[sl] for a in out)
    f = hpw.fold(ref_rows, bound_rows, chains)
    on = np.ones(lpd.shape, dtype=bool) if mask is None else mask
    T = len(ref_rows)
    assert np.all(count[on] == T) and np.all(count[~on] == 0)
    assert np.all(np.isnan(lpd[~on])) and np.all(np.isnan(mean[~on])) and np.all(np.isnan(var[~on]))
    assert np.all(np.abs(lpd[on] - f["lpd"][on]) <= f["lpd_bound"][on])
    assert np.all(np.abs(mean[on] - f["mean"][on]) <= f["mean_bound"][on])
    if T > 1:
        assert np.all(np.abs(var[on] - f["var"][on]) <= f["var_bound"][on])
    else:
        assert np.all(np.isnan(var[on]))


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [LOG, NB, HLOG], ids=["logistic", "negbin", "hier_logistic"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_log_predictive_datasets_and_weight_sets(sim, model, geometry):
    epl = geometry[1]
    P = SMALL[epl]
    lengths = (5, 3, 5, 1)
    a, b = case_for(model, P, 65, seed=11 + model), case_for(model, P, 7, seed=12 + model)
    draws, ch = ragged_chains(model, a["D"], lengths, 3, sim)
    cfg = config(sim, geometry, 1)
    # G = 2 datasets of different size: chains 0-1 on a, 2-3 on b
    res = wa.log_predictive(model, ch, num_params=a["D"], datasets=[a["data"], b["data"]], offset=[a["offset"], None],
                            cfg=cfg, lib_path=sim)
    first = 0
    for g, (c, off) in enumerate(((a, a["offset"]), (b, None))):
        th = np.concatenate(draws[2 * g:2 * g + 2])
        x, y = c["data"][:2]
        ref = hpw.reference(model, x, y, th, epl, off, group_of(model, c))
        check_block((res.lpd, res.mean, res.var, res.count), slice(first, first + y.size), ref["L"], ref["bound"], 2)
        first += y.size
    assert np.isfinite(res.elpd) and np.isfinite(res.se) and res.p_waic > 0 and np.isfinite(res.waic)
    # W = 2 weight sets over a's rows with a mask: set 0 scores rows n % 3 == 0, set 1 the rows n % 3 == 1
    sets = np.stack([(np.arange(65) % 3 != g).astype(np.float64) for g in range(2)])
    res = wa.log_predictive(model, ch, num_params=a["D"], data=a["data"], offset=a["offset"], weight_sets=sets, cfg=cfg,
                            lib_path=sim)
    x, y = a["data"][:2]
    for g in range(2):
        th = np.concatenate(draws[2 * g:2 * g + 2])
        ref = hpw.reference(model, x, y, th, epl, a["offset"], group_of(model, a))
        check_block(tuple(v[g] for v in (res.lpd, res.mean, res.var, res.count)), slice(None), ref["L"], ref["bound"], 2,
                    sets[g] == 0)
    # a block whose chains hold one draw in total: var is NaN
    one = wa.MarkovChains.from_host([draws[3]], lib_path=sim)
    r1 = wa.log_predictive(model, one, num_params=a["D"], data=a["data"], offset=a["offset"], cfg=cfg, lib_path=sim)
    assert np.all(r1.count == 1) and np.all(np.isnan(r1.var)) and np.all(np.isfinite(r1.lpd))
    assert np.array_equal(r1.lpd, r1.mean)


def test_log_predictive_with_minus_infinity(sim):
    """Poisson rows whose link overflows: l = -inf at ONE draw contributes 0 to the sum (lpd finite, the mean -inf);
    l = -inf at ALL draws gives lpd = -inf."""
    geometry, epl = (1, 2), 2
    c = make_case(POIS, SMALL[epl], 6, seed=2)
    x, y = c["data"]
    D = c["D"]
    big = 900.0 * x[0] / float(x[0] @ x[0])        # eta_0 ~ 900
    both = np.linalg.pinv(x[:2]) @ np.array([900.0, 900.0])  # ... and eta_1 as well (the minimum-norm solution)
    th = thetas(POIS, D, 4, seed=1)
    e = wa.DeviceEngine(POIS, D, 1, config(sim, geometry, 1), params=np.ones(D), data=c["data"], lib_path=sim)
    ll_big = e.log_lik(np.stack([big, both]))
    assert ll_big[0, 0] == -math.inf and ll_big[1, 0] == -math.inf
    draws = np.concatenate([th, both[None]])   # one overflowing draw among five
    ll = e.log_lik(draws)
    inf_rows = np.flatnonzero(np.isinf(ll[-1]))
    assert 0 in inf_rows and np.isfinite(ll[:-1]).all()
    lpd, mean, var, count = e.log_predictive(wa.MarkovChains.from_host([draws[:2], draws[2:]], lib_path=sim))
    for n in inf_rows:
        expect = np.log(np.sum(np.exp(ll[:-1, n] - ll[:-1, n].max()))) + ll[:-1, n].max() - np.log(5)
        assert abs(lpd[n] - expect) <= 1e-12 * max(1.0, abs(expect)) and mean[n] == -math.inf and np.isnan(var[n])
    allinf = np.stack([both, both, both])
    lpd, mean, var, count = e.log_predictive(wa.MarkovChains.from_host([allinf[:1], allinf[1:]], lib_path=sim))
    assert lpd[0] == -math.inf and count[0] == 3
    e.close()


def numpy_fold(ll_chains):
    """the fold wn_pointwise.h states, in numpy float64 on log_lik rows: per chain sequentially, chains merged in order"""
    state = None
    for ll in ll_chains:
        m, s, mean, m2 = np.full(ll.shape[1], -np.inf), np.zeros(ll.shape[1]), np.zeros(ll.shape[1]), np.zeros(ll.shape[1])
        for i, l in enumerate(ll):
            up = l > m
            with np.errstate(invalid="ignore"):
                ex = np.exp(np.where(l == m, 0.0, -np.abs(l - m)))
            s = np.where(up, s * ex + 1.0, s + ex)
            m = np.where(up, l, m)
            d = l - mean
            mean = mean + d / (i + 1)
            m2 = m2 + d * (l - mean)
        n = float(len(ll))
        if state is None:
            state = (n, m, s, mean, m2)
            continue
        na, ma, sa, meana, m2a = state
        big = np.maximum(ma, m)
        s = sa * np.exp(ma - big) + s * np.exp(m - big)
        nn = na + n
        d = mean - meana
        state = (nn, big, s, meana + d * (n / nn), (m2a + m2) + (d * d) * (na * n / nn))
    n, m, s, mean, m2 = state
    return m + np.log(s) - np.log(n), mean, m2 / (n - 1)


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [LOG, NB], ids=["logistic", "negbin"])
def test_invariance(sim, model, monkeypatch):
    geometry, epl, N = (1, 2), 2, 70
    c = make_case(model, SMALL[epl], N, seed=21 + model)
    lengths = (5, 3, 5, 1)
    draws, ch = ragged_chains(model, c["D"], lengths, 9, sim)
    e = engine(sim, model, c, 1, geometry, 1, offset=c["offset"])
    base = e.log_predictive(ch)
    # the fold of log_lik rows in numpy, in the stated order, to the fold's own bound (the entries are the device's own)
    lls = [e.log_lik(d) for d in draws]
    lpd, mean, var = numpy_fold(lls)
    allrows = np.concatenate(lls)
    T, C = allrows.shape[0], len(lengths)
    spread = allrows.max(axis=0) - allrows.min(axis=0)
    big = np.abs(allrows).max(axis=0)
    lpd_b = U * ((T + C) * (6 + spread) + 6 * (2 * big + math.log(T) + 1)) * 2   # both sides round
    mean_b = 2 * 4 * (T + C) * U * big
    assert np.all(np.abs(base[0] - lpd) <= lpd_b) and np.all(np.abs(base[1] - mean) <= mean_b)
    dev = np.abs(allrows - allrows.mean(axis=0)).max(axis=0)
    assert np.all(np.abs(base[2] - var) <= 2 * dev * mean_b * T / (T - 1) + 2 * 8 * (T + C) * U * var)
    # two grids, and a workspace that holds one chain at a time: identical bits
    monkeypatch.setenv("WALNUTS_AMD_POINTWISE_GRID", "3")
    small_grid = e.log_predictive(ch)
    monkeypatch.delenv("WALNUTS_AMD_POINTWISE_GRID")
    monkeypatch.setenv("WALNUTS_AMD_POINTWISE_WORKSPACE", "1")
    one_chain_slabs = e.log_predictive(ch)
    monkeypatch.delenv("WALNUTS_AMD_POINTWISE_WORKSPACE")
    for other in (small_grid, one_chain_slabs):
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(base, other))
    e.close()
    # permuting the rows of the data permutes the outputs bit for bit
    perm = np.random.default_rng(4).permutation(N)
    cp = dict(c, data=tuple(a[perm] for a in c["data"]), offset=c["offset"][perm])
    e = engine(sim, model, cp, 1, geometry, 1, offset=cp["offset"])
    permuted = e.log_predictive(ch)
    e.close()
    assert all(np.array_equal(a[perm], b) for a, b in zip(base, permuted))


def valid_folds(W, N, rng):
    """fold_weights with row 0 held out by set 0 again (fold_weights gives it a weight there, so that no two sets are
    alike: as it stands its row 0 is held out by no set)"""
    sets = fold_weights(W, N, rng)
    sets[0, 0] = 0.0
    return sets


@pytest.mark.timeout(1800)
def test_kfold_elpd(sim):
    model, geometry, epl, W, N = LOG, (1, 2), 2, 4, 30
    c = make_case(model, SMALL[epl], N, seed=77)
    cfg = config(sim, geometry, 1)
    draws, ch = ragged_chains(model, c["D"], (3, 2, 3, 2, 3, 2, 3, 2), 13, sim)
    sets = valid_folds(W, N, np.random.default_rng(9))
    args = dict(num_params=c["D"], data=c["data"], offset=c["offset"], cfg=cfg, lib_path=sim)
    kf = wa.kfold_elpd(model, ch, weight_sets=sets, **args)
    per_set = wa.log_predictive(model, ch, weight_sets=sets, **args)
    assert kf.lpd.shape == (N,) and np.all(kf.count == 5)
    for n in range(N):
        g = n % W
        assert sets[g, n] == 0
        for a, b in ((kf.lpd, per_set.lpd), (kf.mean, per_set.mean), (kf.var, per_set.var), (kf.count, per_set.count)):
            assert a[n] == b[g, n]
    assert np.isfinite(kf.elpd) and kf.elpd == float(np.sum(kf.lpd)) and np.isfinite(kf.se)
    # the K views of the same chains give the same bits
    views = [wa.MarkovChains.from_host(draws[2 * g:2 * g + 2], lib_path=sim) for g in range(W)]
    kv = wa.kfold_elpd(model, views, weight_sets=sets, **args)
    assert np.array_equal(kv.lpd, kf.lpd) and np.array_equal(kv.var, kf.var)
    # a row held out never (fold_weights as it stands) or twice
    with pytest.raises(ValueError, match="row 0 is held out by 0"):
        wa.kfold_elpd(model, ch, weight_sets=fold_weights(W, N, np.random.default_rng(9)), **args)
    twice = sets.copy()
    twice[1, 4] = 0.0
    with pytest.raises(ValueError, match="row 4 is held out by 2"):
        wa.kfold_elpd(model, ch, weight_sets=twice, **args)


def test_refusals(sim, tmp_path):
    cfg = config(sim, (1, 2), 1)
    c = make_case(LOG, 5, 9, seed=1)
    _, ch = ragged_chains(LOG, c["D"], (2, 2, 2), 1, sim)
    # a model without data
    e = wa.DeviceEngine(wa.MODEL_STD_NORMAL, 5, 2, cfg, lib_path=sim)
    with pytest.raises(ValueError, match="std_normal"):
        e.log_lik(np.zeros((1, 5)))
    with pytest.raises(ValueError, match="std_normal"):
        e.log_predictive(ch)
    e.close()
    # dims mismatch, chain count not a multiple of G
    e = engine(sim, LOG, c, 2, (1, 2), 1, datasets=[c["data"], c["data"]], data=None)
    _, wrong = ragged_chains(LOG, c["D"] + 1, (2, 2), 1, sim)
    with pytest.raises(ValueError, match="dimensions"):
        e.log_predictive(wrong)
    with pytest.raises(ValueError, match="multiple"):
        e.log_predictive(ch)
    with pytest.raises(ValueError, match="dataset"):
        e.log_lik(np.zeros((1, c["D"])), dataset=2)
    e.close()
    # a run-time model without the hook, built as in test_runtime_model.py
    gxx = ["g++", "-x", "c++", "-std=c++20", "-O1", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden", "-pthread",
           "-DWN_CPU_SIM", "-I", os.path.join(HERE, "cpusim")]
    header = os.path.join(HERE, "helpers", "user_diag_model.h")
    so = models.build_device_model(header, "user::MyDiagNormal", "user_diag_pw", 9, 130, out_dir=str(tmp_path),
                                   elems_per_lane=4, lib_path=sim, compiler=gxx)
    mid = models.load_device_model(so, "user_diag_pw", lib_path=sim)
    e = wa.DeviceEngine(mid, 130, 2, wa.default_config(sim, elems_per_lane=4), params=np.ones(130), lib_path=sim)
    _, ch130 = ragged_chains(LOG, 130, (2, 2), 1, sim)
    with pytest.raises(ValueError, match="user_diag_pw"):
        e.log_predictive(ch130)
    e.close()
