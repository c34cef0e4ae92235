"""CPU tier: per-row offsets and weights of the data models and weight sets over one shared block of rows
(wn_observations::offset / weight / num_weight_sets; DeviceEngine(offset=, weights=, weight_sets=),
walnuts_device(...)) under the workgroup emulation.

References: mpmath with an exact eta and a per-chain K u bound (tests/helpers/hp_weighted_reference.py); standalone
engines, bit for bit, for trailing zero weights, weight sets and datasets with their own offsets and weights.  The
device side of the same kernel source is compared bit for bit in test_weights_gpu.py."""
import ctypes as C
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
import hp_reference as hp  # noqa: E402
import hp_weighted_reference as hw  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from walnuts_amd import models  # noqa: E402
from test_datasets_sim import compare_blocks, drive, drop_in, flat  # noqa: E402

LIN, LOG, POIS, NB, LSIG, HLOG = hw.LIN, hw.LOG, hw.POIS, hw.NB, hw.LSIG, hw.HLOG
MODELS = (LIN, LOG, POIS, NB, LSIG, HLOG)
IDS = ["linear", "logistic", "poisson", "negbin", "linear_sigma", "hier_logistic"]
GEOMETRIES = ((1, 2), (1, 4), (1, 8), (1, 16))
COLUMNS = {2: 5, 4: 70, 8: 150, 16: 40}  # columns of x: one wavefront per chain, with padding
GROUPS = 3
COMBOS = ("offset", "weights", "both")


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def dims(model, P):
    """num_params for P columns of x"""
    return P + (1 if model in (NB, LSIG) else 0) + (GROUPS + 1 if model == HLOG else 0)


def make_case(model, P, N, seed):
    """dict(data=(x, y[, group]), params, D, offset, weights): moderate values; weights in (0.25, 3) with a ZERO at row
    1 (inside the first block) when N > 2."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    offset = rng.normal(size=N) * 0.5
    eta = x @ rng.normal(size=P) + offset
    group = rng.integers(0, GROUPS, size=N).astype(np.int32)
    fam = hw.family(model)
    if fam == "logit":
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    elif fam == "log":
        y = rng.poisson(np.exp(eta)).astype(np.float64)
    elif fam == "negbin":
        y = rng.negative_binomial(2.0, 2.0 / (2.0 + np.exp(eta))).astype(np.float64)
    else:
        y = eta + 0.7 * rng.normal(size=N)
    D = dims(model, P)
    params = rng.uniform(0.5, 4.0, size=D)
    if model == HLOG:
        params[P:P + GROUPS] = 1.0
        params[-1] = 1.5
    if model in (NB, LSIG):
        params[-1] = 2.0
    weights = rng.uniform(0.25, 3.0, size=N)
    if N > 2:
        weights[1] = 0.0
    data = (x, y, group) if model == HLOG else (x, y)
    return dict(data=data, params=params, D=D, offset=offset, weights=weights)


def thetas(model, D, C, seed):
    th = np.random.default_rng(seed).normal(size=(C, D)) * 0.3
    if model in (NB, LSIG, HLOG):
        th[:, -1] = np.resize([0.3, -0.5], C)
    return th


def config(lib, geometry, fma, **kw):
    return wa.default_config(lib, fused_multiply_add=fma, waves_per_chain=geometry[0], elems_per_lane=geometry[1], **kw)


def engine(lib, model, c, num_chains, geometry, fma, **kw):
    args = dict(data=c["data"], params=c["params"])
    args.update(kw)
    return wa.DeviceEngine(model, c["D"], num_chains, config(lib, geometry, fma), lib_path=lib, **args)


def reference_args(c):
    d = c["data"]
    return d[0], d[1], c["params"]


def edge_ns(epl):
    B = hp.block_rows(epl)
    return sorted({1, B - 1, B, B + 1})


def check_edge_matrix(lib, model, geometry, fma):
    """Test 1 (also run on the device by test_weights_gpu.py): every combination at N in {1, B - 1, B, B + 1} within
    the bound, and the three mistakes of hw.sensitivity at least 100 bounds away."""
    epl = geometry[1]
    worst = 0.0
    for N in edge_ns(epl):
        c = make_case(model, COLUMNS[epl], N, seed=100 * N + epl + model)
        theta = thetas(model, c["D"], 2, seed=N)
        group = c["data"][2] if model == HLOG else None
        for combo in COMBOS:
            o = c["offset"] if combo != "weights" else None
            w = c["weights"] if combo != "offset" else None
            e = engine(lib, model, c, 2, geometry, fma, offset=o, weights=w)
            assert e.lanes == 64 and e.dim_padded == 64 * epl
            lp, g = e.logp_grad(theta)
            e.close()
            ref = hw.case(model, *reference_args(c), theta, epl, o, w, group)
            ratio = hw.error_ratio(lp, g, ref)
            print(f"model {model} geometry {geometry} fma {fma} N {N} {combo}: error / bound = {ratio:.3f}")
            assert ratio <= 1.0, (N, combo, ratio)
            worst = max(worst, ratio)
            assert hw.sensitivity(model, *reference_args(c), theta, ref, o, w, group) >= 100.0, (N, combo)
    return worst


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", MODELS, ids=IDS)
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("fma", [0, 1])
def test_against_high_precision(sim, model, geometry, fma, record_property):
    record_property("max_error_over_bound", check_edge_matrix(sim, model, geometry, fma))


# ---- trailing zero weights are truncation ---------------------------------------------------------------------------

@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [LOG, POIS, NB, HLOG], ids=["logistic", "poisson", "negbin", "hier_logistic"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_trailing_zero_weights_equal_truncation(sim, model, geometry):
    epl = geometry[1]
    B = hp.block_rows(epl)
    for m in (B, B + 1):
        N = m + B + 1  # the zero-weight rows end a block, fill one and begin another
        c = make_case(model, COLUMNS[epl], N, seed=7 * m + model)
        w = c["weights"].copy()
        w[m:] = 0.0
        o = c["offset"].copy()
        if model == POIS:
            o[m] = 800.0  # eta > 710: exp overflows on a row that must not count
        short = dict(c, data=tuple(a[:m] for a in c["data"]))
        full = engine(sim, model, c, 3, geometry, 1, offset=o, weights=w)
        cut = engine(sim, model, short, 3, geometry, 1, offset=o[:m], weights=w[:m])
        theta = thetas(model, c["D"], 3, seed=m)
        a, b = full.logp_grad(theta), cut.logp_grad(theta)
        assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1]))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), m
        for u, v in zip(drive(full, 0), drive(cut, 0)):
            for key in v:
                assert np.array_equal(u[key], v[key], equal_nan=True), (m, key)
        assert np.all(np.isfinite(full.logp()))


# ---- weight sets ----------------------------------------------------------------------------------------------------

def fold_weights(W, N, rng):
    """W weight vectors: 0/1 folds scaled by a weight per row, no two alike"""
    base = rng.uniform(0.5, 2.0, size=N)
    sets = np.stack([base * (np.arange(N) % W != g) for g in range(W)])
    sets[0, 0] = 2.5
    return sets


@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", [LOG, NB], ids=["logistic", "negbin"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("fma", [0, 1])
def test_weight_sets_equal_standalone_engines(sim, model, geometry, fma):
    epl = geometry[1]
    W, k = 3, 2
    N = 2 * hp.block_rows(epl) + 3
    c = make_case(model, COLUMNS[epl], N, seed=50 + epl)
    sets = fold_weights(W, N, np.random.default_rng(3))
    e = engine(sim, model, c, W * k, geometry, fma, offset=c["offset"], weight_sets=sets)
    assert e.num_datasets == W and e.lanes == 64
    batched = drive(e, 0)
    for g in range(W):
        alone = engine(sim, model, c, k, geometry, fma, offset=c["offset"], weights=sets[g])
        assert alone.num_datasets == 1
        compare_blocks(batched, drive(alone, g * k), g, k)
        alone.close()
    assert not np.array_equal(batched[-1]["pos"][:k], batched[-1]["pos"][k:2 * k])
    e.close()


@pytest.mark.timeout(900)
def test_one_weight_set_is_one_weight_vector(sim):
    c = make_case(LOG, 5, 9, seed=2)
    runs = []
    for kw in (dict(weight_sets=c["weights"][None, :]), dict(weights=c["weights"])):
        e = engine(sim, LOG, c, 4, (1, 2), 1, **kw)
        assert e.num_datasets == 1
        runs.append(drive(e, 0, average=True))  # (mass averaging takes the pooled path: the engine holds no datasets)
    for a, b in zip(*runs):
        for key in a:
            assert np.array_equal(a[key], b[key], equal_nan=True), key
    res = drop_in(sim, LOG, c["D"], c["params"], 4, data=c["data"], weight_sets=c["weights"][None, :],
                  keep_on_device=True, min_warmup_iter=3, max_warmup_iter=3, min_sampling_iter=3, max_sampling_iter=3)
    assert res[1].num_chains() == 4  # one MarkovChains, not a list of views


@pytest.mark.timeout(1800)
def test_monitors_per_weight_set(sim):
    model, k, W, N = LOG, 3, 3, 21
    c = make_case(model, 5, N, seed=31)
    sets = fold_weights(W, N, np.random.default_rng(5))
    sets[1] *= 6.0  # (a set that adapts differently)
    geometry = (1, 2)
    e = engine(sim, model, c, W * k, geometry, 1, weight_sets=sets)
    alone = [engine(sim, model, c, k, geometry, 1, weights=sets[g]) for g in range(W)]
    engines = [(e, 0)] + [(a, g * k) for g, a in enumerate(alone)]
    for eng, off in engines:
        eng.init_positions(seed=4, chain_offset=off, scale=0.5)
        eng.init_masses_from_grad(1e-5, average=True)
        eng.adapt_step(seed=5, chain_offset=off)
        eng.seed_chains(6, off)
        eng.warmup_steps(4)
    m = e.masses()
    step, mass = e.warmup_spread_per_dataset()
    for g, a in enumerate(alone):
        assert np.array_equal(m[g * k:(g + 1) * k], a.masses()), g
        assert (step[g], mass[g]) == a.warmup_spread(), g
    assert len(set(step.tolist())) == W
    for eng, _ in engines:
        eng.freeze()
        eng.sample_steps(6)
    r = e.rhat_per_dataset()
    for g, a in enumerate(alone):
        assert r[g] == a.rhat(), g
    with pytest.raises(ValueError, match="holds no datasets"):
        alone[0].rhat_per_dataset()


@pytest.mark.timeout(1800)
def test_drop_in_call_per_weight_set(sim):
    model, k, W, N = LOG, 2, 3, 19
    c = make_case(model, 5, N, seed=41)
    D, s2, d = c["D"], c["params"], c["data"]
    sets = fold_weights(W, N, np.random.default_rng(6))
    fixed = dict(min_warmup_iter=7, max_warmup_iter=7, min_sampling_iter=6, max_sampling_iter=6, data=d,
                 offset=c["offset"])
    mixed = flat(drop_in(sim, model, D, s2, W * k, weight_sets=sets, **fixed))
    for g in range(W):
        # the standalone call with the same chain ids: every set equal to set g, which is the call with weights=sets[g]
        same = flat(drop_in(sim, model, D, s2, W * k, weights=sets[g], **fixed))
        again = flat(drop_in(sim, model, D, s2, W * k, weight_sets=np.stack([sets[g]] * W), **fixed))
        for u, v, t in zip(mixed, same, again):
            assert np.array_equal(u[g * k:(g + 1) * k], v[g * k:(g + 1) * k]), g
            assert np.array_equal(v, t), g
    assert not np.array_equal(mixed[0][:k], mixed[0][k:2 * k])
    res, views = drop_in(sim, model, D, s2, W * k, weight_sets=sets, keep_on_device=True, thin=1, **fixed)
    assert len(views) == W
    for g, v in enumerate(views):
        assert v.num_chains() == k and v.dims() == D
        block = mixed[0][g * k:(g + 1) * k]
        assert np.allclose(v.mean(), block.reshape(-1, D).mean(axis=0), rtol=1e-12, atol=1e-12)
        assert np.all(np.isfinite(v.r_hat()))


# ---- semantics ------------------------------------------------------------------------------------------------------

@pytest.mark.timeout(900)
@pytest.mark.parametrize("model", [LOG, NB, HLOG], ids=["logistic", "negbin", "hier_logistic"])
def test_integer_weights_are_repeated_rows(sim, model):
    geometry, N = (1, 2), 11
    c = make_case(model, 5, N, seed=3)
    w = np.random.default_rng(1).integers(0, 4, size=N).astype(np.float64)
    w[0] = 2.0
    rows = np.repeat(np.arange(N), w.astype(int))
    repeated = tuple(a[rows] for a in c["data"])
    theta = thetas(model, c["D"], 2, seed=2)
    lp, g = engine(sim, model, c, 2, geometry, 1, offset=c["offset"], weights=w).logp_grad(theta)
    group = c["data"][2] if model == HLOG else None
    _, _, blp, bg = hw.case(model, *reference_args(c), theta, 2, c["offset"], w, group)
    lp_rep, g_rep, _, _ = hw.reference(model, repeated[0], repeated[1], c["params"], theta, c["offset"][rows], None,
                                       None if group is None else repeated[2])
    assert hw.error_ratio(lp, g, (lp_rep, g_rep, blp, bg)) <= 1.0
    # ... and the engine on the physically repeated rows agrees to within both bounds
    lp2, g2 = engine(sim, model, dict(c, data=repeated), 2, geometry, 1, offset=c["offset"][rows]).logp_grad(theta)
    _, _, blp2, bg2 = hw.case(model, repeated[0], repeated[1], c["params"], theta, 2, c["offset"][rows], None,
                              None if group is None else repeated[2])
    assert np.all(np.abs(lp - lp2) <= blp + blp2) and np.all(np.abs(g - g2) <= bg + bg2)


@pytest.mark.timeout(900)
def test_binomial_counts_through_weights(sim):
    N, P, epl = 13, 5, 2
    rng = np.random.default_rng(12)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    trials = rng.integers(1, 30, size=N).astype(np.float64)
    succ = rng.binomial(trials.astype(int), 1 / (1 + np.exp(-(x @ rng.normal(size=P))))).astype(np.float64)
    succ[0], succ[1] = 0.0, trials[1]
    s2 = rng.uniform(0.5, 4.0, size=P)
    yfrac = succ / trials
    theta = rng.normal(size=(2, P)) * 0.5
    e = wa.DeviceEngine(LOG, P, 2, config(sim, (1, epl), 1), params=s2, lib_path=sim, data=(x, yfrac), weights=trials)
    lp, g = e.logp_grad(theta)
    _, _, blp, bg = hw.case(LOG, x, yfrac, s2, theta, epl, None, trials)
    lp_ref, g_ref = np.empty(2), np.empty((2, P))
    with mp.workdps(60):  # the binomial log-likelihood up to log C(m, k): k eta - m softplus(eta)
        m = lambda v: mp.mpf(float(v))  # noqa: E731
        for c in range(2):
            eta = [mp.fsum(m(x[n, j]) * m(theta[c, j]) for j in range(P)) for n in range(N)]
            ll = mp.fsum(m(succ[n]) * eta[n] - m(trials[n]) * mp.log1p(mp.exp(eta[n])) for n in range(N))
            lp_ref[c] = float(ll - mp.fsum(m(theta[c, j]) ** 2 / (2 * m(s2[j])) for j in range(P)))
            r = [m(succ[n]) - m(trials[n]) / (1 + mp.exp(-eta[n])) for n in range(N)]
            g_ref[c] = [float(mp.fsum(m(x[n, j]) * r[n] for n in range(N)) - m(theta[c, j]) / m(s2[j])) for j in range(P)]
    assert hw.error_ratio(lp, g, (lp_ref, g_ref, blp, bg)) <= 1.0


@pytest.mark.timeout(900)
@pytest.mark.parametrize("model", [LIN, LOG, POIS], ids=["linear", "logistic", "poisson"])
def test_all_zero_weights_leave_the_prior(sim, model):
    geometry, N = (1, 2), 19
    c = make_case(model, 5, N, seed=9)
    theta = thetas(model, c["D"], 3, seed=4)
    lp, g = engine(sim, model, c, 3, geometry, 1, offset=c["offset"], weights=np.zeros(N)).logp_grad(theta)
    # the prior alone, from the same kernel: linear regression on one row x = 0, y = 0 (r = 0, term -0.5 * 0 * 0)
    zero = dict(c, data=(np.zeros((1, 5)), np.zeros(1)))
    lp0, g0 = engine(sim, LIN, zero, 3, geometry, 1).logp_grad(theta)
    assert np.array_equal(lp, lp0) and np.array_equal(g, g0)
    assert np.array_equal(g, -theta * (1.0 / c["params"]))


# ---- with datasets= -------------------------------------------------------------------------------------------------

@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [POIS, HLOG], ids=["poisson", "hier_logistic"])
def test_datasets_with_their_own_offsets_and_weights(sim, model):
    geometry, k = (1, 2), 2
    cases = [make_case(model, 5, n, seed=60 + n) for n in (17, 1, 20)]
    D, params = cases[0]["D"], cases[0]["params"]
    offsets = [cases[0]["offset"], None, cases[2]["offset"]]
    weights = [None, cases[1]["weights"], cases[2]["weights"]]
    e = wa.DeviceEngine(model, D, 3 * k, config(sim, geometry, 1), params=params, lib_path=sim,
                        datasets=[c["data"] for c in cases], offset=offsets, weights=weights)
    assert e.num_datasets == 3
    batched = drive(e, 0)
    for g, c in enumerate(cases):
        # (a None entry is offset 0 / weight 1 on an engine that carries the field: the weighted order with w = 1)
        alone = wa.DeviceEngine(model, D, k, config(sim, geometry, 1), params=params, lib_path=sim, data=c["data"],
                                offset=offsets[g], weights=np.ones(len(c["offset"])) if weights[g] is None else weights[g])
        compare_blocks(batched, drive(alone, g * k), g, k)
    # a missing entry is offset 0 / weight 1: dataset 1 without its weights is another engine
    plain = wa.DeviceEngine(model, D, k, config(sim, geometry, 1), params=params, lib_path=sim, data=cases[1]["data"])
    assert not np.array_equal(drive(plain, k)[-1]["pos"], batched[-1]["pos"][k:2 * k])


# ---- refusals -------------------------------------------------------------------------------------------------------

@pytest.mark.timeout(600)
def test_refusals(sim):
    D, N = 5, 20
    c = make_case(LOG, D, N, seed=1)
    x, y = c["data"]
    s2 = c["params"]
    cfg = wa.default_config(sim)
    lib = wa._ffi.load_library(sim)
    dp = wa._ffi._dp

    def create(model, chains, offset=None, weight=None, sets=0, offsets=None, G=0, ys=y):
        h, err = C.c_void_p(), C.c_void_p()
        keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, ys)]
        obs = wa._ffi.Observations(x=keep[0].ctypes.data_as(dp), y=keep[1].ctypes.data_as(dp), num_obs=N,
                                   num_weight_sets=sets)
        if offset is not None:
            keep.append(np.ascontiguousarray(offset, dtype=np.float64))
            obs.offset = keep[-1].ctypes.data_as(dp)
        if weight is not None:
            keep.append(np.ascontiguousarray(weight, dtype=np.float64))
            obs.weight = keep[-1].ctypes.data_as(dp)
        if offsets is not None:
            keep.append(np.ascontiguousarray(offsets, dtype=np.int64))
            obs.obs_offsets, obs.num_datasets = keep[-1].ctypes.data_as(wa._ffi._i64p), G
        rc = lib.wn_engine_create_observed(C.byref(h), model, D, s2.ctypes.data_as(dp), C.byref(obs), chains,
                                           C.byref(cfg), C.byref(err))
        if rc == 0:
            lib.wn_engine_destroy(h)
            return None
        msg = lib.walnutpie_get_error_message(err).decode()
        kind = lib.walnutpie_get_error_type(err)
        lib.walnutpie_destroy_error(err)
        return kind, msg

    config_error = 1
    w = np.ones(N)
    neg, inf, nan_o = w.copy(), w.copy(), np.zeros(N)
    neg[3], inf[4], nan_o[5] = -0.5, np.inf, np.nan
    sets = np.ones((2, N))
    bad_set = sets.copy()
    bad_set[1, 7] = np.nan
    cases = [
        (dict(model=LOG, chains=2, weight=neg), "every weight must be finite and >= 0, observation 3 has -0.500000"),
        (dict(model=LOG, chains=2, weight=inf), "every weight must be finite and >= 0, observation 4 has inf"),
        (dict(model=LOG, chains=2, weight=bad_set, sets=2),
         "every weight must be finite and >= 0, observation 7 of weight set 1 has nan"),
        (dict(model=LOG, chains=2, offset=nan_o), "every offset must be finite, observation 5 has nan"),
        (dict(model=LOG, chains=2, weight=sets, sets=2, offsets=[0, 10, 20], G=2),
         "weight sets share one block of rows: not with obs_offsets (several datasets)"),
        (dict(model=LOG, chains=3, weight=sets, sets=2),
         "num_chains must be a multiple of num_weight_sets (chain c reads weight set c / (num_chains / num_weight_sets))"),
        (dict(model=LOG, chains=2, weight=w, sets=-1), "num_weight_sets must not be negative"),
        (dict(model=LOG, chains=2, sets=2), "num_weight_sets > 1 needs weight [num_weight_sets][num_obs]"),
    ]
    for kw, msg in cases:
        assert create(**kw) == (config_error, msg), msg
    assert create(model=LOG, chains=2, weight=np.zeros(N)) is None  # an all-zero vector: the prior is proper
    assert create(model=LOG, chains=2, weight=w, sets=1) is None and create(model=LOG, chains=2, weight=w, sets=0) is None
    # logistic y: a proportion only on an engine with weights; the unweighted message is unchanged
    yfrac = y.copy()
    yfrac[2] = 0.25
    assert create(model=LOG, chains=2, ys=yfrac) == (config_error, "logistic_regression needs every y in {0, 1}")
    assert create(model=LOG, chains=2, ys=yfrac, offset=np.zeros(N)) == (config_error,
                                                                        "logistic_regression needs every y in {0, 1}")
    assert create(model=LOG, chains=2, ys=yfrac, weight=w) is None
    yfrac[2] = 1.25
    kind, msg = create(model=LOG, chains=2, ys=yfrac, weight=w)
    assert kind == config_error and msg.startswith("logistic_regression with weights needs every y in [0, 1]"), msg
    # Python shape errors
    common = dict(params=s2, lib_path=sim)
    with pytest.raises(ValueError, match=r"offset must have shape \(20,\), got \(19,\)"):
        wa.DeviceEngine(LOG, D, 2, cfg, data=(x, y), offset=np.zeros(19), **common)
    with pytest.raises(ValueError, match=r"weights must have shape \(20,\), got \(2, 20\)"):
        wa.DeviceEngine(LOG, D, 2, cfg, data=(x, y), weights=sets, **common)
    with pytest.raises(ValueError, match=r"weight_sets must have shape \(W, 20\), got \(20,\)"):
        wa.DeviceEngine(LOG, D, 2, cfg, data=(x, y), weight_sets=w, **common)
    with pytest.raises(ValueError, match="weight_sets is available with data only"):
        wa.DeviceEngine(LOG, D, 2, cfg, datasets=[(x, y)], weight_sets=sets, **common)
    with pytest.raises(ValueError, match="weights and weight_sets are mutually exclusive"):
        wa.DeviceEngine(LOG, D, 2, cfg, data=(x, y), weights=w, weight_sets=sets, **common)
    with pytest.raises(ValueError, match="offset, weights and weight_sets need data or datasets"):
        wa.DeviceEngine(wa.MODEL_STD_NORMAL, D, 2, cfg, lib_path=sim, weights=w)
    with pytest.raises(ValueError, match=r"weights must have one entry per dataset \(2\), got 1"):
        wa.DeviceEngine(LOG, D, 2, cfg, datasets=[(x, y), (x, y)], weights=[w], **common)
    with pytest.raises(ValueError, match=r"offset of dataset 1 must have shape \(20,\), got \(3,\)"):
        wa.DeviceEngine(LOG, D, 2, cfg, datasets=[(x, y), (x, y)], offset=[None, np.zeros(3)], **common)
    with pytest.raises(ValueError, match="num_chains must be a multiple of num_weight_sets"):
        wa.walnuts_device(LOG, model_params=s2, num_params=D, num_chains=3, data=(x, y), weight_sets=sets, lib_path=sim,
                          min_warmup_iter=2, max_warmup_iter=2, min_sampling_iter=2, max_sampling_iter=2)


# ---- a model compiled at run time -----------------------------------------------------------------------------------

@pytest.mark.timeout(1800)
def test_runtime_compiled_copy_of_the_glm_header_with_row_terms(sim, tmp_path):
    gxx = ["g++", "-x", "c++", "-std=c++20", "-O1", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden", "-pthread",
           "-DWN_CPU_SIM", "-I", os.path.join(HERE, "cpusim")]
    header = os.path.join(os.path.dirname(HERE), "walnuts_amd", "csrc", "models", "glm.h")
    c = make_case(POIS, 150, 21, seed=12)
    so = models.build_device_model(header, "wn::PoissonRegressionModel", "user_poisson_rows", 10, c["D"],
                                   out_dir=str(tmp_path), lib_path=sim, compiler=gxx)
    mid = models.load_device_model(so, "user_poisson_rows", lib_path=sim)
    assert mid == 10
    sets = fold_weights(2, 21, np.random.default_rng(2))
    runs = [drive(engine(sim, m, c, 4, (1, 4), 1, offset=c["offset"], weight_sets=sets), 0) for m in (POIS, mid)]
    for a, b in zip(*runs):
        for key in a:
            assert np.array_equal(a[key], b[key], equal_nan=True), key
