"""CPU tier: many datasets of one data model in one engine (wn_engine_create_observed with obs_offsets,
DeviceEngine(datasets=...), walnutpie_sample_device_observed*, walnuts_device(datasets=...)) under the workgroup emulation.

The contract checked here: chain c of dataset g = c // k evolves bit for bit as chain c - g*k of a standalone engine
built from dataset g alone and seeded with chain_offset = g*k; the per-dataset statistics equal the standalone engines'
pooled ones; identical datasets give the shared-data engine; the drop-in call stops per dataset in lock step."""
import math
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
from walnuts_amd import models  # noqa: E402
from test_data_models_sim import LIN, LOG, make_data  # noqa: E402

SIM_GEOMETRIES = ((1, 2), (1, 4), (1, 8), (1, 16))
DIM = {2: 7, 4: 150, 8: 300, 16: 300}  # one wavefront per chain, with padding


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def dataset_sizes(epl, k_index):
    """Ragged observation counts around the geometry's row block B: 1, B, B + 1 and an odd count, rotated per case."""
    B = hp.block_rows(epl)
    sizes = [1, B, B + 1, 2 * B + 3]
    return [sizes[(k_index + i) % 4] for i in range(3)]


def make_datasets(model, D, sizes, seed):
    out = []
    for g, n in enumerate(sizes):
        x, y, _ = make_data(model, D, n, seed=seed + 17 * g)
        if g == 1:
            y = 1.0 - y if model == LOG else -y  # (a dataset far from its neighbours: misrouting changes everything)
        out.append((x, y))
    s2 = np.random.default_rng(seed).uniform(0.5, 4.0, size=D)
    return out, s2


def config(lib, geometry, fma, **kw):
    return wa.default_config(lib, fused_multiply_add=fma, waves_per_chain=geometry[0], elems_per_lane=geometry[1], **kw)


def state(e):
    est = e.estimator()
    return dict(pos=e.positions(), logp=e.logp(), depth=e.depths(), grads=e.grad_evals(), rng=e.rng_draws(),
                failed=e.failed_extensions(), steps=e.step_sizes(), adam=e.adam(), inv_mass=e.inv_mass(),
                masses=e.masses(), **est)


def drive(e, offset, seed=11, average=False):
    """init, masses from the gradient, adapt_step, single and fused warmup steps, freeze, sample_steps(8)."""
    snaps = []
    e.init_positions(seed=seed, chain_offset=offset, scale=0.5)
    e.init_masses_from_grad(1e-5, average=average)
    snaps.append(dict(masses=e.masses()))
    e.adapt_step(seed=seed + 1, chain_offset=offset)
    e.seed_chains(seed + 2, offset)
    e.warmup_step()
    e.warmup_steps(3)
    snaps.append(state(e))
    e.freeze()
    e.sample_steps(8)
    e.check()
    s = state(e)
    s.pop("masses")
    snaps.append(s)
    return snaps


def compare_blocks(batched, standalone, g, k):
    for a, b in zip(batched, standalone):
        for key in b:
            blk = a[key][g * k:(g + 1) * k]
            assert np.array_equal(blk, b[key], equal_nan=True), (g, key)


@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", [LIN, LOG])
@pytest.mark.parametrize("geometry", SIM_GEOMETRIES)
@pytest.mark.parametrize("fma", [0, 1])
def test_equals_standalone_engines(sim, model, geometry, fma):
    epl = geometry[1]
    D = DIM[epl]
    for ki, k in enumerate((1, 2, 5)):
        datasets, s2 = make_datasets(model, D, dataset_sizes(epl, ki), seed=100 + ki)
        cfg = config(sim, geometry, fma)
        e = wa.DeviceEngine(model, D, 3 * k, cfg, params=s2, lib_path=sim, datasets=datasets)
        assert e.num_datasets == 3 and e.lanes == 64
        batched = drive(e, 0)
        for g, d in enumerate(datasets):
            alone = wa.DeviceEngine(model, D, k, cfg, params=s2, lib_path=sim, data=d)
            compare_blocks(batched, drive(alone, g * k), g, k)
            alone.close()
        e.close()


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [LIN, LOG])
def test_identical_datasets_equal_the_shared_data_engine(sim, model):
    D = 7
    x, y, s2 = make_data(model, D, 19, seed=3)
    cfg = config(sim, (1, 2), 1)
    batched = drive(wa.DeviceEngine(model, D, 6, cfg, params=s2, lib_path=sim, datasets=[(x, y)] * 3), 0)
    shared = drive(wa.DeviceEngine(model, D, 6, cfg, params=s2, lib_path=sim, data=(x, y)), 0)
    for a, b in zip(batched, shared):
        for key in b:
            assert np.array_equal(a[key], b[key], equal_nan=True), key


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [LIN, LOG])
@pytest.mark.parametrize("geometry", SIM_GEOMETRIES)
def test_logp_grad_against_high_precision(sim, model, geometry):
    epl = geometry[1]
    D = DIM[epl]
    k = 2
    datasets, s2 = make_datasets(model, D, dataset_sizes(epl, 1), seed=7)
    e = wa.DeviceEngine(model, D, 3 * k, config(sim, geometry, 1), params=s2, lib_path=sim, datasets=datasets)
    theta = np.random.default_rng(5).normal(size=(3 * k, D)) * 0.3
    lp, g = e.logp_grad(theta)
    for ds, (x, y) in enumerate(datasets):
        rows = slice(ds * k, (ds + 1) * k)
        assert hp.error_ratio(lp[rows], g[rows], hp.glm_case(model, x, y, s2, theta[rows], epl)) <= 1.0, ds
        xn, yn = datasets[(ds + 1) % 3]  # the neighbouring dataset's reference is far outside the bound
        assert hp.error_ratio(lp[rows], g[rows], hp.glm_case(model, xn, yn, s2, theta[rows], epl)) >= 100.0, ds


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("k", [3, 7])
def test_statistics_per_dataset(sim, k):
    check_statistics_per_dataset(sim, k)


def check_statistics_per_dataset(sim, k):
    """rhat_per_dataset, warmup_spread_per_dataset and per-dataset mass averaging equal the standalone engines'; the
    pooled statistics are their two stages composed; at G = 1 the per-dataset statistics are the pooled ones."""
    model, D = LOG, 7
    datasets, s2 = make_datasets(model, D, [5, 1, 12], seed=31)
    cfg = config(sim, (1, 2), 1)
    e = wa.DeviceEngine(model, D, 3 * k, cfg, params=s2, lib_path=sim, datasets=datasets)
    alone = [wa.DeviceEngine(model, D, k, cfg, params=s2, lib_path=sim, data=d) for d in datasets]
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
        s_ref, m_ref = a.warmup_spread()
        assert step[g] == s_ref and mass[g] == m_ref, g
    assert len(set(step.tolist())) == 3  # (the datasets' values differ: nothing is pooled)
    assert_pooled_spread_is_its_stages(e)
    for eng, _ in engines:
        eng.freeze()
        eng.sample_steps(6)
    r = e.rhat_per_dataset()
    for g, a in enumerate(alone):
        assert r[g] == a.rhat(), g
    # the pooled statistics keep their meaning on a batched engine
    pooled = wa.DeviceEngine(model, D, 3 * k, cfg, params=s2, lib_path=sim, data=datasets[0])
    assert pooled.num_datasets == 1
    with pytest.raises(ValueError, match="holds no datasets"):
        pooled.rhat_per_dataset()
    assert np.isfinite(e.rhat())
    assert_pooled_rhat_is_its_stages(e)
    check_one_dataset(sim, model, D, k, cfg, s2, datasets[1])


def assert_pooled_spread_is_its_stages(e):
    """warmup_spread() is warmup_sums -> warmup_max_rel over all of the engine's chains."""
    s, col = e.warmup_sums()
    assert e.warmup_spread() == e.warmup_max_rel(s, col, e.C)


def assert_pooled_rhat_is_its_stages(e):
    """rhat() is lp_sums -> lp_sq_dev(mean of means) -> sqrt(1 + variance of means / mean of variances)."""
    s0, s1, n = e.lp_sums()
    q = e.lp_sq_dev(s0 / n)
    assert e.rhat() == math.sqrt(1 + (q / (n - 1)) / (s1 / n))


def check_one_dataset(lib, model, D, k, cfg, s2, d):
    """An engine built with datasets=[d] (G = 1): the per-dataset statistics and mass averaging are the pooled ones."""
    pair = [wa.DeviceEngine(model, D, k, cfg, params=s2, lib_path=lib, datasets=[d]) for _ in range(2)]
    for u, fn in zip(pair, ("wn_engine_average_masses", "wn_engine_average_masses_datasets")):
        assert u.num_datasets == 1
        u.init_positions(seed=4, chain_offset=0, scale=0.5)
        u.init_masses_from_grad(1e-5)
        u._call(getattr(u.lib, fn))
    m = pair[0].masses()
    assert np.array_equal(m, pair[1].masses())
    assert np.all(m == m[0]) and not np.all(m == 1.0)
    u = pair[0]
    u.adapt_step(seed=5)
    u.seed_chains(6)
    u.warmup_steps(4)
    step, mass = u.warmup_spread_per_dataset()
    assert (step[0], mass[0]) == u.warmup_spread()
    assert_pooled_spread_is_its_stages(u)
    u.freeze()
    u.sample_steps(6)
    assert np.isfinite(u.rhat())
    assert u.rhat_per_dataset()[0] == u.rhat()
    assert_pooled_rhat_is_its_stages(u)
    for u in pair:
        u.close()


DROP_IN = dict(seed=9, id=2, init_radius=0.5, max_trajectory_doublings=4)


def drop_in(sim, model, D, s2, num_chains, **kw):
    args = dict(model_params=s2, num_params=D, num_chains=num_chains, lib_path=sim, save_inv_metric=True, **DROP_IN)
    args.update(kw)
    return wa.walnuts_device(model, **args)


def flat(results):
    return (np.array([np.asarray(r) for r in results]), np.array([r.warmup.stepsize for r in results]),
            np.array([r.warmup.inv_metric for r in results]))


@pytest.mark.timeout(1800)
def test_drop_in_call_without_cross_talk(sim):
    model, D, k = LOG, 7, 2
    datasets, s2 = make_datasets(model, D, [9, 2, 16], seed=41)
    fixed = dict(min_warmup_iter=7, max_warmup_iter=7, min_sampling_iter=6, max_sampling_iter=6)
    # all datasets equal to d: the shared-data call on d
    d = datasets[0]
    a = flat(drop_in(sim, model, D, s2, 3 * k, datasets=[d] * 3, **fixed))
    b = flat(drop_in(sim, model, D, s2, 3 * k, data=d, **fixed))
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    # block g of distinct datasets: block g of the call whose datasets are all copies of dataset g
    mixed = flat(drop_in(sim, model, D, s2, 3 * k, datasets=datasets, **fixed))
    for g, dg in enumerate(datasets):
        same = flat(drop_in(sim, model, D, s2, 3 * k, datasets=[dg] * 3, **fixed))
        for u, v in zip(mixed, same):
            assert np.array_equal(u[g * k:(g + 1) * k], v[g * k:(g + 1) * k]), g
    assert not np.array_equal(mixed[0][:k], mixed[0][k:2 * k])
    # the resident call: one MarkovChains view per dataset, over the same draws
    res, views = drop_in(sim, model, D, s2, 3 * k, datasets=datasets, keep_on_device=True, thin=1, **fixed)
    assert len(views) == 3
    for g, v in enumerate(views):
        assert v.num_chains() == k and v.dims() == D
        block = mixed[0][g * k:(g + 1) * k]
        assert np.allclose(v.mean(), block.reshape(-1, D).mean(axis=0), rtol=1e-12, atol=1e-12)
    del res
    views[0].close()
    assert np.all(np.isfinite(views[2].mean()))  # (the block outlives the first view)


def replay(sim, model, D, s2, datasets, k, a):
    """The drop-in call's controller rules, replayed through the engine API: warmup looks every 5 iterations from
    min_warmup_iter, sampling R-hat looks every 5 from min_sampling_iter, every dataset has to pass."""
    C = len(datasets) * k
    cfg = wa.default_config(sim, max_trajectory_doublings=a["max_trajectory_doublings"])
    e = wa.DeviceEngine(model, D, C, cfg, params=s2, lib_path=sim, datasets=datasets)
    e.init_positions(seed=a["seed"], chain_offset=0, scale=a["init_radius"])
    e.init_masses_from_grad(1e-5)
    e.set_step_sizes(1.0)
    e.adapt_step(seed=a["seed"], chain_offset=0)
    e.seed_chains(a["seed"] + a["id"] + C, 0)
    warm, first_ok = 0, {}
    while warm < a["max_warmup_iter"]:
        e.warmup_step()
        warm += 1
        if warm >= a["min_warmup_iter"] and warm < a["max_warmup_iter"] and warm % 5 == 0:
            step, mass = e.warmup_spread_per_dataset()
            ok = (mass <= a["mass_converge_tol"]) & (step <= a["step_size_converge_tol"])
            for g in np.flatnonzero(ok):
                first_ok.setdefault(int(g), warm)
            if ok.all():
                break
    e.freeze()
    samp = 0
    while samp < a["max_sampling_iter"]:
        e.sample_step()
        samp += 1
        if (samp >= a["min_sampling_iter"] and samp >= 2 and samp < a["max_sampling_iter"] and k > 1
                and (samp - a["min_sampling_iter"]) % 5 == 0):
            r = e.rhat_per_dataset()
            for g in np.flatnonzero(r <= a["rhat_converge_tol"]):
                first_ok.setdefault(("rhat", int(g)), samp)
            if np.all(r <= a["rhat_converge_tol"]):
                break
    return warm, samp, first_ok


@pytest.mark.timeout(3600)
def test_adaptive_stopping_per_dataset(sim):
    model, D, k = LIN, 3, 4
    rng = np.random.default_rng(8)
    datasets = []
    for n, scale in ((40, 1.0), (40, 1.0), (3, 10.0)):  # the last one: three rows, large |x|: it adapts differently
        x = rng.normal(size=(n, D)) * scale
        datasets.append((x, x @ rng.normal(size=D) + rng.normal(size=n)))
    s2 = np.full(D, 100.0)
    a = dict(DROP_IN, min_warmup_iter=5, max_warmup_iter=60, min_sampling_iter=5, max_sampling_iter=60,
             step_size_converge_tol=0.5, mass_converge_tol=2.0, rhat_converge_tol=1.2)
    warm, samp, first_ok = replay(sim, model, D, s2, datasets, k, a)
    res = drop_in(sim, model, D, s2, 3 * k, datasets=datasets, save_warmup=True,
                  **{key: v for key, v in a.items() if key not in DROP_IN})
    lengths_warm = [r.warmup.warmup_draws.shape[0] for r in res]
    lengths_samp = [np.asarray(r).shape[0] for r in res]
    assert lengths_warm == [warm] * (3 * k) and lengths_samp == [samp] * (3 * k), (warm, samp, first_ok)
    # both phases stopped early, and warmup went on past a look that some datasets had already passed
    assert warm < a["max_warmup_iter"] and samp < a["max_sampling_iter"], (warm, samp, first_ok)
    assert min(first_ok[g] for g in range(3)) < warm, first_ok


@pytest.mark.timeout(600)
def test_refusals(sim):
    D = 5
    x, y, s2 = make_data(LOG, D, 20, seed=1)
    cfg = wa.default_config(sim)
    lib = wa._ffi.load_library(sim)
    import ctypes as C

    def create(model, xs, ys, offsets, G, chains, params=s2):
        h, err = C.c_void_p(), C.c_void_p()
        xs, ys = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(ys, dtype=np.float64)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        obs = wa._ffi.Observations(x=xs.ctypes.data_as(wa._ffi._dp), y=ys.ctypes.data_as(wa._ffi._dp),
                                   obs_offsets=off.ctypes.data_as(wa._ffi._i64p), num_datasets=G)
        rc = lib.wn_engine_create_observed(C.byref(h), model, D, None if params is None else params.ctypes.data_as(wa._ffi._dp),
                                           C.byref(obs), chains, C.byref(cfg), C.byref(err))
        if rc == 0:
            lib.wn_engine_destroy(h)
            return None
        msg = lib.walnutpie_get_error_message(err).decode()
        kind = lib.walnutpie_get_error_type(err)
        lib.walnutpie_destroy_error(err)
        return kind, msg

    config_error = 1  # WalnutpyErrorType: config
    cases = [
        ((LOG, x, y, [0, 20], 0, 2), "num_datasets must be positive"),
        ((LOG, x, y, [0, 10, 20], 2, 3),
         "num_chains must be a multiple of num_datasets (chain c reads dataset c / (num_chains / num_datasets))"),
        ((LOG, x, y, [1, 10, 20], 2, 2), "obs_offsets must start at 0"),
        ((LOG, x, y, [0, 10, 10], 2, 2),
         "obs_offsets must be strictly increasing (every dataset needs at least one observation)"),
        ((LOG, x, y, [0, 12, 10], 2, 2),
         "obs_offsets must be strictly increasing (every dataset needs at least one observation)"),
        ((wa.MODEL_STD_NORMAL, x, y, [0, 10, 20], 2, 2),
         "std_normal model reads no data (it does not declare kUsesData)"),
    ]
    xb = x.copy()
    xb[13, 1] = np.inf
    cases.append(((LOG, xb, y, [0, 10, 20], 2, 2), "data x must be finite"))
    yb = y.copy()
    yb[19] = np.nan
    cases.append(((LIN, x, yb, [0, 10, 20], 2, 2), "data y must be finite"))
    y2 = y.copy()
    y2[14] = 0.5
    for args, msg in cases:
        assert create(*args) == (config_error, msg), msg
    kind, msg = create(LOG, x, y2, [0, 10, 20], 2, 2)
    assert kind == config_error and msg.startswith("dataset 1: ") and "y in {0, 1}" in msg, msg
    xl = np.zeros((3, 1100))
    with pytest.raises(ValueError, match="num_params <= 1024"):
        wa.DeviceEngine(LIN, 1100, 2, cfg, params=np.ones(1100), lib_path=sim, datasets=[(xl[:1], np.zeros(1)),
                                                                                          (xl[1:], np.zeros(2))])
    with pytest.raises(ValueError, match="mutually exclusive"):
        wa.DeviceEngine(LOG, D, 2, cfg, params=s2, lib_path=sim, data=(x, y), datasets=[(x, y)])
    with pytest.raises(ValueError, match="data and datasets are mutually exclusive"):
        wa.walnuts_device(LOG, model_params=s2, num_params=D, data=(x, y), datasets=[(x, y)], lib_path=sim)
    with pytest.raises(ValueError, match="datasets is not available with devices"):
        wa.walnuts_device(LOG, model_params=s2, num_params=D, datasets=[(x, y)], devices=[0, 0], lib_path=sim)
    with pytest.raises(ValueError, match="datasets is not available with reference_streams"):
        wa.walnuts_device(LOG, model_params=s2, num_params=D, datasets=[(x, y)], reference_streams=True, lib_path=sim)
    with pytest.raises(ValueError, match="num_chains must be a multiple of num_datasets"):
        wa.walnuts_device(LOG, model_params=s2, num_params=D, num_chains=3, datasets=[(x, y)] * 2, lib_path=sim,
                          min_warmup_iter=2, max_warmup_iter=2, min_sampling_iter=2, max_sampling_iter=2)


@pytest.mark.timeout(1800)
def test_runtime_compiled_copy_of_the_glm_header_batched(sim, tmp_path):
    gxx = ["g++", "-x", "c++", "-std=c++20", "-O1", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden", "-pthread",
           "-DWN_CPU_SIM", "-I", os.path.join(HERE, "cpusim")]
    header = os.path.join(os.path.dirname(HERE), "walnuts_amd", "csrc", "models", "glm.h")
    D = 150
    so = models.build_device_model(header, "wn::LogisticRegressionModel", "user_logistic_ds", 14, D,
                                   out_dir=str(tmp_path), lib_path=sim, compiler=gxx)
    mid = models.load_device_model(so, "user_logistic_ds", lib_path=sim)
    datasets, s2 = make_datasets(LOG, D, [3, 9, 17], seed=12)
    cfg = config(sim, (1, 4), 1)
    runs = [drive(wa.DeviceEngine(m, D, 6, cfg, params=s2, lib_path=sim, datasets=datasets), 0) for m in (LOG, mid)]
    for a, b in zip(*runs):
        for key in a:
            assert np.array_equal(a[key], b[key], equal_nan=True), key
