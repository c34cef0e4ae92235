"""CPU tier: simulated replicates and posterior predictive checks through the engine (walnuts_amd/csrc/wn_replicate.h;
wn_engine_replicate, wn_engine_replicate_chains, wn_engine_replicate_check, wa.replicate_draws,
wa.posterior_predictive_check) under the workgroup emulation.

References: the sampler probe fed predict()'s mu and scale (purity: a replicate depends on its key and on the row's mu
and scale alone; the samplers themselves are held to their Python restatement in test_devrand_sim.py), and the check's
reduction replayed in Python floats (tests/helpers/hp_replicate_reference.py).  The device side of the same kernel source
is compared bit for bit in test_replicate_gpu.py."""
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
import hp_math_reference as hm  # noqa: E402
import hp_replicate_reference as hr  # noqa: E402
import hp_weighted_reference as hw  # noqa: E402
import walnuts_amd as wa  # noqa: E402
import wnso  # noqa: E402
from walnuts_amd import _ffi, models  # noqa: E402
from test_pointwise_sim import GEOMETRIES, SMALL, case_for, overflowing_theta, ragged_chains, thetas_for  # noqa: E402
from test_predict_sim import LENGTHS, download  # noqa: E402
from test_weights_sim import config, engine, make_case  # noqa: E402

LOG, POIS, NB, LSIG, HLOG = hw.LOG, hw.POIS, hw.NB, hw.LSIG, hw.HLOG
MODELS = (LOG, POIS, NB, LSIG, HLOG)
IDS = ["logistic", "poisson", "negbin", "linear_sigma", "hier_logistic"]
KIND = {LOG: hr.BERNOULLI, POIS: hr.POISSON, NB: hr.NEGBIN, LSIG: hr.NORMAL, HLOG: hr.BERNOULLI}
SEED = 2 ** 33 + 77
NAMES = ("sum", "sumsq", "min", "max", "zeros", "pearson")


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def rep_case_data(model, epl, N, seed):
    """test_pointwise_sim.case_for with the coefficients of the count models scaled (x times 4, offsets + 1.5) so that
    mu = exp(eta) of one tile straddles 10, the threshold between the two Poisson samplers"""
    c = case_for(model, SMALL[epl], N, seed=seed)
    if model in (POIS, NB):
        c["data"] = (4.0 * c["data"][0],) + tuple(c["data"][1:])
        c["offset"] = c["offset"] + 1.5
    return c


def scales_of(lib, model, theta):
    """the scale each position's family draws with: dexp(s) of the last coordinate (the device's bits, through the maths
    probe), 1 where the family has none"""
    if model in (NB, LSIG):
        return hm.math_probe(_ffi.load_library(lib), hm.EXP, theta[:, -1])
    return np.ones(theta.shape[0])


def probe_rows(lib, model, mu, scale, chain, draw):
    """what the samplers alone give for one draw's rows: mu [N], scale a scalar"""
    return hr.sampler_probe(_ffi.load_library(lib), KIND[model], mu, np.full(mu.shape, scale), SEED, chain, draw, 0, hr.GATHER)[0]


def rep_case(lib, model, geometry, fma, N=65, seed=17):
    """4 ragged chains in W = 2 blocks over shared rows with the mask n % 3 == 0 (test_predict_sim.fold_case's layout):
    predict()'s matrices, the replicate matrix of every chain's draws, both generated blocks downloaded, and the check
    with and without the mask"""
    epl = geometry[1]
    c = rep_case_data(model, epl, N, seed=3 * N + model)
    sets = np.ones((2, N))
    mask = np.tile(np.arange(N) % 3 == 0, (2, 1))
    draws, ch = ragged_chains(model, c["D"], LENGTHS, seed, lib)
    e = engine(lib, model, c, 2, geometry, fma, offset=c["offset"], weight_sets=sets)
    matrices = [e.predict(d) for d in draws]
    rep = [e.replicate(d, SEED) for d in draws]
    gen = []
    for b in range(2):
        g = e.replicate_chains(ch, SEED, block=b)
        gen.append(g)
    host = [a for b in range(2) for a in download(gen[b], max(LENGTHS[2 * b:2 * b + 2]), LENGTHS[2 * b:2 * b + 2])]
    check = e.replicate_check(ch, SEED, mask)
    check_all = e.replicate_check(ch, SEED)
    e.close()
    return dict(c=c, draws=draws, chains=ch, matrices=matrices, rep=rep, gen=gen, host=host, mask=mask, check=check,
                check_all=check_all, model=model, N=N)


def bits(f):
    """everything of a case that the device must reproduce"""
    return f["rep"] + f["host"] + list(f["check"]) + list(f["check_all"])


def check_purity(lib, f):
    """replicate(theta)[t] is the probe under chain t, draw 0, fed predict()'s mu and scale; the chains block is the probe
    under the matching (chain, draw); block b's chains carry their index in the WHOLE chains block"""
    model, N = f["model"], f["N"]
    for c, (theta, (eta, mu, v), rep, gen) in enumerate(zip(f["draws"], f["matrices"], f["rep"], f["host"])):
        scale = scales_of(lib, model, theta)
        assert rep.shape == (len(theta), N) and gen.shape == (len(theta), N)
        for t in range(len(theta)):
            assert hm.same_bits(rep[t], probe_rows(lib, model, mu[t], scale[t], t, 0)), (c, t)
            assert hm.same_bits(gen[t], probe_rows(lib, model, mu[t], scale[t], c, t)), (c, t)
        assert not np.isnan(rep).any() and not np.isnan(gen).any()
    if model in (POIS, NB) and N > 60:
        mu = np.concatenate([m[1] for m in f["matrices"]])
        assert (mu < 10).any(axis=1).all() and (mu >= 10).any(axis=1).all()   # every tile straddles the threshold


def check_reduction(f):
    """all 12 arrays against the Python-float replay on the replicate and predict matrices, exactly; min / max / zeros
    against NumPy's; NaN beyond a chain's length"""
    N = f["N"]
    for stats, live in ((f["check"], f["mask"][0]), (f["check_all"], np.ones(N, dtype=bool))):
        rep, obs = stats
        assert rep.shape == (6, 4, max(LENGTHS)) and obs.shape == rep.shape
        y = f["c"]["data"][1]
        for c, n in enumerate(LENGTHS):
            assert np.all(np.isnan(rep[:, c, n:])) and np.all(np.isnan(obs[:, c, n:]))
            eta, mu, v = f["matrices"][c]
            for i in range(n):
                want_rep = hr.check_statistics(f["host"][c][i], mu[i], v[i], live)
                want_obs = hr.check_statistics(y, mu[i], v[i], live)
                assert hm.same_bits(rep[:, c, i], want_rep), (c, i, rep[:, c, i], want_rep)
                assert hm.same_bits(obs[:, c, i], want_obs), (c, i, obs[:, c, i], want_obs)
                q = f["host"][c][i][live]
                assert rep[2, c, i] == q.min() and rep[3, c, i] == q.max() and rep[4, c, i] == np.sum(q == 0)
                assert obs[2, c, i] == y[live].min() and obs[3, c, i] == y[live].max() and obs[4, c, i] == np.sum(y[live] == 0)


@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", MODELS, ids=IDS)
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("fma", [0, 1])
def test_purity_and_reduction(sim, model, geometry, fma):
    f = rep_case(sim, model, geometry, fma)
    check_purity(sim, f)
    check_reduction(f)


@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", MODELS, ids=IDS)
@pytest.mark.parametrize("N", [1, 63])
def test_small_blocks(sim, model, N):
    f = rep_case(sim, model, (1, 2), 1, N=N)
    check_purity(sim, f)
    check_reduction(f)


@pytest.mark.timeout(3600)
@pytest.mark.parametrize("model", MODELS, ids=IDS)
@pytest.mark.parametrize("geometry", [(1, 4), (1, 8)])
@pytest.mark.parametrize("N", [1, 63])
def test_small_blocks_at_four_and_eight_per_lane(sim, model, geometry, N):
    f = rep_case(sim, model, geometry, 1, N=N)
    check_purity(sim, f)
    check_reduction(f)


def check_invariance(lib, monkeypatch, geometry=(1, 2)):
    """one workgroup instead of one per item: identical bits everywhere, with and without the mask.  Another row order:
    row j of the permuted block is drawn on stream j from ITS mu, so the permuted block's replicate is the probe fed the
    permuted mu -- nothing but the key and the row's own mu and scale enters."""
    for model in (NB, HLOG):
        base = bits(rep_case(lib, model, geometry, 1))
        monkeypatch.setenv("WALNUTS_AMD_POINTWISE_GRID", "1")
        other = bits(rep_case(lib, model, geometry, 1))
        monkeypatch.delenv("WALNUTS_AMD_POINTWISE_GRID")
        assert len(base) == len(other) and all(hm.same_bits(a, b) for a, b in zip(base, other)), model
    model, N = NB, 65
    c = rep_case_data(model, geometry[1], N, seed=5)
    theta = thetas_for(model, c["D"], 2, seed=1)
    perm = np.random.default_rng(3).permutation(N)
    e = engine(lib, model, c, 1, geometry, 1, offset=c["offset"])
    mu = e.predict(theta)[1]
    e.close()
    pc = dict(c, data=tuple(a[perm] for a in c["data"]), offset=c["offset"][perm])
    e = engine(lib, model, pc, 1, geometry, 1, offset=pc["offset"])
    mu_p, rep_p = e.predict(theta)[1], e.replicate(theta, SEED)
    e.close()
    assert hm.same_bits(mu_p, mu[:, perm])
    scale = scales_of(lib, model, theta)
    for t in range(2):
        assert hm.same_bits(rep_p[t], probe_rows(lib, model, mu[t, perm], scale[t], t, 0))


def test_invariance_under_grid_mask_and_row_order(sim, monkeypatch):
    check_invariance(sim, monkeypatch)


@pytest.mark.parametrize("geometry", GEOMETRIES[1:])
def test_invariance_at_the_wider_geometries(sim, monkeypatch, geometry):
    check_invariance(sim, monkeypatch, geometry)


def check_seeds_and_streams(lib):
    """another seed, chain or draw changes the replicates; a short sampling run gives the same bits with a replicate call
    in its middle: the engine's momentum and tree streams are untouched"""
    model = POIS
    c = rep_case_data(model, 2, 65, seed=9)
    theta = np.repeat(thetas_for(model, c["D"], 1, seed=2), 3, axis=0)
    same = wa.MarkovChains.from_host([theta[:2], theta[:1]], lib_path=lib)
    e = engine(lib, model, c, 1, (1, 2), 1, offset=c["offset"])
    a, b = e.replicate(theta, SEED), e.replicate(theta, SEED + 1)
    gen = download(e.replicate_chains(same, SEED), 2, (2, 1))
    e.close()
    e_rep = a
    assert not np.array_equal(a, b)                                              # the seed
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])    # the chain (position t), equal theta
    assert np.array_equal(gen[0][0], e_rep[0]) and np.array_equal(gen[1][0], e_rep[1])   # (chain c, draw 0) = position c
    assert not np.array_equal(gen[0][0], gen[0][1])                              # the draw, equal theta
    runs = []
    for middle in (False, True):
        e = engine(lib, model, c, 3, (1, 2), 1, offset=c["offset"])
        e.set_positions(theta * 0.1)
        e.set_step_sizes(np.full(3, 0.05))
        e.seed_chains(SEED)
        e.freeze()
        e.sample_step()
        if middle:
            e.replicate(theta, SEED)
            e.replicate_check(same.__class__.from_host([theta[:2], theta[:1], theta[:1]], lib_path=lib), SEED)
        e.sample_step()
        e.sample_step()
        runs.append((e.positions(), e.logp(), e.rng_draws()))
        e.close()
    for x, y in zip(*runs):
        assert hm.same_bits(x, y)
    assert not np.array_equal(runs[0][0], theta * 0.1)


def test_seeds_ids_and_the_engines_own_streams(sim):
    check_seeds_and_streams(sim)


def check_nan_rule_and_masks(lib, geometry=(1, 2)):
    """a draw whose Poisson link overflows on a live row has NaN in all six replicate statistics and only there; one live
    row; a block that is masked out entirely: sums 0, min +inf, max -inf"""
    model, N = POIS, 65
    c = case_for(model, SMALL[geometry[1]], N, seed=21)
    theta = overflowing_theta(model, c, thetas_for(model, c["D"], 3, seed=4))   # the last position overflows row 0
    ch = wa.MarkovChains.from_host([theta], lib_path=lib)
    e = engine(lib, model, c, 1, geometry, 1, offset=c["offset"])
    mu = e.predict(theta)[1]
    assert mu[2, 0] == np.inf and np.isfinite(mu[:2]).all()
    rep, obs = e.replicate_check(ch, SEED)
    assert np.all(np.isnan(rep[:, 0, 2])) and not np.isnan(rep[:, 0, :2]).any()
    assert not np.isnan(obs[:5]).any()
    full = e.replicate(theta, SEED)
    assert np.isnan(full[2, 0]) and not np.isnan(full[:2]).any()
    served = mu[2] <= hr.POISSON_MU_MAX   # the rows the samplers do not serve masked out: the draw is valid again
    assert not served[0] and served.sum() > 10 and np.array_equal(np.isnan(full[2]), ~served)
    rep2, _ = e.replicate_check(ch, SEED, served)
    assert not np.isnan(rep2[:, 0, :]).any()
    one = np.arange(N) == 7
    rep1, obs1 = e.replicate_check(ch, SEED, one)
    y = c["data"][1]
    block = download(e.replicate_chains(ch, SEED), 3, (3,))[0]   # the check's draw i of chain 0 is keyed (chain 0, draw i):
    assert hm.same_bits(block[0], full[0])                       # the block's row i, and replicate()'s position 0 only
    for i in range(2):
        q = block[i, 7]
        assert rep1[0, 0, i] == q and rep1[1, 0, i] == q * q and rep1[2, 0, i] == q and rep1[3, 0, i] == q
        assert rep1[4, 0, i] == float(q == 0)
        assert obs1[0, 0, i] == y[7] and obs1[2, 0, i] == y[7] and obs1[3, 0, i] == y[7]
    none, none_obs = e.replicate_check(ch, SEED, np.zeros(N))
    for a in (none, none_obs):
        assert np.all(a[[0, 1, 4, 5]] == 0.0) and np.all(a[2] == np.inf) and np.all(a[3] == -np.inf)
    e.close()


def test_nan_rule_one_live_row_and_an_all_masked_block(sim):
    check_nan_rule_and_masks(sim)


@pytest.mark.parametrize("geometry", GEOMETRIES[1:])
def test_nan_rule_and_masks_at_the_wider_geometries(sim, geometry):
    check_nan_rule_and_masks(sim, geometry)


def check_generated_quantiles(f):
    """the generated chains are MarkovChains like any other: shape, lengths, and quantiles equal to the summary oracle's
    on the downloaded block"""
    gen, host, lengths = f["gen"][1], f["host"][2:], LENGTHS[2:]
    assert gen.num_chains() == 2 and gen.dims() == f["N"] and gen.num_draws() == sum(lengths)
    assert gen.min_chain_size() == min(lengths) and gen.max_chain_size() == max(lengths)
    probs = [0.05, 0.5, 0.95]
    assert np.array_equal(gen.quantiles(probs), wnso.quantiles(host, probs))
    assert np.array_equal(gen.mean(), wnso.mean(host))


def test_generated_chains_against_the_summary_oracle(sim):
    check_generated_quantiles(rep_case(sim, NB, (1, 2), 1))


def check_wrappers(sim):
    model, geometry, N = HLOG, (1, 2), 65
    c = case_for(model, SMALL[2], N, seed=5)
    cfg = config(sim, geometry, 1)
    draws, ch = ragged_chains(model, c["D"], LENGTHS, 3, sim)
    x, y, group = c["data"]
    e = engine(sim, model, c, 1, geometry, 1, offset=c["offset"])
    rep, obs = e.replicate_check(ch, SEED)
    gen_want = download(e.replicate_chains(ch, SEED), max(LENGTHS), LENGTHS)
    e.close()
    args = dict(num_params=c["D"], offset=c["offset"], cfg=cfg, lib_path=sim, seed=SEED)
    gen = wa.replicate_draws(model, ch, data=(x, group), **args)
    assert gen.num_chains() == 4 and gen.dims() == N
    for a, b in zip(download(gen, max(LENGTHS), LENGTHS), gen_want):
        assert np.array_equal(a, b)
    assert np.array_equal(gen.quantiles([0.1, 0.9]), wnso.quantiles(gen_want, [0.1, 0.9]))
    res = wa.posterior_predictive_check(model, ch, data=c["data"], **args)
    for s, name in enumerate(NAMES):
        assert hm.same_bits(res.rep[name], rep[s]) and hm.same_bits(res.obs[name], obs[s]), name
    valid = ~np.isnan(rep[0])
    assert valid.sum() == sum(LENGTHS) and res.invalid.tolist() == [0]
    for name in NAMES:
        assert res.p_value[name].shape == (1,)
        assert res.p_value[name][0] == np.mean(res.rep[name][valid] >= res.obs[name][valid])
    assert np.array_equal(res.rep["mean"][valid], (rep[0] / N)[valid])
    assert np.allclose(res.obs["var"][valid], np.var(y, ddof=1)) and np.allclose(res.obs["mean"][valid], y.mean())
    # a mask, and two weight sets over the shared rows: one p-value per set
    rows = np.arange(N) % 3 == 0
    masked = wa.posterior_predictive_check(model, ch, data=c["data"], rows=rows, **args)
    assert np.allclose(masked.obs["mean"][valid], y[rows].mean())
    two = wa.posterior_predictive_check(model, ch, data=c["data"], weight_sets=np.ones((2, N)), **args)
    assert two.p_value["sum"].shape == (2,) and two.invalid.tolist() == [0, 0]
    assert hm.same_bits(two.rep["sum"], rep[0])   # the same rows, chains and seed: the same replicates
    with pytest.raises(ValueError, match="MarkovChains"):
        wa.replicate_draws(model, [ch], data=(x, group), **args)


@pytest.mark.timeout(1800)
def test_wrappers(sim):
    check_wrappers(sim)


def test_refusals(sim, tmp_path):
    cfg = config(sim, (1, 2), 1)
    c = make_case(LOG, 5, 9, seed=1)
    _, ch = ragged_chains(LOG, c["D"], (2, 2, 2), 1, sim)
    # a model without data
    e = wa.DeviceEngine(wa.MODEL_STD_NORMAL, 5, 2, cfg, lib_path=sim)
    for call in (lambda: e.replicate(np.zeros((1, 5)), 1), lambda: e.replicate_check(ch, 1), lambda: e.replicate_chains(ch, 1)):
        with pytest.raises(ValueError, match="std_normal model: this engine holds no data"):
            call()
    e.close()
    # dims mismatch, chain count not a multiple of G, dataset / block out of range
    e = engine(sim, LOG, c, 2, (1, 2), 1, datasets=[c["data"], c["data"]], data=None)
    _, wrong = ragged_chains(LOG, c["D"] + 1, (2, 2), 1, sim)
    _, even = ragged_chains(LOG, c["D"], (2, 2), 1, sim)
    for call in (e.replicate_check, e.replicate_chains):
        with pytest.raises(ValueError, match="dimensions"):
            call(wrong, 1)
        with pytest.raises(ValueError, match="multiple"):
            call(ch, 1)
    with pytest.raises(ValueError, match="dataset must be in"):
        e.replicate(np.zeros((1, c["D"])), 1, dataset=2)
    for block in (-1, 2):
        with pytest.raises(ValueError, match="block must be in"):
            e.replicate_chains(even, 1, block=block)
    with pytest.raises(ValueError, match="row_mask must have shape"):
        e.replicate_check(even, 1, np.ones(3))
    # two datasets: chain block g meets dataset g's rows and observations
    rep, obs = e.replicate_check(even, 1)
    assert rep.shape == (6, 2, 2) and np.array_equal(obs[0, 0], obs[0, 1])   # (the two datasets are the same rows)
    err = C.c_void_p()
    assert e.lib.wn_engine_replicate(e.h, None, 1, 0, 1, None, C.byref(err)) != 0
    assert e.lib.walnutpie_get_error_type(err) == 1 and b"null argument" in e.lib.walnutpie_get_error_message(err)
    e.lib.walnutpie_destroy_error(err)
    e.close()
    # weight sets share one block of rows
    e = engine(sim, LOG, c, 2, (1, 2), 1, weight_sets=np.ones((2, 9)))
    with pytest.raises(ValueError, match="weight sets share one block"):
        e.replicate(np.zeros((1, c["D"])), 1, dataset=1)
    e.close()
    # a run-time model without the hook, built as in test_runtime_model.py
    gxx = ["g++", "-x", "c++", "-std=c++20", "-O1", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden", "-pthread",
           "-DWN_CPU_SIM", "-I", os.path.join(HERE, "cpusim")]
    header = os.path.join(HERE, "helpers", "user_diag_model.h")
    so = models.build_device_model(header, "user::MyDiagNormal", "user_diag_rp", 30, 130, out_dir=str(tmp_path),
                                   elems_per_lane=4, lib_path=sim, compiler=gxx)
    mid = models.load_device_model(so, "user_diag_rp", lib_path=sim)
    e = wa.DeviceEngine(mid, 130, 2, wa.default_config(sim, elems_per_lane=4), params=np.ones(130), lib_path=sim)
    _, ch130 = ragged_chains(LOG, 130, (2, 2), 1, sim)
    with pytest.raises(ValueError, match="user_diag_rp"):
        e.replicate_check(ch130, 1)
    e.close()
