"""CPU tier: PSIS-LOO (walnuts_amd/csrc/wn_psis.h; wn_engine_psis_loo, DeviceEngine.psis_loo, wa.psis_loo) under the
workgroup emulation.

References: the header's definition in mpmath and in float64 NumPy (tests/helpers/hp_psis_reference.py), applied to the
device's own pointwise terms (DeviceEngine.log_lik of the same draws: the matrix is shown to equal them bit for bit), and
the closed-form leave-one-out density of a linear regression.  The device side of the same kernel source is compared bit
for bit in test_psis_gpu.py."""
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
import hp_psis_reference as hps  # noqa: E402
import hp_weighted_reference as hw  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from walnuts_amd import models  # noqa: E402
from test_pointwise_sim import case_for, thetas_for  # noqa: E402
from test_weights_sim import config, engine, make_case  # noqa: E402

LIN, LOG = hw.LIN, hw.LOG
KEYS = ("elpd_loo", "pareto_k", "ess", "lpd")
# The absolute bound on elpd_loo, pareto_k, ess and lpd against the mpmath reference: the emulation's worst error over
# CASES was 2.27e-12 (S = 2 000, N = 65, linear regression), times 16, rounded up to a power of two.
BOUND = 2.0 ** -34
assert BOUND <= 1e-9
# (S, N, model, P, masked): every S of the table (M = 4: no fit; M = 5; fewer draws than threads; M = 128, 129, 135) and
# every N, both models, P in {1, 5}, with and without a mask
CASES = ((24, 130, LIN, 1, False), (25, 65, LOG, 5, True), (200, 64, LOG, 1, False), (1800, 63, LIN, 5, True),
         (1830, 1, LOG, 5, False), (2000, 130, LOG, 5, True), (2000, 65, LIN, 1, False))
TAILS = {24: 4, 25: 5, 200: 40, 1800: 128, 1830: 129, 2000: 135}


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def ragged(S):
    """four chains of different lengths that add up to S, the last of one draw"""
    a, b = S // 2, S // 3
    return (a, b, S - a - b - 1, 1)


def chains_for(model, D, lengths, seed, lib):
    draws = [thetas_for(model, D, n, seed + i) for i, n in enumerate(lengths)]
    return draws, wa.MarkovChains.from_host(draws, lib_path=lib)


def mask_for(N):
    return np.arange(N) % 3 == 0


def run_case(lib, case, geometry=(1, 2), fma=1, with_log_lik=True):
    """(psis_loo's five outputs, log_lik [S, N] of the same draws or None, mask or None)"""
    S, N, model, P, masked = case
    c = case_for(model, P, N, seed=S + N)
    draws, ch = chains_for(model, c["D"], ragged(S), S, lib)
    mask = mask_for(N) if masked else None
    e = engine(lib, model, c, 1, geometry, fma, offset=c["offset"])
    out = e.psis_loo(ch, mask)
    ll = e.log_lik(np.concatenate(draws)) if with_log_lik else None
    e.close()
    return out, ll, mask


_references = {}


def reference(case, ll, mask):
    """the mpmath reference of a case's evaluated rows, computed once"""
    if case not in _references:
        which = np.arange(ll.shape[1]) if mask is None else np.flatnonzero(mask)
        _references[case] = (which, hps.rows(ll, which))
    return _references[case]


def worst_error(out, which, ref):
    worst = 0.0
    for i, key in enumerate(KEYS):
        got, want = out[i][which], ref[key]
        same = got == want                      # (+inf against +inf)
        assert np.all(np.isfinite(got[~same])) and np.all(np.isfinite(want[~same])), key
        if not np.all(same):
            worst = max(worst, float(np.max(np.abs(got[~same] - want[~same]))))
    return worst


def check_masked(out, mask):
    off = ~mask
    assert np.all(out[4][off] == 0)
    for a in out[:4]:
        assert np.all(np.isnan(a[off]))


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("case", CASES, ids=[f"S{c[0]}-N{c[1]}-{'lin' if c[2] == LIN else 'log'}-P{c[3]}" for c in CASES])
def test_against_high_precision(sim, case, record_property):
    S, N = case[:2]
    assert hps.tail_size(S) == TAILS[S] and hps.candidates(TAILS[S]) == 30 + math.isqrt(TAILS[S])
    out, ll, mask = run_case(sim, case)
    which, ref = reference(case, ll, mask)
    assert np.all(out[4][which] == S)
    if mask is not None:
        check_masked(out, mask)
    if TAILS[S] < 5:
        assert np.all(out[1][which] == math.inf)
    else:   # the reference fitted every row: the integers (tail and M) are its own
        assert np.all(np.isfinite(ref["pareto_k"]))
    worst = worst_error(out, which, ref)
    print(f"S {S} N {N}: worst absolute error {worst:.3g} (bound {BOUND:.3g})")
    record_property("worst_abs_error", worst)
    assert worst <= BOUND
    # the float64 reference agrees with the mpmath one to the same bound (what the GPU tier's end-to-end test relies on)
    npr = hps.numpy_rows(ll[:, which])
    assert worst_error([npr[k] for k in KEYS], np.arange(which.size), ref) <= BOUND


def constant_column(lib):
    """A row whose x and offset are zero has the same l at every draw: no tail to fit, the weights are equal.
    -> the outputs at S = 24 and S = 200"""
    N, P = 9, 5
    outs = []
    c = make_case(LOG, P, N, seed=8)
    x, y = c["data"]
    x[3] = 0.0
    off = c["offset"].copy()
    off[3] = 0.0
    for S in (24, 200):
        draws, ch = chains_for(LOG, c["D"], ragged(S), 5, lib)
        e = engine(lib, LOG, c, 1, (1, 2), 1, data=(x, y), offset=off)
        elpd, k, ess, lpd, count = outs_S = e.psis_loo(ch)
        outs.append(outs_S)
        l = e.log_lik(draws[0][:1])[0, 3]
        e.close()
        assert abs(l - math.log(0.5)) < 1e-15
        assert k[3] == math.inf and count[3] == S
        assert abs(elpd[3] - l) <= BOUND and abs(lpd[3] - l) <= BOUND and abs(ess[3] - S) <= BOUND
        if S == 200:
            assert np.all(np.isfinite(np.delete(k, 3)))
    return outs


def test_constant_column(sim):
    constant_column(sim)


def every_draw_twice(lib, half):
    """Two identical chains: every value is tied with its copy, and the odd M (5 of 26, 41 of 206) splits a pair across
    the cutoff -- the tie at T is counted into the tail once and stays below it once.  -> the outputs"""
    N, P = 7, 5
    S = 2 * half
    assert hps.tail_size(S) % 2 == 1
    c = make_case(LOG, P, N, seed=half)
    d = thetas_for(LOG, c["D"], half, 3)
    ch = wa.MarkovChains.from_host([d, d], lib_path=lib)
    e = engine(lib, LOG, c, 1, (1, 2), 1, offset=c["offset"])
    out = e.psis_loo(ch)
    ll = e.log_lik(np.concatenate([d, d]))
    e.close()
    ref = hps.rows(ll)
    assert worst_error(out, np.arange(N), ref) <= BOUND
    assert np.all(out[4] == S)
    return out


@pytest.mark.parametrize("half", [13, 103])
def test_every_draw_twice(sim, half):
    every_draw_twice(sim, half)


def nan_draw(sim):
    """One NaN draw in block 0: NaN for every row of dataset 0, dataset 1 as if it stood alone.  (`sim`: the library, None
    for the device's)  -> the PsisLoo of both blocks"""
    P = 5
    a, b = make_case(LOG, P, 65, seed=1), make_case(LOG, P, 9, seed=2)
    lengths = (30, 20, 25, 25)
    draws = [thetas_for(LOG, a["D"], n, 40 + i) for i, n in enumerate(lengths)]
    draws[1][7, 2] = math.nan
    ch = wa.MarkovChains.from_host(draws, lib_path=sim)
    cfg = config(sim, (1, 2), 1)
    res = wa.psis_loo(LOG, ch, num_params=a["D"], datasets=[a["data"], b["data"]], offset=[a["offset"], b["offset"]],
                      cfg=cfg, lib_path=sim)
    assert isinstance(res, wa.PsisLoo) and res.elpd_loo.shape == (74,)
    for v in (res.elpd_loo, res.pareto_k, res.ess, res.lpd):
        assert np.all(np.isnan(v[:65])) and np.all(np.isfinite(v[65:]))
    assert np.all(res.count[:65] == 50) and np.all(res.count[65:] == 50)
    alone = wa.psis_loo(LOG, wa.MarkovChains.from_host(draws[2:], lib_path=sim), num_params=b["D"], data=b["data"],
                        offset=b["offset"], cfg=cfg, lib_path=sim)
    for key in KEYS + ("count",):
        assert np.array_equal(getattr(res, key)[65:], getattr(alone, key))
    # the same two blocks as views: the same bits
    views = [wa.MarkovChains.from_host(draws[:2], lib_path=sim), wa.MarkovChains.from_host(draws[2:], lib_path=sim)]
    by_view = wa.psis_loo(LOG, views, num_params=a["D"], datasets=[a["data"], b["data"]],
                          offset=[a["offset"], b["offset"]], cfg=cfg, lib_path=sim)
    for key in KEYS + ("count",):
        assert np.array_equal(getattr(res, key), getattr(by_view, key), equal_nan=True)
    assert alone.elpd == float(np.sum(alone.elpd_loo)) and alone.looic == -2.0 * alone.elpd and np.isfinite(alone.se)
    assert alone.p_loo == float(np.sum(alone.lpd - alone.elpd_loo)) and alone.p_loo > 0
    assert alone.num_bad == int(np.sum(alone.pareto_k > 0.7))
    return res


def test_nan_draw(sim):
    nan_draw(sim)


def invariance(lib, monkeypatch, model=LOG, P=5, geometry=(1, 2), S=200):
    """What must not change a bit: a workspace of exactly 64 rows (three slabs for N = 130) against the default, the grid,
    the order of the rows; and the matrix is log_lik's.  -> the five outputs (for the GPU tier's comparison)"""
    N = 130
    c = case_for(model, P, N, seed=21)
    draws, ch = chains_for(model, c["D"], ragged(S), 9, lib)
    e = engine(lib, model, c, 1, geometry, 1, offset=c["offset"])
    base = e.psis_loo(ch)
    ld = (S + 7) // 8 * 8
    slabs = e.psis_loo(ch, workspace_bytes=64 * ld * 8)
    monkeypatch.setenv("WALNUTS_AMD_POINTWISE_GRID", "3")
    small_grid = e.psis_loo(ch)
    monkeypatch.setenv("WALNUTS_AMD_POINTWISE_GRID", "64")
    other_grid = e.psis_loo(ch, workspace_bytes=64 * ld * 8)
    monkeypatch.delenv("WALNUTS_AMD_POINTWISE_GRID")
    for other in (slabs, small_grid, other_grid):
        assert all(np.array_equal(a, b) for a, b in zip(base, other))
    matrix = e._psis_matrix(ch, S)
    assert matrix.shape == (N, S) and np.array_equal(matrix.T, e.log_lik(np.concatenate(draws)))
    e.close()
    rev = dict(c, data=tuple(a[::-1].copy() for a in c["data"]), offset=c["offset"][::-1].copy())
    e = engine(lib, model, rev, 1, geometry, 1, offset=rev["offset"])
    reversed_rows = e.psis_loo(ch)
    e.close()
    assert all(np.array_equal(a[::-1], b) for a, b in zip(base, reversed_rows))
    return base


@pytest.mark.timeout(1800)
def test_invariance(sim, monkeypatch):
    out = invariance(sim, monkeypatch)
    assert np.all(np.isfinite(out[0])) and np.all(out[4] == 200)


# ---- against the truth ---------------------------------------------------------------------------------------------
def linear_truth(seed):
    """N = 40, P = 3, prior variance 4, unit noise, y[0] shifted by 6 -> data, prior variances, 8 chains of 250 independent
    draws from the exact posterior, and the closed-form log p(y_n | y_-n) of every row"""
    N, P, S = 40, 3, 2000
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P))
    y = x @ rng.normal(size=P) + rng.normal(size=N)
    y[0] += 6.0
    s2 = np.full(P, 4.0)
    prec = x.T @ x + np.diag(1.0 / s2)
    Sigma = np.linalg.inv(prec)
    mu = Sigma @ x.T @ y
    draws = rng.multivariate_normal(mu, Sigma, size=S)
    exact = np.empty(N)
    for n in range(N):
        Sn = np.linalg.inv(prec - np.outer(x[n], x[n]))
        mn = Sn @ (x.T @ y - x[n] * y[n])
        v = 1.0 + x[n] @ Sn @ x[n]
        exact[n] = -0.5 * (y[n] - x[n] @ mn) ** 2 / v - 0.5 * math.log(2 * math.pi * v)
    return (x, y), s2, [draws[i * 250:(i + 1) * 250] for i in range(8)], exact


def check_truth(lib, seed):
    data, s2, chains, exact = linear_truth(seed)
    res = wa.psis_loo(LIN, wa.MarkovChains.from_host(chains, lib_path=lib), num_params=3, data=data,
                      cfg=config(lib, (1, 2), 1), lib_path=lib)
    assert np.all(res.count == 2000)
    good = res.pareto_k <= 0.5
    err_loo, err_lpd = np.sum(np.abs(res.elpd_loo - exact)[good]), np.sum(np.abs(res.lpd - exact)[good])
    print(f"seed {seed}: {int(good.sum())} rows, sum |elpd_loo - exact| {err_loo:.4g}, sum |lpd - exact| {err_lpd:.4g}, "
          f"worst khat {res.pareto_k.max():.3g}, num_bad {res.num_bad}")
    assert good.sum() >= 35
    assert err_loo <= 0.25 * err_lpd
    return res


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("seed", [2, 4])
def test_exact_loo_of_linear_regression(sim, seed):
    res = check_truth(sim, seed)
    if seed == 4:
        assert res.num_bad >= 1 and res.pareto_k[0] > 0.7   # the shifted row
    else:
        assert res.num_bad == 0


def test_refusals(sim, tmp_path):
    cfg = config(sim, (1, 2), 1)
    c = make_case(LOG, 5, 9, seed=1)
    _, ch = chains_for(LOG, c["D"], (10, 10, 10), 1, sim)
    args = dict(num_params=c["D"], data=c["data"], cfg=cfg, lib_path=sim)
    with pytest.raises(ValueError, match="weight_sets"):
        wa.psis_loo(LOG, ch, weight_sets=np.ones((3, 9)), **args)
    # a model without data
    e = wa.DeviceEngine(wa.MODEL_STD_NORMAL, 5, 2, cfg, lib_path=sim)
    with pytest.raises(ValueError, match="std_normal"):
        e.psis_loo(ch)
    e.close()
    # dims mismatch, chain count not a multiple of G
    e = engine(sim, LOG, c, 2, (1, 2), 1, datasets=[c["data"], c["data"]], data=None)
    _, wrong = chains_for(LOG, c["D"] + 1, (10, 10), 1, sim)
    with pytest.raises(ValueError, match="dimensions"):
        e.psis_loo(wrong)
    with pytest.raises(ValueError, match="multiple"):
        e.psis_loo(ch)
    e.close()
    # more draws than the tail limit admits: one chain that claims 1 864 136 draws of a buffer that holds one (the call
    # is refused before anything reads them); 1 864 135 would pass (M = 4 096)
    assert hps.tail_size(1864135) == 4096 and hps.tail_size(1864136) == 4097
    one = np.zeros((1, c["D"]))
    fake = wa.MarkovChains.from_device(one.ctypes.data, 1, 1864136, c["D"], lib_path=sim)
    e = engine(sim, LOG, c, 1, (1, 2), 1)
    with pytest.raises(ValueError, match="4096.*thin="):
        e.psis_loo(fake)
    e.close()
    # a run-time model without the hook, built as in test_runtime_model.py
    gxx = ["g++", "-x", "c++", "-std=c++20", "-O1", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden", "-pthread",
           "-DWN_CPU_SIM", "-I", os.path.join(HERE, "cpusim")]
    header = os.path.join(HERE, "helpers", "user_diag_model.h")
    so = models.build_device_model(header, "user::MyDiagNormal", "user_diag_psis", 31, 130, out_dir=str(tmp_path),
                                   elems_per_lane=4, lib_path=sim, compiler=gxx)
    mid = models.load_device_model(so, "user_diag_psis", lib_path=sim)
    e = wa.DeviceEngine(mid, 130, 2, wa.default_config(sim, elems_per_lane=4), params=np.ones(130), lib_path=sim)
    _, ch130 = chains_for(LOG, 130, (10, 10), 1, sim)
    with pytest.raises(ValueError, match="user_diag_psis"):
        e.psis_loo(ch130)
    e.close()
