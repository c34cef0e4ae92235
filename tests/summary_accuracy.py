"""Shared body of the summary ACCURACY tests (CPU tier under the emulation, GPU tier on the device): the device
against the exact-arithmetic summaries of tests/helpers/hp_summary_reference.py within that helper's derived bounds,
the stated rule for non-finite draws, and the guard of the two-columns-per-lane kernels."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hp_summary_reference as hs  # noqa: E402
import summary_parity as sp  # noqa: E402
from summary_parity import wa, ws, wnso  # noqa: E402

PROBS = (0.0, 0.05, 0.25, 0.5, 0.6, 0.75, 0.95, 1.0)
PHIS = (0.99, -0.9, 0.0)     # runs until t < bound stops it / the antithetic tail matters / stops at once
MAX_PRODUCTS = 2e5           # exact products per case
LENGTHS = (3, 4, 5, 16, 17, 19, 20, 21, 32, 33, 36, 37)


def _ill(chains, d, kind):
    """column d made ill-conditioned, in place"""
    scale = 1.0 + d % 7
    for c, x in enumerate(chains):
        if kind == "off8":
            x[:, d] += 1e8 * scale
        elif kind == "off15":
            x[:, d] += 1e15 * scale
        elif kind == "tiny":
            x[:, d] *= 1e-140
        elif kind == "huge":
            x[:, d] *= 1e140
        elif kind == "rhat":          # chains with very different means: a large R-hat
            x[:, d] += 50.0 * scale * c
        else:
            raise KeyError(kind)


# name -> (seed, C, D, lens, {column: ill-conditioning})
# A column offset by 1e15 times its scale has a variance the bound makes no claim about beyond a few draws (the rounded
# mean's term N em^2 exceeds the variance), so its rho is a near tie by definition wherever the ESS reads one: such
# columns appear where the shortest chain has at most 5 draws and the sequence reads no rho (longer chains beside it).
CASES = {}
for _L in LENGTHS:                       # min_len = L: min_len - 4 straddles the lag blocks; 32/33: the wide limit
    CASES[f"len{_L}"] = (100 + _L, 2, 2, [_L + (0 if _L in (32, 37) else 1), _L], {})
CASES.update({
    "one_chain_one_column": (1, 1, 1, [19], {}),
    "one_chain_pair": (2, 1, 2, [37], {}),
    "three_chains_second_tile": (3, 3, 65, [33, 36, 37], {3: "off8", 5: "tiny", 7: "huge", 9: "rhat"}),
    "three_chains_wide_two_tiles": (4, 3, 130, [32, 19, 17], {3: "off8", 5: "tiny", 7: "huge", 9: "rhat", 66: "off8"}),
    "three_chains_wide_short": (5, 3, 130, [16, 3, 5], {2: "off15", 3: "off8", 5: "tiny", 7: "huge", 9: "rhat", 129: "off15"}),
    "three_chains_long_beside_short": (6, 3, 2, [36, 5, 20], {0: "off15", 1: "off8"}),
    "run_of_256_plus_one": (7, 257, 2, None, {}),
    "run_of_256_plus_one_ill": (8, 257, 2, None, {0: "off15", 1: "rhat"}),
    "pair_off8": (9, 3, 2, [20, 21, 36], {0: "off8", 1: "off8"}),
    "pair_tiny_huge": (10, 3, 2, [20, 21, 36], {0: "tiny", 1: "huge"}),
    "pair_rhat": (11, 3, 2, [17, 33, 4], {0: "rhat", 1: "rhat"}),
    "two_chains_one_column": (12, 2, 1, [21, 20], {}),
})
SUMMARIES = ("mean", "sample_variance", "sample_standard_deviation", "autocovariance", "r_hat",
             "effective_sample_size", "monte_carlo_standard_error", "quantiles")


def make_case(name):
    seed, C, D, lens, ill = CASES[name]
    rng = np.random.default_rng(seed)
    if lens is None:
        lens = [int(n) for n in rng.integers(3, 7, size=C)]
    phi = np.array([PHIS[d % 3] for d in range(D)])
    chains = sp.ar_chains(rng, C, D, lens, phi)
    for d, kind in ill.items():
        _ill(chains, d, kind)
    return chains


@functools.lru_cache(maxsize=None)
def reference(name):
    """the exact summaries of a case, computed once and shared"""
    cols = hs.columns(make_case(name))
    assert sum(c.products for c in cols) <= MAX_PRODUCTS, name
    return cols


def near_ties(name):
    return [d for d, c in enumerate(reference(name)) if c.near_tie]


def check_case(name, lib_path=None):
    """(a) every summary within its bound of the exact value, (b) the oracle's bits, (c) exact extremes; -> the worst
    error / bound per summary"""
    chains = make_case(name)
    cols = reference(name)
    D = len(cols)
    got = sp.check_all(chains, lib_path=lib_path, probs=PROBS)          # (b)
    near = near_ties(name)
    print(name, "columns", D, "near ties", len(near))
    assert len(near) <= D // 50, (name, near)
    stacked = np.concatenate(chains)
    q = got["quantiles"]
    assert np.array_equal(q[0], stacked.min(axis=0)) and np.array_equal(q[-1], stacked.max(axis=0))   # (c)
    worst = dict.fromkeys(SUMMARIES, 0.0)
    unbounded = dict.fromkeys(SUMMARIES, 0)

    def see(what, d, value, want):
        if want.e == hs.INF:
            unbounded[what] += 1
        r = hs.ratio(value, want)
        assert r <= 1.0, (name, what, d, float(value), want, r)
        worst[what] = max(worst[what], r)

    for d, c in enumerate(cols):                                                                  # (a)
        see("mean", d, got["mean"][d], c.mean)
        see("sample_variance", d, got["sample_variance"][d], c.var)
        see("sample_standard_deviation", d, got["sample_standard_deviation"][d], c.sd)
        row = 0
        for m, n in enumerate(c.lens):
            for t in range(n):
                see("autocovariance", d, got["autocovariance"][row + t, d], c.acov[m][t])
            row += n
        if c.C >= 2:
            see("r_hat", d, got["r_hat"][d], c.r_hat)
        if d not in near:
            see("effective_sample_size", d, got["effective_sample_size"][d], c.ess)
            see("monte_carlo_standard_error", d, got["monte_carlo_standard_error"][d], c.mcse)
        for k, p in enumerate(PROBS):
            see("quantiles", d, q[k, d], c.quantile(p))
    print(name, "worst error/bound", {k: float("%.3g" % v) for k, v in worst.items()},
          "no claim", {k: v for k, v in unbounded.items() if v})
    return worst


# ---- non-finite draws ---------------------------------------------------------------------------------------------
CLEAN = (0, 2, 7)
NAN_COL, INF_COL, BOTH_COL, ALLNAN_COL, CONST_COL = 1, 3, 4, 5, 6


def nonfinite_block(lens):
    rng = np.random.default_rng(21)
    chains = sp.ar_chains(rng, len(lens), 8, lens, np.array([PHIS[d % 3] for d in range(8)]))
    chains[1][4, NAN_COL] = np.nan
    chains[0][2, INF_COL] = np.inf
    chains[0][5, BOTH_COL] = np.inf
    chains[2][1, BOTH_COL] = -np.inf
    for x in chains:
        x[:, ALLNAN_COL] = np.nan
        x[:, CONST_COL] = 3.0
    return chains


def check_nonfinite_moments(lens, lib_path=None):
    """Moments, autocovariance, R-hat, ESS and MCSE propagate IEEE arithmetic as the reference's code does: the
    oracle's bits (NaN where it has NaN), the outcomes read off summary.hpp:593-619,663-749 as literals, and clean
    columns in the same wavefront keep the bits they have alone.  Returning at all is the stopping claim: the host
    driver of the resumable sequence either finishes or raises."""
    chains = nonfinite_block(lens)
    N = sum(lens)
    got = sp.check_all(chains, lib_path=lib_path, probs=PROBS)
    alone = sp.check_all([c[:, list(CLEAN)] for c in chains], lib_path=lib_path, probs=PROBS)
    for name in got:
        assert np.array_equal(got[name][..., list(CLEAN)], alone[name]), name
        assert np.all(np.isfinite(alone[name])), name
    nan = np.nan
    bad = [NAN_COL, INF_COL, BOTH_COL, ALLNAN_COL, CONST_COL]
    # a NaN draw poisons its chain's sum; +inf gives an infinite mean and inf - inf in the deviations; both infinities
    # cancel to NaN in the sum; a constant column has zero variances, so R-hat is sqrt(1 + 0/0) and rho(1) is 0/0
    literal = {"mean": [nan, np.inf, nan, nan, 3.0],
               "sample_variance": [nan, nan, nan, nan, 0.0],
               "sample_standard_deviation": [nan, nan, nan, nan, 0.0],
               "r_hat": [nan, nan, nan, nan, nan],
               # rho(1) is NaN, `(even + odd) > 0` is false, the sequence stops at once with even = 1:
               # tau = -1 + 2 * rho(0) + rho(2) = 2
               "effective_sample_size": [N / 2.0] * 5,
               "monte_carlo_standard_error": [nan, nan, nan, nan, 0.0]}
    for name, want in literal.items():
        assert np.array_equal(got[name][bad], np.array(want), equal_nan=True), (name, got[name][bad])
    assert np.all(got["autocovariance"][:, CONST_COL] == 0.0) and np.all(np.isnan(got["autocovariance"][:, ALLNAN_COL]))
    rows1 = slice(lens[0], lens[0] + lens[1])                 # the NaN draw is in chain 1: its lags only
    ac = got["autocovariance"][:, NAN_COL]
    assert np.all(np.isnan(ac[rows1])) and np.all(np.isfinite(np.delete(ac, np.arange(N)[rows1])))


def np_quantiles(chains, probs):
    """the stated rule: numpy.sort's order (NaNs last whatever their sign bit) and the reference's formula in double"""
    x = np.concatenate(chains)
    N = x.shape[0]
    srt = np.sort(x, axis=0)
    out = np.empty((len(probs), x.shape[1]))
    with np.errstate(invalid="ignore"):
        for k, p in enumerate(probs):
            h = float(p) * float(N - 1)
            lo = int(np.floor(h))
            hi = min(lo + 1, N - 1)
            out[k] = srt[lo] + (h - float(lo)) * (srt[hi] - srt[lo])
    return out


def _quantiles_vs_numpy(chains, probs, lib_path):
    dev = wa.MarkovChains.from_host(chains, lib_path=lib_path)
    got = ws.quantiles(dev, probs)
    dev.close()
    want = np_quantiles(chains, probs)
    assert np.array_equal(got, want, equal_nan=True), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert np.array_equal(wnso.quantiles(chains, probs), want, equal_nan=True)
    return got


def nan_sign_block():
    """65 draws (N - 1 = 64: p = r / 64 gives h = r exactly); columns 0 and 1 are equal but for the SIGN of their five
    NaNs; column 2 has infinities at both ends; column 3 infinities and NaNs"""
    rng = np.random.default_rng(31)
    x = np.repeat(rng.normal(size=(65, 1)), 4, axis=1)
    rows = [7, 20, 33, 46, 59]
    pos, neg = np.nan, np.copysign(np.nan, -1.0)
    assert not np.signbit(pos) and np.signbit(neg)
    x[rows, 0] = [pos, neg, pos, neg, pos]
    x[rows, 1] = [neg, pos, neg, neg, neg]
    x[[1, 2], 2] = -np.inf
    x[[3, 4], 2] = np.inf
    x[[1, 3], 3] = [-np.inf, np.inf]
    x[rows[:3], 3] = [neg, pos, neg]
    return [x[:30].copy(), x[30:].copy()]


def check_nan_sign_quantiles(lib_path=None):
    chains = nan_sign_block()
    first_nan = 60                                        # 65 draws, five NaNs: ranks 60 .. 64
    # lo and hi on finite ranks; hi on the first NaN rank (0 * (NaN - lo) is NaN), with a fraction; lo on it; both
    # beyond; three more; then eleven on a grid: a second sweep of the radix select
    probs = [58 / 64, 59 / 64, 59.5 / 64, first_nan / 64, 60.5 / 64, 1 / 64, 0.5 / 64, 63 / 64] + list(np.linspace(0, 1, 11))
    assert len(probs) > 8
    got = _quantiles_vs_numpy(chains, probs, lib_path)
    assert np.array_equal(got[:, 0], got[:, 1], equal_nan=True)          # the sign of a NaN does not matter
    assert np.isfinite(got[0, 0]) and np.all(np.isnan(got[1:5, 0]))
    # infinities at both ends: -inf + 0 * (-inf - -inf) and inf - inf are NaN where the formula says so, p = 0 and 1 too
    assert np.isnan(got[8, 2]) and np.isnan(got[-1, 2]) and np.isfinite(got[13, 2])


def check_many_nans_quantiles(lib_path=None):
    """2 500 NaNs, more than the radix select's candidate cap (2 048 on the device, 8 under the emulation): every
    pass runs on the one NaN key"""
    rng = np.random.default_rng(41)
    x = rng.normal(size=(3000, 2))
    where = rng.permutation(3000)[:2500]
    x[where, 0] = np.where(rng.uniform(size=2500) < 0.5, np.nan, np.copysign(np.nan, -1.0))
    chains = [x[:1000].copy(), x[1000:].copy()]
    got = _quantiles_vs_numpy(chains, [0.0, 0.1, 0.5, 1.0], lib_path)     # order statistics among the NaNs: 16 passes
    assert np.isfinite(got[1, 0]) and np.isnan(got[2, 0]) and np.all(np.isfinite(got[:, 1]))
    _quantiles_vs_numpy(chains, [0.0, 0.05, 0.1], lib_path)              # finite ranks only: the gathered finish


# ---- the guard of the two-columns-per-lane kernels ------------------------------------------------------------------
def all_summaries(dev):
    return {"mean": ws.mean(dev), "sample_variance": ws.sample_variance(dev),
            "sample_standard_deviation": ws.sample_standard_deviation(dev), "quantiles": ws.quantiles(dev, PROBS),
            "autocovariance": ws.autocovariance(dev), "r_hat": ws.r_hat(dev),
            "effective_sample_size": ws.effective_sample_size(dev),
            "monte_carlo_standard_error": ws.monte_carlo_standard_error(dev)}


def check_wide_guard(place, lib_path=None):
    """Short chains, even D: the same draws through MarkovChains.from_device with 16-byte aligned rows (the wide
    kernels), with an odd chain stride and with a base 8 bytes off a 16-byte boundary (the column loops) give the
    bits of the upload, for every summary.  `place(flat, off)` puts a host vector into memory the library can read,
    its first element `off` doubles past a 16-byte boundary, and returns (address, owner)."""
    rng = np.random.default_rng(51)
    C, T, D = 4, 32, 130
    lens = [32, 3, 17, 20]
    chains = sp.ar_chains(rng, C, D, lens, np.array([PHIS[d % 3] for d in range(D)]))
    up = wa.MarkovChains.from_host(chains, lib_path=lib_path)
    want = all_summaries(up)
    up.close()
    for form, stride, off in (("aligned", T * D, 0), ("odd stride", T * D + 1, 0), ("base off by 8 bytes", T * D, 1)):
        flat = np.full(C * stride, np.nan)                 # NaN wherever no draw lies: a read out of range shows
        for c, x in enumerate(chains):
            flat[c * stride:c * stride + x.size] = x.reshape(-1)
        ptr, owner = place(flat, off)
        assert ptr % 16 == 8 * off
        dev = wa.MarkovChains.from_device(ptr, C, T, D, chain_stride=stride, lengths=lens, lib_path=lib_path)
        got = all_summaries(dev)
        dev.close()
        del owner
        for name in want:
            assert np.array_equal(got[name], want[name]), (form, name)
            assert np.all(np.isfinite(got[name])), (form, name)
