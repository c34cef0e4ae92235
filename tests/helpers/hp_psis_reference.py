"""References for PSIS-LOO (walnuts_amd/csrc/wn_psis.h): the definition the header states, once in mpmath at 256 bits
(`row` / `rows`) and once in plain float64 NumPy (`numpy_rows`).  Both take the [S] column of pointwise terms l of one data
row (draws ordered by chain, then iteration) and return elpd_loo, pareto_k, ess, lpd.

The tail is selected by exact comparison of the doubles r = (-l) - max(-l) as the device forms them (numpy.lexsort on
the value, then the draw index); every value is then computed from l itself."""
import math

import mpmath as mp
import numpy as np

PRECISION = 256


def tail_size(S):
    """M = min(floor(S / 5), ceil(3 sqrt(S))), in integers"""
    root = math.isqrt(9 * S)
    return min(S // 5, root if root * root == 9 * S else root + 1)


def candidates(M):
    return 30 + math.isqrt(M)


def select(l):
    """(tail, cutoff index, M): the draws of the tail in ascending order of r, and the draw at sorted position S - M - 1"""
    l = np.asarray(l, dtype=np.float64)
    S = l.size
    r = (-l) - np.max(-l)
    order = np.lexsort((np.arange(S), r))
    M = tail_size(S)
    return order[S - M:], (order[S - M - 1] if M > 0 else -1), M


def row(l):
    """one column in mpmath -> dict(elpd_loo, pareto_k, ess, lpd, M, tail) (floats; pareto_k = inf without a fit)"""
    l = np.asarray(l, dtype=np.float64)
    S = l.size
    if not np.all(np.isfinite(l)):
        return dict(elpd_loo=math.nan, pareto_k=math.nan, ess=math.nan, lpd=math.nan, M=tail_size(S), tail=None)
    tail, at_cutoff, M = select(l)
    with mp.workprec(PRECISION):
        lm = [mp.mpf(float(v)) for v in l]
        mx = max(-v for v in lm)
        r = [-v - mx for v in lm]
        raw = [mp.exp(v) for v in r]             # raw weights: lw = r
        w = list(raw)
        khat = mp.inf
        if M >= 5:
            e_cut = w[at_cutoff]
            x = [w[s] - e_cut for s in tail]
            xq, xm = x[int(math.floor(M / 4 + 0.5)) - 1], x[M - 1]
            if xq > 0 and xm > 0:
                m = candidates(M)
                b = [1 / xm + (1 - mp.sqrt(mp.mpf(m) / (j - mp.mpf(1) / 2))) / (3 * xq) for j in range(1, m + 1)]
                k = [mp.fsum(mp.log1p(-bj * xi) for xi in x) / M for bj in b]
                L = [M * (mp.log(-bj / kj) - kj - 1) for bj, kj in zip(b, k)]
                wj = [1 / mp.fsum(mp.exp(Li - Lj) for Li in L) for Lj in L]
                bb = mp.fsum(bj * v for bj, v in zip(b, wj))
                kk = mp.fsum(mp.log1p(-bb * xi) for xi in x) / M
                sigma = -kk / bb
                kh = (M * kk + 5) / (mp.mpf(M) + 10)
                if mp.isfinite(kh) and mp.isfinite(sigma):
                    khat = kh
                    for i, s in enumerate(tail, start=1):
                        p = (mp.mpf(i) - mp.mpf(1) / 2) / M
                        smoothed = sigma * mp.expm1(-khat * mp.log1p(-p)) / khat + e_cut
                        w[s] = min(smoothed, mp.mpf(1))      # lw = min(log(...), 0)
        e_mx = mp.exp(-mx)
        # exp(l + lw): below the tail l + r = -mx; in the tail exp(l) w = exp(-mx) (w / exp(r))
        sum_w = mp.fsum(w)
        sum_lw = e_mx * (mp.mpf(S - M) + mp.fsum(w[s] / raw[s] for s in tail))
        elpd = mp.log(sum_lw) - mp.log(sum_w)
        ess = sum_w ** 2 / mp.fsum(v * v for v in w)
        inv = mp.fsum(1 / v for v in raw)        # exp(l) = exp(-mx) / exp(r)
        lpd = mp.log(e_mx * inv) - mp.log(S)
        return dict(elpd_loo=float(elpd), pareto_k=float(khat), ess=float(ess), lpd=float(lpd), M=M, tail=tail)


def rows(lmat, which=None):
    """`row` for the columns lmat[:, n], n in `which` (default: all) -> dict of [len(which)] arrays"""
    lmat = np.asarray(lmat, dtype=np.float64)
    which = range(lmat.shape[1]) if which is None else which
    out = [row(lmat[:, n]) for n in which]
    return {key: np.array([o[key] for o in out]) for key in ("elpd_loo", "pareto_k", "ess", "lpd")}


def numpy_row(l):
    """the same definition in float64 -> (elpd_loo, pareto_k, ess, lpd)"""
    l = np.asarray(l, dtype=np.float64)
    S = l.size
    if not np.all(np.isfinite(l)):
        return (math.nan,) * 4
    tail, at_cutoff, M = select(l)
    r = (-l) - np.max(-l)
    lw = r.copy()
    khat = math.inf
    if M >= 5:
        e_cut = np.exp(r[at_cutoff])
        x = np.exp(r[tail]) - e_cut
        xq, xm = x[int(math.floor(M / 4 + 0.5)) - 1], x[M - 1]
        if xq > 0 and xm > 0:
            m = candidates(M)
            j = np.arange(1, m + 1)
            b = 1 / xm + (1 - np.sqrt(m / (j - 0.5))) / (3 * xq)
            k = np.mean(np.log1p(-b[:, None] * x[None, :]), axis=1)
            L = M * (np.log(-b / k) - k - 1)
            wj = 1 / np.sum(np.exp(L[None, :] - L[:, None]), axis=1)
            bb = np.sum(b * wj)
            kk = np.mean(np.log1p(-bb * x))
            sigma = -kk / bb
            kh = (M * kk + 5) / (M + 10)
            if np.isfinite(kh) and np.isfinite(sigma):
                khat = float(kh)
                p = (np.arange(1, M + 1) - 0.5) / M
                lw[tail] = np.log(sigma * np.expm1(-khat * np.log1p(-p)) / khat + e_cut)
    lw = np.minimum(lw, 0.0)

    def lse(v):
        top = np.max(v)
        return top + np.log(np.sum(np.exp(v - top)))

    wn = np.exp(lw - lse(lw))
    return lse(l + lw) - lse(lw), khat, 1.0 / np.sum(wn * wn), lse(l) - math.log(S)


def numpy_rows(lmat):
    lmat = np.asarray(lmat, dtype=np.float64)
    out = np.array([numpy_row(lmat[:, n]) for n in range(lmat.shape[1])]).reshape(-1, 4)
    return dict(elpd_loo=out[:, 0], pareto_k=out[:, 1], ess=out[:, 2], lpd=out[:, 3])
