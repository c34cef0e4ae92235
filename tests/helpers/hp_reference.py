"""High-precision references for the device models' log densities and gradients, with an error bound per chain.

Every reference takes the exact float64 inputs and evaluates the model's density in mpmath at DPS decimal digits
(a product of two doubles is exact at that precision and the sums are mpmath.fsum), then rounds once to float64.  The
one exception: a GLM case with N * D * C > MPMATH_LIMIT -- in this suite only test_logp_grad_matches_numpy at D = 1000,
N = 300, C = 4 -- is evaluated in np.longdouble (x87 extended, 64-bit significand) instead, where mpmath would take
tens of seconds.  Its own error, at most ~(D + N) * 2^-64 times the absolute version, stays below 1/30 of the bound.

The bound is not a relative tolerance on |logp|.  For each chain it is K * u * (the "absolute" version of the same
computation: every term and every intermediate replaced by its magnitude), u = 2^-53, with K read off the reduction
depths of the kernels (comments at glm_bound / simple_bound).  For separable logistic data logp is a small difference
of large terms, and only a bound of this kind stays both valid and tight there.

sensitivity() says how far outside the bound three indexing mistakes would land -- one observation dropped, y shifted by
one row, two columns of x swapped -- so a test can show that its bound could not hide one."""
import math

import mpmath as mp
import numpy as np

DPS = 40
U = 2.0 ** -53
LIN, LOG = 4, 5  # walnuts_amd.MODEL_LINEAR_REGRESSION / MODEL_LOGISTIC_REGRESSION
STD, DIAG, FUNNEL, RW1 = 0, 1, 2, 3
# ulps for the link's exp / log (wnd::dexp / wnd::dlog: a few ulps each), the one true division, the rounding of
# 1 + exp(-|eta|) (an absolute u: see glm_bound), and the factor by which the "1" of that sum can exceed |r| + A
# (<= 4: |eta| < 1 gives |r| >= 0.26, |eta| >= 1 gives A >= 1)
C_LINK = 16


def block_rows(epl):
    """Rows per register block of models/glm.h (kBlock)."""
    return 2 if epl >= 16 else 32 // epl


def _mpf_rows(a):
    return [[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(a)]


MPMATH_LIMIT = 200_000


def _glm_reference_longdouble(model, x, y, s2, theta):
    ld = np.longdouble
    X, Y, S2, TH = (np.asarray(a, dtype=ld) for a in (x, y, s2, np.atleast_2d(theta)))
    eta = TH @ X.T  # [C, N]
    A = np.abs(TH) @ np.abs(X).T
    if model == LIN:
        r = Y - eta
        ln = -r * r / 2
        la = r * r / 2
    elif model == LOG:
        sp = np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta)))
        r = Y - 1 / (1 + np.exp(-eta))
        ln = Y * eta - sp
        la = np.abs(Y * eta) + sp + 1
    else:
        raise ValueError(model)
    prior = TH * TH / (2 * S2)
    lp = ln.sum(axis=1) - prior.sum(axis=1)
    lpa = (la + np.abs(r) * A).sum(axis=1) + prior.sum(axis=1)
    g = r @ X - TH / S2
    ga = (np.abs(r) + A) @ np.abs(X) + np.abs(TH) / S2
    return tuple(np.asarray(a, dtype=np.float64) for a in (lp, g, lpa, ga))


def glm_reference(model, x, y, s2, theta):
    """Exact-input high-precision logp [C], grad [C, D] and their absolute versions for models/glm.h.

    eta_n = fsum_j x_nj theta_j (exact products), then the link.  Returns (lp, g, lp_abs, g_abs, ...), with
      lp_abs = sum_n (|l_n|' + |r_n| A_n) + sum_j theta_j^2 / (2 s_j^2),    A_n = sum_j |x_nj theta_j|
      g_abs_j = sum_n |x_nj| (|r_n| + A_n) + |theta_j| / s_j^2
    where |l_n|' is the absolute version of the row's term: r^2 / 2 (linear), |y eta| + softplus(eta) + 1 (logistic:
    the 1 of 1 + exp(-|eta|), whose rounding is an absolute error of u in log(1 + exp(-|eta|)))."""
    if x.size * np.atleast_2d(theta).shape[0] > MPMATH_LIMIT and np.finfo(np.longdouble).nmant >= 63:
        return _glm_reference_longdouble(model, x, y, s2, theta)
    with mp.workdps(DPS):
        X = _mpf_rows(x)
        Y = [mp.mpf(float(v)) for v in y]
        S2 = [mp.mpf(float(v)) for v in s2]
        N, D = len(X), len(S2)
        th_all = np.atleast_2d(theta)
        out = [np.empty(len(th_all)) for _ in range(2)] + [np.empty((len(th_all), D)) for _ in range(2)]
        lp_o, lpa_o, g_o, ga_o = out[0], out[1], out[2], out[3]
        for c, th_row in enumerate(th_all):
            th = [mp.mpf(float(v)) for v in th_row]
            lp_terms, lpa_terms, r, A = [], [], [], []
            for n in range(N):
                prods = [X[n][j] * th[j] for j in range(D)]
                eta = mp.fsum(prods)
                a = mp.fsum(abs(p) for p in prods)
                if model == LIN:
                    rn = Y[n] - eta
                    ln = -rn * rn / 2
                    la = rn * rn / 2
                elif model == LOG:
                    sp = mp.log1p(mp.exp(eta)) if eta < 0 else eta + mp.log1p(mp.exp(-eta))
                    rn = Y[n] - 1 / (1 + mp.exp(-eta))
                    ln = Y[n] * eta - sp
                    la = abs(Y[n] * eta) + sp + 1
                else:
                    raise ValueError(model)
                r.append(rn)
                A.append(a)
                lp_terms.append(ln)
                lpa_terms.append(la + abs(rn) * a)
            prior = [th[j] * th[j] / (2 * S2[j]) for j in range(D)]
            lp_o[c] = float(mp.fsum(lp_terms) - mp.fsum(prior))
            lpa_o[c] = float(mp.fsum(lpa_terms) + mp.fsum(prior))
            for j in range(D):
                g_o[c, j] = float(mp.fsum([X[n][j] * r[n] for n in range(N)]) - th[j] / S2[j])
                ga_o[c, j] = float(mp.fsum([abs(X[n][j]) * (abs(r[n]) + A[n]) for n in range(N)]) + abs(th[j]) / S2[j])
    return lp_o, g_o, lpa_o, ga_o


def glm_bound(lp_abs, g_abs, N, epl):
    """Per-chain error bounds (lp [C], g [C, D]) for models/glm.h at EPL elements per lane (one wavefront per chain).

    eta_n: EPL lane-local multiply-adds, then a 6-level butterfly -> |d eta_n| <= (EPL + 6) u A_n.  The link turns that
    into |d r_n| <= (EPL + 6) u A_n + C_LINK u (|r_n| + A_n) (|d sigmoid| <= 1/4; the mean's absolute error of a few u is
    covered because |r| + A >= 0.26 always) and into |d l_n| <= |r_n| |d eta_n| + C_LINK u |l_n|'.
    logp: each lane adds its rows' terms in turn (ceil(N / B) adds), then the prior partial of EPL multiply-adds with a
    rounded reciprocal variance, then the 6-level lane reduction:
        K_lp = ceil(N / B) + EPL + 6 (eta) + 6 (lanes) + 4 (prior, reciprocal, final add) + C_LINK.
    gradient j: -theta_j * rs2_j, then one multiply-add per row, all N rows in order:
        K_g = N + 2 + EPL + 6 (eta) + C_LINK."""
    B = block_rows(epl)
    k_lp = -(-N // B) + epl + 6 + 6 + 4 + C_LINK
    k_g = N + 2 + epl + 6 + C_LINK
    return k_lp * U * np.asarray(lp_abs), k_g * U * np.asarray(g_abs)


def error_ratio(lp, g, ref):
    """max over chains and components of |computed - reference| / bound (<= 1: within the bound).  `ref` =
    (lp_ref, g_ref, lp_bound, g_bound)."""
    lp_ref, g_ref, blp, bg = ref
    r_lp = np.abs(np.asarray(lp) - lp_ref) / np.maximum(blp, 1e-300)
    r_g = np.abs(np.asarray(g) - g_ref) / np.maximum(bg, 1e-300)
    return float(max(r_lp.max(), r_g.max()))


def glm_case(model, x, y, s2, theta, epl):
    """(lp_ref, g_ref, lp_bound, g_bound) for one GLM case."""
    lp, g, lpa, ga = glm_reference(model, x, y, s2, theta)
    blp, bg = glm_bound(lpa, ga, len(y), epl)
    return lp, g, blp, bg


def sensitivity(model, x, y, s2, theta, ref):
    """How far outside the bound three indexing mistakes land: for each of (the last observation dropped, y shifted by
    one row, the first and last columns of x swapped) that changes the inputs at all, the largest |perturbed reference
    - reference| / bound over chains and components; returns the smallest of these."""
    lp_ref, g_ref, blp, bg = ref
    N, D = x.shape
    cases = [(x[:-1], y[:-1])]
    if not np.array_equal(np.roll(y, 1), y):
        cases.append((x, np.roll(y, 1)))
    xs = x.copy()
    xs[:, [0, D - 1]] = xs[:, [D - 1, 0]]
    if not np.array_equal(xs, x):
        cases.append((xs, y))
    worst = math.inf
    for xp, yp in cases:
        lp, g, _, _ = glm_reference(model, xp.reshape(-1, D), yp, s2, theta)
        d = max((np.abs(lp - lp_ref) / blp).max(), (np.abs(g - g_ref) / bg).max())
        worst = min(worst, float(d))
    return worst


# ---- the models without data ------------------------------------------------------------------------------------

def _rw1_inv_sigma_sq_error():
    """Relative error of the kernel's constant 1 / (1 - rho * rho), each operation rounded, rho = 0.99 (models/rw1.h):
    1 - rho^2 cancels, so it is ~50 u, not one."""
    rho = 0.99
    computed = 1.0 / (1.0 - rho * rho)
    with mp.workdps(DPS):
        exact = 1 / (1 - mp.mpf(rho) ** 2)
        return float(abs(mp.mpf(computed) - exact) / exact)


RW1_CONST_REL = _rw1_inv_sigma_sq_error()


def simple_reference(model, theta, params=None):
    """High-precision logp [C], grad [C, D] and their absolute versions for the std / diagonal normal, the funnel and
    rw1 (models/rw1.h's header formula with rho the double 0.99)."""
    th_all = np.atleast_2d(theta)
    C, D = th_all.shape
    lp_o, lpa_o = np.empty(C), np.empty(C)
    g_o, ga_o = np.empty((C, D)), np.empty((C, D))
    with mp.workdps(DPS):
        P = None if params is None else [mp.mpf(float(v)) for v in params]
        for c in range(C):
            t = [mp.mpf(float(v)) for v in th_all[c]]
            if model == STD:
                lp = -mp.fsum(v * v for v in t) / 2
                lpa = -lp
                g = [-v for v in t]
                ga = [abs(v) for v in t]
            elif model == DIAG:
                q = [t[j] * t[j] / P[j] for j in range(D)]
                lp = -mp.fsum(q) / 2
                lpa = -lp
                g = [-t[j] / P[j] for j in range(D)]
                ga = [abs(v) for v in g]
            elif model == FUNNEL:  # v ~ N(0, 3^2), x_i | v ~ N(0, e^v)
                v = t[0]
                S = mp.fsum(a * a for a in t[1:])
                ev = mp.exp(-v)
                hd = mp.mpf(D - 1) / 2
                lp = -v * v / 18 - ev * S / 2 - hd * v
                lpa = v * v / 18 + ev * S / 2 + hd * abs(v)
                g = [-v / 9 + ev * S / 2 - hd] + [-a * ev for a in t[1:]]
                ga = [abs(v) / 9 + ev * S / 2 + hd] + [abs(a) * ev for a in t[1:]]
            elif model == RW1:
                rho = mp.mpf(0.99)
                inv = 1 / (1 - rho * rho)
                r = [t[0]] + [t[n] - rho * t[n - 1] for n in range(1, D)]
                ra = [abs(t[0])] + [abs(t[n]) + rho * abs(t[n - 1]) for n in range(1, D)]
                w = [r[0]] + [r[n] * inv for n in range(1, D)]
                wa = [ra[0]] + [ra[n] * inv for n in range(1, D)]
                lp = -mp.fsum(r[n] * w[n] for n in range(D)) / 2
                lpa = mp.fsum(ra[n] * wa[n] for n in range(D)) / 2
                g = [-w[n] + (rho * w[n + 1] if n + 1 < D else 0) for n in range(D)]
                ga = [wa[n] + (rho * wa[n + 1] if n + 1 < D else 0) for n in range(D)]
            else:
                raise ValueError(model)
            lp_o[c], lpa_o[c] = float(lp), float(lpa)
            g_o[c] = [float(a) for a in g]
            ga_o[c] = [float(a) for a in ga]
    return lp_o, g_o, lpa_o, ga_o


def simple_bound(model, lp_abs, g_abs, per_lane, nw):
    """Per-chain error bounds for the models without data, `per_lane` = Dp / (64 NW) coordinates per lane (register
    kernels: EPL; streaming: two per tile).

    logp: each lane accumulates its coordinates' terms in turn (per_lane adds), the 64 lanes reduce in 6 levels and the
    NW wavefronts' partials in at most NW adds; a few more for finish(), the diagonal normal's rounded reciprocal
    variances and the funnel's rounded 1/18, 1/9 and its exp (C_LINK covers the ulps of exp):
        K = per_lane + 6 + NW + C_LINK.
    The gradients are one to three roundings per coordinate, except the funnel's first one, which carries the sum S:
    the same K covers both.  rw1 adds the relative error of its constant 1 / (1 - rho^2) (RW1_CONST_REL, ~50 u)."""
    k = per_lane + 6 + nw + C_LINK
    rel = k * U + (RW1_CONST_REL if model == RW1 else 0.0)
    return rel * np.asarray(lp_abs), rel * np.asarray(g_abs)


def simple_case(model, theta, params, per_lane, nw):
    lp, g, lpa, ga = simple_reference(model, theta, params)
    blp, bg = simple_bound(model, lpa, ga, per_lane, nw)
    return lp, g, blp, bg
