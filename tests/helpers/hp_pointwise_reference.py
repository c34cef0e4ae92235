"""High-precision reference for the pointwise log-likelihood and the predictive fold (walnuts_amd/csrc/wn_pointwise.h),
in the style of hp_weighted_reference.py: everything in mpmath at DPS digits from the float64 inputs, and bounds that are
K * u * the absolute version of the computation, K counted from the order of operations.

    eta_n = fsum_j x_nj beta_j (+ v_{g(n)}) + o_n,      A_n = sum_j |x_nj beta_j| (+ |v_{g(n)}|) + |o_n|
    l_n(theta) = the row term of hp_weighted_reference._row (the models' own, constants dropped) + c_n(y_n)
    c_n = -1/2 log 2 pi (identity links, linear_regression_sigma), 0 (logit links), -lgamma(y_n + 1) (log links, NB)
    l_abs = |row term|_abs + |dl/deta| A_n + |c_n|

THE BOUND OF ONE ENTRY, |l_device - l| <= K u l_abs + u |c_n|, with K counted along the kernel's order:
    eta: slot-order multiply-adds and the packed butterfly, depth EPL + 6 (hp_reference.glm_bound's count);
    + 1 for the add of the group effect (hierarchical models), whose value tau * z_g carries the K_TAU roundings of
      dexp(s) and one product: + K_TAU + 1 there;
    + 1 for the add of the offset;
    + C_LINK (identity, logit) or C_COUNT (log, negative binomial, sigma) for the link evaluation
      (hp_reference.C_LINK, hp_count_reference.C_COUNT: the links' own counted depths, the scale's constants included);
    + 1 for the add of the constant, the kernel's last operation;
    and one ulp of |c_n| for the host's constant (long double lgammal, rounded once): the u |c_n| term.
K multiplies the whole absolute version (a bound for the sum of the parts' own counts).

THE FOLD over the T draws of C chains of a block (draws in chain order, then iteration order), from the exact matrix:
    lpd = log mean_t exp l_t,   mean, var (T - 1 in the denominator) of l_t.
With d_l = max_t |l_device,t - l_t| <= max_t (entry bound), Dmax = max_t l_t - min_t l_t and L = max_t |l_t|:
    lpd:  log-sum-exp is 1-Lipschitz in the sup norm: d_l; each of the T running updates and C merges rounds the
          argument l - m (u Dmax relative in the exponential), evaluates dexp (C_EXP = 4 u, its 2 ulp doubled), one
          product and one add (2 u): (T + C)(6 + Dmax) u relative on s, i.e. absolute on log s; dlog twice
          (C_EXP u each on |log s|, |log T|) and the two final adds (u each on the partial sums):
          lpd_bound = d_l + u ((T + C)(6 + Dmax) + 6 (|m| + |log s| + |log T|)),  m = max_t l_t, s = sum exp(l_t - m)
    mean: the Welford update and the pairwise merge round 4 operations per draw / chain on values <= L:
          mean_bound = d_l + 4 (T + C) u L
    var:  a perturbation e of every l_t moves M2 by at most 2 dev e T, dev = max_t |l_t - mean|; the updates' own
          roundings are relative: var_bound = 2 dev mean_bound T / (T - 1) + 8 (T + C) u var
Nothing here was tuned to an observed error.  Entries that are not finite (a link that overflows) are compared for
non-finiteness by the tests, not against a bound.

sensitivity() says how far outside the entry bound five mistakes land: the offset dropped, the constant omitted, the
mask shifted by one row, block g's draws scored on block g + 1's rows, the weights applied."""
import math

import mpmath as mp
import numpy as np

import hp_weighted_reference as hw
from hp_count_reference import C_COUNT
from hp_reference import C_LINK, U

DPS = 60
C_EXP = 4


def k_entry(model, epl):
    fam = hw.family(model)
    k = epl + 6 + 1 + (C_LINK if fam in ("identity", "logit") else C_COUNT) + 1
    if model in hw.HIER:
        k += 1 + hw.K_TAU + 1
    return k


def row_const(fam, Y):
    if fam in ("identity", "sigma"):
        return -mp.log(2 * mp.pi) / 2
    if fam == "logit":
        return mp.mpf(0)
    return -mp.loggamma(Y + 1)


def reference(model, x, y, theta, epl, offset=None, group=None, constant=True):
    """dict(L: [T][N] mpf, ll: float64 [T, N], bound: [T, N]) -- the exact matrix, its rounding, the entry bounds"""
    fam = hw.family(model)
    th_all = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    T, D = th_all.shape
    N, P = x.shape
    hier = model in hw.HIER
    scale = fam in ("negbin", "sigma")
    J = D - P - 1 if hier else 0
    K = k_entry(model, epl)
    m = lambda v: mp.mpf(float(v))  # noqa: E731
    L, ll, bound = [], np.empty((T, N)), np.empty((T, N))
    with mp.workdps(DPS):
        X = [[m(v) for v in row] for row in x]
        Y = [m(v) for v in y]
        O = [m(v) for v in offset] if offset is not None else [mp.mpf(0)] * N
        Cn = [row_const(fam, Yn) if constant else mp.mpf(0) for Yn in Y]
        for t in range(T):
            th = [m(v) for v in th_all[t]]
            s = th[D - 1] if (hier or scale) else mp.mpf(0)
            tau = mp.exp(s)
            if hier:
                v = [th[P + j] if model in hw.CENTERED else tau * th[P + j] for j in range(J)]
            row = []
            for n in range(N):
                prods = [X[n][j] * th[j] for j in range(P)]
                vg = v[int(group[n])] if hier else mp.mpf(0)
                eta = mp.fsum(prods) + vg + O[n]
                A = mp.fsum(abs(p) for p in prods) + abs(vg) + abs(O[n])
                l, la, r = hw._row(fam, eta, Y[n], s)[:3]
                row.append(l + Cn[n])
                la_all = la + abs(r) * A + abs(Cn[n])
                b = K * U * la_all + U * abs(Cn[n])
                ll[t, n] = float(l + Cn[n])
                bound[t, n] = float(b) if mp.isfinite(b) and b < mp.mpf(10) ** 300 else math.inf
            L.append(row)
    return dict(L=L, ll=ll, bound=bound)


def fold(L_rows, bound_rows, num_chains):
    """The predictive values of ONE block from its draws' exact rows (L_rows: [T][N] mpf, in fold order) and their entry
    bounds [T, N]: dict(lpd, mean, var, lpd_bound, mean_bound, var_bound), float64 [N] each."""
    T, N = len(L_rows), len(L_rows[0])
    C = num_chains
    out = {k: np.empty(N) for k in ("lpd", "mean", "var", "lpd_bound", "mean_bound", "var_bound")}
    with mp.workdps(DPS):
        for n in range(N):
            col = [L_rows[t][n] for t in range(T)]
            dl = mp.mpf(float(np.max(np.asarray(bound_rows)[:, n])))
            big, small = max(col), min(col)
            s = mp.fsum(mp.exp(c - big) for c in col)
            lpd = big + mp.log(s) - mp.log(T)
            mean = mp.fsum(col) / T
            var = mp.fsum((c - mean) ** 2 for c in col) / (T - 1) if T > 1 else mp.nan
            Lmax = max(abs(c) for c in col)
            dev = max(abs(c - mean) for c in col)
            lpd_b = dl + U * ((T + C) * (6 + (big - small)) + 6 * (abs(big) + abs(mp.log(s)) + abs(mp.log(T))))
            mean_b = dl + 4 * (T + C) * U * Lmax
            var_b = 2 * dev * mean_b * T / (T - 1) + 8 * (T + C) * U * var if T > 1 else mp.nan
            for k, v in (("lpd", lpd), ("mean", mean), ("var", var), ("lpd_bound", lpd_b), ("mean_bound", mean_b),
                         ("var_bound", var_b)):
                out[k][n] = float(v)
    return out


def error_ratio(ll, ref):
    """max |ll - reference| / bound over the finite entries; the others must agree on non-finiteness exactly"""
    ll = np.asarray(ll)
    fin = np.isfinite(ref["ll"])
    assert np.array_equal(np.isfinite(ll), fin), "device and reference disagree on which entries are finite"
    assert np.array_equal(ll[~fin], ref["ll"][~fin], equal_nan=True)
    if not fin.any():
        return 0.0
    return float((np.abs(ll[fin] - ref["ll"][fin]) / np.maximum(ref["bound"][fin], 1e-300)).max())


def sensitivity(model, x, y, theta, epl, ref, offset=None, group=None, weights=None, other_rows=None, mask=None):
    """The smallest distance, in entry bounds, between `ref` and what each mistake would have produced -- each only
    where it applies: the offset dropped; the constant omitted (families that have one); the mask shifted by one row
    (the rows the shifted mask evaluates, compared with the rows it should have); block g's draws scored on block
    g + 1's rows (`other_rows`: that block's (x, y, offset, group), same N); the weights applied (w_n l_n for l_n)."""
    fin = np.isfinite(ref["ll"]) & np.isfinite(ref["bound"])
    b = np.maximum(ref["bound"], 1e-300)

    def dist(ll_wrong):
        d = np.abs(ll_wrong - ref["ll"])[fin] / b[fin]
        return float(d.max()) if d.size else math.inf

    worst = math.inf
    if offset is not None and np.any(offset != 0):
        worst = min(worst, dist(reference(model, x, y, theta, epl, None, group)["ll"]))
    if hw.family(model) != "logit":
        worst = min(worst, dist(reference(model, x, y, theta, epl, offset, group, constant=False)["ll"]))
    if mask is not None and len(y) > 1 and not np.array_equal(np.roll(mask, 1), mask):
        worst = min(worst, dist(np.roll(ref["ll"], 1, axis=1)))   # row n reports its neighbour's value
    if other_rows is not None:
        xo, yo, oo, go = other_rows
        worst = min(worst, dist(reference(model, xo, yo, theta, epl, oo, go)["ll"]))
    if weights is not None and not np.all((weights == 1) | (weights == 0)):
        worst = min(worst, dist(ref["ll"] * np.asarray(weights)[None, :]))
    return worst
