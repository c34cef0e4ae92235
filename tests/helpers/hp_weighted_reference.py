"""High-precision reference for the data models with per-row offsets and weights (walnuts_amd/csrc/models/glm.h,
glm_scale.h, hier_glm.h; the order of operations in glm.h's header), with an error bound per chain in the style of
hp_reference.py / hp_count_reference.py: K * u * the absolute version of the computation.

Everything is evaluated in mpmath at DPS digits from the float64 inputs with an exact eta:
    eta_n = fsum_j x_nj beta_j (+ v_{g(n)}) + o_n,      A_n = sum_j |x_nj beta_j| (+ |v_{g(n)}|) + |o_n|
    logp  = prior(theta) + sum_n w_n l_n(eta_n, y_n, s),  r_n = w_n dl_n / deta_n,  d/ds += w_n dl_n / ds
(priors unweighted; v_g = tau z_g or a_g, the hierarchical models' group effect).

The bound is the unweighted models' bound with its absolute version multiplied through by w_n -- every row's term of
lp_abs, g_abs and the d/ds partial carries w_n, the prior terms carry none -- and K raised by the roundings the order
of operations adds:
    offset: lanes 0..B-1 add o_n to eta, ONE add: |d eta_n| grows by u (A_n + |o_n|).  A_n above already holds |o_n|,
            so this is +1 on the eta depth (EPL + 6) wherever it enters, in K_lp and in K_g;
    weight: the link is evaluated with a zero running sum -- the add of the row's term to the running sum that the
            unweighted path makes inside the link is now the add of Cx::mad(w, t, ll), the same count -- and the product
            w * t is rounded once more when the engine does not fuse: +1 in K_lp.  r = w * r (and ds_n * w) is one
            rounded product: +1 in K_g.
So K_lp and K_g are each the family's K + K_ROW_TERMS, K_ROW_TERMS = 2, whichever of the two fields is present (a bound
for both holds for either).  The families' K are those of hp_reference.glm_bound (linear, logistic),
hp_count_reference.count_bound (Poisson, negative binomial, linear with sigma) and test_hier_models_sim.hier_bound.

sensitivity() says how far outside the bound three mistakes land: the offset dropped, the weights shifted by one row,
w^2 in place of w."""
import math

import mpmath as mp
import numpy as np

from hp_count_reference import C_COUNT, abs_digamma_diff, abs_lgamma_diff
from hp_reference import C_LINK, U, block_rows

DPS = 60
LIN, LOG, POIS, NB, LSIG = 4, 5, 24, 25, 26
HLIN, HLOG, HLIN_C, HLOG_C, HPOIS, HPOIS_C = 15, 16, 17, 18, 27, 28
HIER = (HLIN, HLOG, HLIN_C, HLOG_C, HPOIS, HPOIS_C)
CENTERED = (HLIN_C, HLOG_C, HPOIS_C)
K_ROW_TERMS = 2
K_TAU = 12  # test_hier_models_sim.K_TAU


def family(model):
    if model in (LIN, HLIN, HLIN_C):
        return "identity"
    if model in (LOG, HLOG, HLOG_C):
        return "logit"
    if model in (POIS, HPOIS, HPOIS_C):
        return "log"
    return {NB: "negbin", LSIG: "sigma"}[model]


def _row(fam, eta, Y, S):
    """(l, l_abs, r, r_abs, slope, ds, ds_abs, dslope) of one row, as hp_reference / hp_count_reference define them"""
    zero = mp.mpf(0)
    if fam == "identity":
        r = Y - eta
        return -r * r / 2, r * r / 2, r, abs(r), mp.mpf(1), zero, zero, zero
    if fam == "logit":
        sp = mp.log1p(mp.exp(eta)) if eta < 0 else eta + mp.log1p(mp.exp(-eta))
        r = Y - 1 / (1 + mp.exp(-eta))
        return Y * eta - sp, abs(Y * eta) + sp + 1, r, abs(r), mp.mpf(1), zero, zero, zero
    if fam == "log":
        mu = mp.exp(eta)
        return Y * eta - mu, abs(Y * eta) + mu, Y - mu, Y + mu, mu, zero, zero, zero
    if fam == "negbin":
        phi = mp.exp(-S)
        t = eta + S
        sp = mp.log1p(mp.exp(t))
        sig = 1 / (1 + mp.exp(-t))
        lg = mp.loggamma(Y + phi) - mp.loggamma(phi)
        dg = mp.digamma(Y + phi) - mp.digamma(phi)
        r = Y - (Y + phi) * sig
        fphi = float(phi)
        lg_abs = abs_lgamma_diff(float(Y), fphi)
        dg_abs = abs_digamma_diff(float(dg), fphi)
        l_abs = lg_abs + abs(Y * t) + (Y + phi) * sp + phi * (sp + dg_abs)
        slope = abs(Y - r)
        ds_abs = Y + (Y + phi) * sig + phi * (sp + dg_abs) + Y
        return (lg + Y * t - (Y + phi) * sp, l_abs, r, Y + (Y + phi) * sig, slope, r + phi * (sp - dg), ds_abs,
                slope + mp.exp(eta))
    isig2 = mp.exp(-2 * S)
    d = Y - eta
    r = d * isig2
    return -d * d * isig2 / 2 - S, d * d * isig2 / 2 + abs(S), r, abs(r), isig2, d * d * isig2 - 1, d * d * isig2 + 1, 2 * abs(r)


def reference(model, x, y, params, theta, offset=None, weights=None, group=None):
    """(lp [C], g [C, D], lp_abs, g_abs) in float64, rounded once from mpmath."""
    fam = family(model)
    th_all = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    C, D = th_all.shape
    N, P = x.shape
    hier = model in HIER
    scale = fam in ("negbin", "sigma")
    J = D - P - 1 if hier else 0
    lp_o, lpa_o = np.empty(C), np.empty(C)
    g_o, ga_o = np.zeros((C, D)), np.zeros((C, D))
    m = lambda v: mp.mpf(float(v))  # noqa: E731
    with mp.workdps(DPS):
        X = [[m(v) for v in row] for row in x]
        Y = [m(v) for v in y]
        O = [m(v) for v in offset] if offset is not None else [mp.mpf(0)] * N
        W = [m(v) for v in weights] if weights is not None else [mp.mpf(1)] * N
        S2 = [m(v) for v in params[:P]]
        for c in range(C):
            th = [m(v) for v in th_all[c]]
            s = th[D - 1] if (hier or scale) else mp.mpf(0)
            tau = mp.exp(s)
            if hier:
                v = [th[P + j] if model in CENTERED else tau * th[P + j] for j in range(J)]
            ll, lla, rw, raw, dsw, dsaw = [], [], [], [], [], []
            for n in range(N):
                prods = [X[n][j] * th[j] for j in range(P)]
                vg = v[int(group[n])] if hier else mp.mpf(0)
                eta = mp.fsum(prods) + vg + O[n]
                A = mp.fsum(abs(p) for p in prods) + abs(vg) + abs(O[n])
                l, la, r, ra, slope, ds, dsa, dslope = _row(fam, eta, Y[n], s)
                ll.append(W[n] * l)
                lla.append(W[n] * (la + abs(r) * A))
                rw.append(W[n] * r)
                if fam in ("identity", "logit"):  # hp_reference.glm_reference: |r| + A
                    raw.append(W[n] * (abs(r) + A))
                else:                             # hp_count_reference.count_reference: r_abs + slope A
                    raw.append(W[n] * (ra + slope * A))
                dsw.append(W[n] * ds)
                dsaw.append(W[n] * (dsa + dslope * A))
            prior = mp.fsum(th[j] * th[j] / (2 * S2[j]) for j in range(P))
            lp = mp.fsum(ll) - prior
            lpa = mp.fsum(lla) + prior
            g = [mp.fsum(X[n][j] * rw[n] for n in range(N)) - th[j] / S2[j] for j in range(P)]
            ga = [mp.fsum(abs(X[n][j]) * raw[n] for n in range(N)) + abs(th[j]) / S2[j] for j in range(P)]
            if scale:
                tt = mp.exp(2 * s) / m(params[-1]) ** 2
                lp += s - tt / 2
                lpa += abs(s) + tt / 2
                g.append(mp.fsum(dsw) + 1 - tt)
                ga.append(mp.fsum(dsaw) + 1 + tt)
            if hier:
                tt = tau * tau / m(params[-1]) ** 2
                lp += s - tt / 2
                lpa += abs(s) + tt / 2
                Sj = [mp.fsum(rw[n] for n in range(N) if int(group[n]) == j) for j in range(J)]
                Sa = [mp.fsum(raw[n] for n in range(N) if int(group[n]) == j) for j in range(J)]
                u = th[P:P + J]
                if model in CENTERED:
                    q = mp.fsum(a * a for a in u) / (tau * tau)
                    lp += -J * s - q / 2
                    lpa += J * abs(s) + q / 2
                    g += [Sj[j] - u[j] / (tau * tau) for j in range(J)]
                    ga += [Sa[j] + abs(u[j]) / (tau * tau) for j in range(J)]
                    g.append(-J + q + 1 - tt)
                    ga.append(J + q + 1 + tt)
                else:
                    zz = mp.fsum(a * a for a in u) / 2
                    lp -= zz
                    lpa += zz
                    g += [tau * Sj[j] - u[j] for j in range(J)]
                    ga += [tau * Sa[j] + abs(u[j]) for j in range(J)]
                    g.append(tau * mp.fsum(u[j] * Sj[j] for j in range(J)) + 1 - tt)
                    ga.append(tau * mp.fsum(abs(u[j]) * Sa[j] for j in range(J)) + 1 + tt)
            lp_o[c], lpa_o[c] = float(lp), float(lpa)
            g_o[c] = [float(a) for a in g]
            ga_o[c] = [float(a) for a in ga]
    return lp_o, g_o, lpa_o, ga_o


def bound(model, lpa, ga, N, epl):
    """The family's K (module docstring) + K_ROW_TERMS, times u, times the weighted absolute versions."""
    B = block_rows(epl)
    fam = family(model)
    if fam in ("identity", "logit"):
        k_lp = -(-N // B) + epl + 6 + 6 + 4 + C_LINK
        k_g = N + 2 + epl + 6 + C_LINK
    else:
        k_lp = -(-N // B) + epl + 6 + 6 + 4 + C_COUNT
        k_g = N + 2 + epl + 6 + 6 + C_COUNT
    if model in HIER:
        k_lp += 1 + K_TAU + epl + 6 + 6
        k_g += 1 + K_TAU + epl + 6 + 6
    return (k_lp + K_ROW_TERMS) * U * np.asarray(lpa), (k_g + K_ROW_TERMS) * U * np.asarray(ga)


def case(model, x, y, params, theta, epl, offset=None, weights=None, group=None):
    """(lp_ref, g_ref, lp_bound, g_bound)"""
    lp, g, lpa, ga = reference(model, x, y, params, theta, offset, weights, group)
    blp, bg = bound(model, lpa, ga, len(y), epl)
    return lp, g, blp, bg


def error_ratio(lp, g, ref):
    lp_ref, g_ref, blp, bg = ref
    r_lp = np.abs(np.asarray(lp) - lp_ref) / np.maximum(blp, 1e-300)
    r_g = np.abs(np.asarray(g) - g_ref) / np.maximum(bg, 1e-300)
    return float(max(r_lp.max(), r_g.max()))


def sensitivity(model, x, y, params, theta, ref, offset=None, weights=None, group=None):
    """The smallest distance, in bounds, of the references with (the offset dropped, the weights shifted by one row,
    w^2 for w) from `ref` -- each only where it changes the inputs at all; inf when none does."""
    lp_ref, g_ref, blp, bg = ref
    cases = []
    if offset is not None and np.any(offset != 0):
        cases.append((None, weights))
    if weights is not None:
        if not np.array_equal(np.roll(weights, 1), weights):
            cases.append((offset, np.roll(weights, 1)))
        if not np.array_equal(weights * weights, weights):
            cases.append((offset, weights * weights))
    worst = math.inf
    for o, w in cases:
        lp, g, _, _ = reference(model, x, y, params, theta, o, w, group)
        d = max((np.abs(lp - lp_ref) / np.maximum(blp, 1e-300)).max(), (np.abs(g - g_ref) / np.maximum(bg, 1e-300)).max())
        worst = min(worst, float(d))
    return worst
