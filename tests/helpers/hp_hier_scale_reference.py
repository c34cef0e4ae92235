"""High-precision references for the grouped models with a scale parameter (walnuts_amd/csrc/models/hier_scale_glm.h:
hier_linear_regression_sigma*), built from hp_reference.py, hp_count_reference.py and hp_weighted_reference.py, with an
error bound per chain of the project's form: K * u * the absolute version of the computation.

    theta = [beta (P) | u (J) | s_tau | s],  tau = exp(s_tau),  v_g = tau z_g (non-centered) or a_g (centered)
    eta_n = x_n . beta + v_{g(n)} + o_n,       A_n = sum_j |x_nj beta_j| + |v_{g(n)}| + |o_n|
    logp  = prior(beta) + prior(u | tau) + [s_tau - tau^2 / (2 sigma_tau^2)] + [s - exp(2 s) / (2 sigma_0^2)]
            + sum_n w_n l_n(eta_n, y_n, s)

x_n . beta and sum_j |x_nj beta_j| are accumulated in np.longdouble as in hp_count_reference.py (64-bit significand: their
own error is below u / 2 of A_n at 1 024 columns, where every bound allows (EPL + 6) u A_n for eta); tau, the group
effect, the offset's add and each row's term -- hp_weighted_reference._row, the flat family's own -- are evaluated in
mpmath at DPS digits.  Rows of weight 0 are removed first: the kernel discards them by select, whatever their eta.

THE BOUND.  No constant grows.  K is hp_weighted_reference.bound's for a grouped model of a count family:
    K_lp = ceil(N / B) + EPL + 6 (eta) + 6 (lanes) + 4 (prior) + C_COUNT      (hp_count_reference.count_bound)
           + 1 (the add of v_g) + K_TAU + EPL + 6 + 6 (the epilogue's lane sum)  (test_hier_models_sim.hier_bound)
    K_g  = N + 2 + EPL + 6 + 6 + C_COUNT + 1 + K_TAU + EPL + 6 + 6
and + K_ROW_TERMS = 2 with offsets or weights (hp_weighted_reference.py counts them).  What the second scale adds is
already inside these: the family's row term with its d/ds partial is what C_COUNT was counted for (glm_scale.h's families,
used as they are); the lane sum of the d/ds partials shares the epilogue's ONE packed butterfly with sum_j z_j S_j, so the
depth EPL + 6 + 6 is paid once as before; the prior of s, (ds + 1) - scale * scale * isig0, is count_bound's "the scale's
prior terms fit in the same K".  The absolute versions carry both priors and, in S_j, the count families' r_abs + slope A.

The pointwise and predict references restate hp_pointwise_reference.reference / hp_predict_reference.reference for the
layout with two trailing scales, from those modules' own pieces (row_const, fold, error_ratio; _response, link_depth,
replay_fold): K is theirs for the flat family plus the grouped models' 1 + K_TAU + 1."""
import math

import mpmath as mp
import numpy as np

import hp_math_reference as hm
import hp_pointwise_reference as hpw
import hp_predict_reference as hpp
import hp_replicate_reference as hr
import hp_weighted_reference as hw
from hp_count_reference import C_COUNT
from hp_reference import U, block_rows, error_ratio  # noqa: F401  (error_ratio: re-exported for the tests)

DPS = 60
HSIG, HSIG_C = 35, 36  # walnuts_amd.MODEL_HIER_LINEAR_REGRESSION_SIGMA, _SIGMA_CENTERED
MODELS = (HSIG, HSIG_C)
CENTERED = (HSIG_C,)
FLAT = {HSIG: hw.LSIG, HSIG_C: hw.LSIG}   # the flat model of the same family
K_TAU = hw.K_TAU
K_ROW_TERMS = hw.K_ROW_TERMS


def family(model):
    return hw.family(FLAT[model])


def _m(v):
    return mp.mpf(float(v))


def _ld_to_mpf(v):
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))   # (the long double, exactly)


def _etas(model, x, theta, offset, group):
    """Per draw t: (s_tau, s, tau, [(eta_n, A_n)]) in mpmath (call inside mp.workdps)."""
    th_all = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    N, P = x.shape
    D = th_all.shape[1]
    J = D - P - 2
    ld = np.longdouble
    X, B = np.asarray(x, dtype=ld), th_all[:, :P].astype(ld)
    ETA, A = B @ X.T, np.abs(B) @ np.abs(X).T
    O = [_m(v) for v in offset] if offset is not None else [mp.mpf(0)] * N
    for t in range(th_all.shape[0]):
        st, s = _m(th_all[t, D - 2]), _m(th_all[t, D - 1])
        tau = mp.exp(st)
        v = [_m(th_all[t, P + j]) if model in CENTERED else tau * _m(th_all[t, P + j]) for j in range(J)]
        rows = []
        for n in range(N):
            vg = v[int(group[n])]
            rows.append((_ld_to_mpf(ETA[t, n]) + vg + O[n], _ld_to_mpf(A[t, n]) + abs(vg) + abs(O[n])))
        yield st, s, tau, rows


def reference(model, x, y, params, theta, offset=None, weights=None, group=None):
    """(lp [C], g [C, D], lp_abs, g_abs) in float64, rounded once."""
    fam = family(model)
    keep = np.arange(len(y)) if weights is None else np.flatnonzero(np.asarray(weights) != 0)
    x, y, group = np.asarray(x)[keep], np.asarray(y)[keep], np.asarray(group)[keep]
    offset = None if offset is None else np.asarray(offset)[keep]
    W = [mp.mpf(1)] * len(keep) if weights is None else [_m(v) for v in np.asarray(weights)[keep]]
    th_all = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    C, D = th_all.shape
    N, P = x.shape
    J = D - P - 2
    lp_o, lpa_o = np.empty(C), np.empty(C)
    g_o, ga_o = np.zeros((C, D)), np.zeros((C, D))
    members = [np.flatnonzero(group == j) for j in range(J)]
    smax = float(np.max(np.abs(th_all[:, D - 2:]))) if C else 0.0
    with mp.workdps(DPS + 20 + int(smax / 2.3)):
        Y = [_m(v) for v in y]
        S2 = [_m(v) for v in params[:P]]
        cols = [[_m(v) for v in x[:, j]] for j in range(P)]
        for c, (st, s, tau, rows) in enumerate(_etas(model, x, th_all, offset, group)):
            th = [_m(v) for v in th_all[c]]
            ll, lla, rw, raw, dsw, dsaw = [], [], [], [], [], []
            for n, (eta, A) in enumerate(rows):
                l, la, r, ra, slope, ds, dsa, dslope = hw._row(fam, eta, Y[n], s)
                ll.append(W[n] * l)
                lla.append(W[n] * (la + abs(r) * A))
                rw.append(W[n] * r)
                raw.append(W[n] * (ra + slope * A))
                dsw.append(W[n] * ds)
                dsaw.append(W[n] * (dsa + dslope * A))
            prior = mp.fsum(th[j] * th[j] / (2 * S2[j]) for j in range(P))
            tt = tau * tau / _m(params[D - 2]) ** 2
            ss = mp.exp(2 * s) / _m(params[D - 1]) ** 2
            lp = mp.fsum(ll) - prior + (st - tt / 2) + (s - ss / 2)
            lpa = mp.fsum(lla) + prior + (abs(st) + tt / 2) + (abs(s) + ss / 2)
            g = [mp.fsum(cols[j][n] * rw[n] for n in range(N)) - th[j] / S2[j] for j in range(P)]
            ga = [mp.fsum(abs(cols[j][n]) * raw[n] for n in range(N)) + abs(th[j]) / S2[j] for j in range(P)]
            Sj = [mp.fsum(rw[n] for n in members[j]) for j in range(J)]
            Sa = [mp.fsum(raw[n] for n in members[j]) for j in range(J)]
            u = th[P:P + J]
            if model in CENTERED:
                q = mp.fsum(a * a for a in u) / (tau * tau)
                lp += -J * st - q / 2
                lpa += J * abs(st) + q / 2
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
            g.append(mp.fsum(dsw) + 1 - ss)
            ga.append(mp.fsum(dsaw) + 1 + ss)
            lp_o[c], lpa_o[c] = float(lp), float(lpa)
            g_o[c] = [float(a) for a in g]
            ga_o[c] = [float(a) for a in ga]
    return lp_o, g_o, lpa_o, ga_o


def k_constants(N, epl, terms):
    """(K_lp, K_g) of the module docstring"""
    B = block_rows(epl)
    extra = 1 + K_TAU + epl + 6 + 6 + (K_ROW_TERMS if terms else 0)
    return -(-N // B) + epl + 6 + 6 + 4 + C_COUNT + extra, N + 2 + epl + 6 + 6 + C_COUNT + extra


def bound(lpa, ga, N, epl, terms):
    k_lp, k_g = k_constants(N, epl, terms)
    return k_lp * U * np.asarray(lpa), k_g * U * np.asarray(ga)


def case(model, x, y, params, theta, epl, offset=None, weights=None, group=None):
    """(lp_ref, g_ref, lp_bound, g_bound); N counts every row handed in (the kernel walks the rows of weight 0 too)"""
    lp, g, lpa, ga = reference(model, x, y, params, theta, offset, weights, group)
    blp, bg = bound(lpa, ga, len(y), epl, offset is not None or weights is not None)
    return lp, g, blp, bg


# ---- the hooks ------------------------------------------------------------------------------------------------------
def k_entry(model, epl):
    """hp_pointwise_reference.k_entry of the flat family, plus the grouped models' add of v_g, K_TAU and the product"""
    return hpw.k_entry(FLAT[model], epl) + 1 + K_TAU + 1


def pointwise_reference(model, x, y, theta, epl, offset=None, group=None, constant=True):
    """hp_pointwise_reference.reference for these models: dict(L [T][N] mpf, ll float64 [T, N], bound [T, N])"""
    fam = family(model)
    th_all = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    T, N = th_all.shape[0], len(y)
    K = k_entry(model, epl)
    L, ll, bnd = [], np.empty((T, N)), np.empty((T, N))
    with mp.workdps(DPS):
        Y = [_m(v) for v in y]
        Cn = [hpw.row_const(fam, Yn) if constant else mp.mpf(0) for Yn in Y]
        for t, (st, s, tau, rows) in enumerate(_etas(model, np.asarray(x), th_all, offset, group)):
            row = []
            for n, (eta, A) in enumerate(rows):
                l, la, r = hw._row(fam, eta, Y[n], s)[:3]
                row.append(l + Cn[n])
                b = K * U * (la + abs(r) * A + abs(Cn[n])) + U * abs(Cn[n])
                ll[t, n] = float(l + Cn[n])
                bnd[t, n] = float(b) if mp.isfinite(b) and b < mp.mpf(10) ** 300 else math.inf
            L.append(row)
    return dict(L=L, ll=ll, bound=bnd)


def k_eta(model, epl):
    return hpp.k_eta(FLAT[model], epl) + 1 + K_TAU + 1


def predict_reference(model, x, theta, epl, offset=None, group=None):
    """hp_predict_reference.reference for these models: dict(eta, mu, v, eta_bound, mu_bound, v_bound), [T, N] each"""
    fam = family(model)
    th_all = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    T, N = th_all.shape[0], np.asarray(x).shape[0]
    ke = k_eta(model, epl)
    kmu, kv = (ke + d for d in hpp.link_depth(fam))
    if fam == "sigma":
        kv = hpp.K_SCALE_SQ   # (no eta in scale * scale)
    out = {k: np.empty((T, N)) for k in ("eta", "mu", "v", "eta_bound", "mu_bound", "v_bound")}
    with mp.workdps(DPS):
        for t, (st, s, tau, rows) in enumerate(_etas(model, np.asarray(x), th_all, offset, group)):
            for n, (eta, A) in enumerate(rows):
                mu, dmu, v, va, dv = hpp._response(fam, eta, s)
                bounds = (ke * U * A, kmu * U * (abs(mu) + abs(dmu) * A), kv * U * (va + abs(dv) * A))
                for name, val, b in zip(hpp.NAMES, (eta, mu, v), bounds):
                    out[name][t, n] = hpp._f(val)
                    out[name + "_bound"][t, n] = hpp._f(b)
    return out


def replicate_probe(lib, model, mu, s, seed, chain, draw):
    """y_rep of one draw's rows from the sampler probe (hp_replicate_reference.sampler_probe) fed the device's own mu [N]
    and scale = wnd::dexp(s) with the device's bits (the maths probe): the normal's sd"""
    scale = hm.math_probe(lib, hm.EXP, np.array([float(s)]))[0]
    return hr.sampler_probe(lib, hr.NORMAL, mu, np.full(len(mu), scale), seed, chain, draw, 0, hr.GATHER)[0]


# ---- hier_linear_regression_sigma: the exact posterior by quadrature ------------------------------------------------
def trapezoid_weights(s):
    w = np.zeros_like(s)
    ds = np.diff(s)
    w[:-1] += ds / 2
    w[1:] += ds / 2
    return w


def exact_moments(x, y, group, params, J, step):
    """Means and variances of [beta (P) | a = tau u (J) | tau, sigma] of hier_linear_regression_sigma*, by a trapezoid
    rule of step `step` over (s_tau, s): given both, (beta, a) ~ N(0, diag(s2, tau^2)) a priori and y = W (beta, a) + e,
    e ~ N(0, sigma^2), W = [x | onehot(group)], so (beta, a) | s_tau, s, y is Gaussian and
    p(s_tau, s | y) ~ N(y; 0, sigma^2 I + W L W^T) exp(s_tau - tau^2 / (2 sigma_tau^2)) exp(s - sigma^2 / (2 sigma_0^2)).
    -> (mean, var, edge): edge is the largest weight on the boundary of the s grid relative to the largest weight (the
    s_tau grid starts where the weight falls like tau, as test_hier_slopes_gpu's does)."""
    N, P = x.shape
    W = np.concatenate([x, np.eye(J)[group]], axis=1)
    WtW, Wty = W.T @ W, W.T @ y
    st1 = np.arange(-12.0, 3.0 + step / 2, step)   # tau from 6e-6 (weight ~ tau) to 20 (exp(-200 / sigma_tau^2))
    s1 = np.arange(-3.0, 3.0 + step / 2, step)     # sigma from 0.05 (exp(-RSS / (2 sigma^2))) to 20
    st, s = (a.reshape(-1) for a in np.meshgrid(st1, s1, indexing="ij"))
    wq = np.outer(trapezoid_weights(st1), trapezoid_weights(s1)).reshape(-1)
    tau, sig = np.exp(st), np.exp(s)
    G = st.size
    diag = np.concatenate([np.broadcast_to(1.0 / params[:P], (G, P)), np.repeat((1.0 / tau ** 2)[:, None], J, axis=1)], axis=1)
    prec = WtW[None] / (sig * sig)[:, None, None] + diag[:, :, None] * np.eye(P + J)[None]
    cov = np.linalg.inv(prec)
    m = (cov @ Wty) / (sig * sig)[:, None]
    _, logdet_prec = np.linalg.slogdet(prec)
    logdet_prior = np.sum(np.log(params[:P])) + 2 * J * st
    logml = -0.5 * (y @ y - m @ Wty) / (sig * sig) - 0.5 * (2 * N * s + logdet_prior + logdet_prec)
    logw = logml + (st - tau ** 2 / (2 * params[P + J] ** 2)) + (s - sig ** 2 / (2 * params[P + J + 1] ** 2))
    rel = np.exp(logw - logw.max())
    on_edge = (s == s1[0]) | (s == s1[-1]) | (st == st1[-1])
    w = wq * rel
    w /= w.sum()
    first = np.concatenate([m, tau[:, None], sig[:, None]], axis=1)
    second = np.concatenate([np.diagonal(cov, axis1=1, axis2=2) + m * m, (tau * tau)[:, None], (sig * sig)[:, None]], axis=1)
    mean = w @ first
    return mean, w @ second - mean * mean, float(rel[on_edge].max())


def exact_posterior(x, y, group, params, J):
    """exact_moments on a grid that has converged: halving the step moves no value by more than 1e-4 of its posterior
    standard deviation (variances: of the variance), and the grid's edges in s, and its upper edge in s_tau, carry no
    weight."""
    mean, var, _ = exact_moments(x, y, group, params, J, 0.125)
    mean2, var2, edge = exact_moments(x, y, group, params, J, 0.0625)
    assert edge <= 1e-12, edge
    assert np.all(np.abs(mean2 - mean) <= 1e-4 * np.sqrt(var2)), np.max(np.abs(mean2 - mean) / np.sqrt(var2))
    assert np.all(np.abs(var2 - var) <= 1e-4 * np.minimum(var2, np.sqrt(var2))), np.max(np.abs(var2 - var) / var2)
    return mean2, var2


def exact_case():
    """P = 2, J = 5, 40 rows, every group observed eight times -> (x, y, group, params, P, J)"""
    P, J, N = 2, 5, 40
    rng = np.random.default_rng(31)
    x = rng.normal(size=(N, P))
    group = np.repeat(np.arange(J), N // J).astype(np.int32)
    a = 0.8 * rng.normal(size=J)
    y = x @ np.array([0.7, -0.4]) + a[group] + 0.7 * rng.normal(size=N)
    params = np.concatenate([np.full(P, 4.0), np.ones(J), [1.0, 1.0]])
    return x, y, group, params, P, J
