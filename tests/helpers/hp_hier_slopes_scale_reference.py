"""High-precision references for varying slopes by group with an estimated noise level (walnuts_amd/csrc/models/
hier_slopes_scale_glm.h: hier_linear_regression_slopes_sigma), built from hp_hier_scale_reference.py and its pieces, with
an error bound per chain of the project's form: K * u * the absolute version of the computation.

    theta = [beta (P) | u_0 (J) | .. | u_{Q-1} (J) | s_0 .. s_{Q-1} | s],  tau_q = exp(s_q),  D = P + Q (J + 1) + 1
    z_{n,0} = 1,  z_{n,q} = x_{n,q-1},  v_n = sum_q tau_q u_{q,g(n)} z_{n,q}
    eta_n = x_n . beta + v_n + o_n,        A_n = sum_j |x_nj beta_j| + sum_q |tau_q u_{q,g(n)} z_{n,q}| + |o_n|
    logp  = prior(beta) - 1/2 sum u^2 + sum_q [s_q - tau_q^2 / (2 sigma_q^2)] + [s - exp(2 s) / (2 sigma_0^2)]
            + sum_n w_n l_n(eta_n, y_n, s)

x_n . beta and sum_j |x_nj beta_j| are accumulated in np.longdouble (hp_hier_scale_reference.py says why that is enough);
every tau_q, the group terms, the offset's add and each row's term -- hp_weighted_reference._row, the flat family's own --
are evaluated in mpmath.  Rows of weight 0 are removed first: the kernel discards them by select, whatever their eta.

THE BOUND.  hp_hier_scale_reference.k_constants (the constants of hier_scale_glm.h's evaluation, none grown) plus a COUNT
of the operations this model adds to one evaluation, K_SLOPES(Q) = 3 (Q - 1) + 1, test_hier_slopes_sim.k_extra's count
without its row terms (k_constants has K_ROW_TERMS already):
    per q >= 1 the product tau_q * u_q (1 rounding) and the multiply-add into v (2 roundings unfused), each relative to a
    partial sum that A_n bounds: 3 (Q - 1) on eta, which the family's term carries into every row term, residual and d/ds
    partial; the product r * z_q before the scatter: 1.
K_TAU covers every tau_q at once, each error being relative to its own term of A_n.  The epilogue's cx.sum1 at q >= 1 has
the depth EPL + 6 + 6 the packed sum of q = 0 has, and every coordinate goes through exactly one of them.  No constant is
fitted.  At Q = 1 the count is 1 above hp_hier_scale_reference's (which this model then reproduces bit for bit).

The pointwise and predict references: hp_hier_scale_reference's, with 3 (Q - 1) more on eta."""
import math

import mpmath as mp
import numpy as np

import hp_hier_scale_reference as hs
import hp_math_reference as hm
import hp_pointwise_reference as hpw
import hp_predict_reference as hpp
import hp_replicate_reference as hr
import hp_weighted_reference as hw
from hp_reference import U, error_ratio  # noqa: F401  (error_ratio: re-exported for the tests)

DPS = hs.DPS
MODEL = 40  # walnuts_amd.MODEL_HIER_LINEAR_REGRESSION_SLOPES_SIGMA
FAMILY = hw.family(hw.LSIG)
_m, _ld_to_mpf = hs._m, hs._ld_to_mpf


def dim(P, J, Q):
    return P + Q * (J + 1) + 1


def k_slopes(Q):
    """the operations the slopes add (module docstring)"""
    return 3 * (Q - 1) + 1


def _etas(x, theta, Q, offset, group):
    """Per draw t: (s_q [Q], s, tau_q [Q], [(eta_n, A_n)]) in mpmath (call inside mp.workdps)."""
    th_all = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    N, P = x.shape
    D = th_all.shape[1]
    J = (D - P - 1) // Q - 1
    assert dim(P, J, Q) == D
    ld = np.longdouble
    X, B = np.asarray(x, dtype=ld), th_all[:, :P].astype(ld)
    ETA, A = B @ X.T, np.abs(B) @ np.abs(X).T
    O = [_m(v) for v in offset] if offset is not None else [mp.mpf(0)] * N
    Z = [[mp.mpf(1)] + [_m(x[n, q - 1]) for q in range(1, Q)] for n in range(N)]
    for t in range(th_all.shape[0]):
        sq = [_m(th_all[t, D - 1 - Q + q]) for q in range(Q)]
        s = _m(th_all[t, D - 1])
        tau = [mp.exp(a) for a in sq]
        rows = []
        for n in range(N):
            j = int(group[n])
            terms = [tau[q] * _m(th_all[t, P + q * J + j]) * Z[n][q] for q in range(Q)]
            rows.append((_ld_to_mpf(ETA[t, n]) + mp.fsum(terms) + O[n],
                         _ld_to_mpf(A[t, n]) + mp.fsum(abs(a) for a in terms) + abs(O[n])))
        yield sq, s, tau, rows


def reference(x, y, params, theta, Q, offset=None, weights=None, group=None):
    """(lp [C], g [C, D], lp_abs, g_abs) in float64, rounded once."""
    keep = np.arange(len(y)) if weights is None else np.flatnonzero(np.asarray(weights) != 0)
    x, y, group = np.asarray(x)[keep], np.asarray(y)[keep], np.asarray(group)[keep]
    offset = None if offset is None else np.asarray(offset)[keep]
    W = [mp.mpf(1)] * len(keep) if weights is None else [_m(v) for v in np.asarray(weights)[keep]]
    th_all = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    C, D = th_all.shape
    N, P = x.shape
    J = (D - P - 1) // Q - 1
    lp_o, lpa_o = np.empty(C), np.empty(C)
    g_o, ga_o = np.zeros((C, D)), np.zeros((C, D))
    members = [np.flatnonzero(group == j) for j in range(J)]
    smax = float(np.max(np.abs(th_all[:, D - 1 - Q:]))) if C else 0.0
    with mp.workdps(DPS + 20 + int(smax / 2.3)):
        Y = [_m(v) for v in y]
        S2 = [_m(v) for v in params[:P]]
        cols = [[_m(v) for v in x[:, j]] for j in range(P)]
        Z = [[mp.mpf(1)] * N] + [cols[q - 1] for q in range(1, Q)]
        for c, (sq, s, tau, rows) in enumerate(_etas(x, th_all, Q, offset, group)):
            th = [_m(v) for v in th_all[c]]
            ll, lla, rw, raw, dsw, dsaw = [], [], [], [], [], []
            for n, (eta, A) in enumerate(rows):
                l, la, r, ra, slope, ds, dsa, dslope = hw._row(FAMILY, eta, Y[n], s)
                ll.append(W[n] * l)
                lla.append(W[n] * (la + abs(r) * A))
                rw.append(W[n] * r)
                raw.append(W[n] * (ra + slope * A))
                dsw.append(W[n] * ds)
                dsaw.append(W[n] * (dsa + dslope * A))
            prior = mp.fsum(th[j] * th[j] / (2 * S2[j]) for j in range(P))
            tt = [tau[q] * tau[q] / _m(params[D - 1 - Q + q]) ** 2 for q in range(Q)]
            ss = mp.exp(2 * s) / _m(params[D - 1]) ** 2
            zz = mp.fsum(a * a for a in th[P:P + Q * J]) / 2
            lp = mp.fsum(ll) - prior - zz + mp.fsum(sq[q] - tt[q] / 2 for q in range(Q)) + (s - ss / 2)
            lpa = mp.fsum(lla) + prior + zz + mp.fsum(abs(sq[q]) + tt[q] / 2 for q in range(Q)) + (abs(s) + ss / 2)
            g = [mp.fsum(cols[j][n] * rw[n] for n in range(N)) - th[j] / S2[j] for j in range(P)]
            ga = [mp.fsum(abs(cols[j][n]) * raw[n] for n in range(N)) + abs(th[j]) / S2[j] for j in range(P)]
            gs, gsa = [], []
            for q in range(Q):
                u = th[P + q * J:P + (q + 1) * J]
                Sj = [mp.fsum(rw[n] * Z[q][n] for n in members[j]) for j in range(J)]
                Sa = [mp.fsum(raw[n] * abs(Z[q][n]) for n in members[j]) for j in range(J)]
                g += [tau[q] * Sj[j] - u[j] for j in range(J)]
                ga += [tau[q] * Sa[j] + abs(u[j]) for j in range(J)]
                gs.append(tau[q] * mp.fsum(u[j] * Sj[j] for j in range(J)) + 1 - tt[q])
                gsa.append(tau[q] * mp.fsum(abs(u[j]) * Sa[j] for j in range(J)) + 1 + tt[q])
            g += gs + [mp.fsum(dsw) + 1 - ss]
            ga += gsa + [mp.fsum(dsaw) + 1 + ss]
            lp_o[c], lpa_o[c] = float(lp), float(lpa)
            g_o[c] = [float(a) for a in g]
            ga_o[c] = [float(a) for a in ga]
    return lp_o, g_o, lpa_o, ga_o


def k_constants(N, Q, epl, terms):
    """(K_lp, K_g): hp_hier_scale_reference.k_constants plus k_slopes(Q) (module docstring)"""
    k_lp, k_g = hs.k_constants(N, epl, terms)
    return k_lp + k_slopes(Q), k_g + k_slopes(Q)


def bound(lpa, ga, N, Q, epl, terms):
    k_lp, k_g = k_constants(N, Q, epl, terms)
    return k_lp * U * np.asarray(lpa), k_g * U * np.asarray(ga)


def case(x, y, params, theta, Q, epl, offset=None, weights=None, group=None):
    """(lp_ref, g_ref, lp_bound, g_bound); N counts every row handed in (the kernel walks the rows of weight 0 too)"""
    lp, g, lpa, ga = reference(x, y, params, theta, Q, offset, weights, group)
    blp, bg = bound(lpa, ga, len(y), Q, epl, offset is not None or weights is not None)
    return lp, g, blp, bg


# ---- the hooks ------------------------------------------------------------------------------------------------------
def k_entry(Q, epl):
    return hs.k_entry(hs.HSIG, epl) + 3 * (Q - 1)


def pointwise_reference(x, y, theta, Q, epl, offset=None, group=None, constant=True):
    """dict(L [T][N] mpf, ll float64 [T, N], bound [T, N]), as hp_hier_scale_reference.pointwise_reference"""
    th_all = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    T, N = th_all.shape[0], len(y)
    K = k_entry(Q, epl)
    L, ll, bnd = [], np.empty((T, N)), np.empty((T, N))
    with mp.workdps(DPS):
        Y = [_m(v) for v in y]
        Cn = [hpw.row_const(FAMILY, Yn) if constant else mp.mpf(0) for Yn in Y]
        for t, (sq, s, tau, rows) in enumerate(_etas(np.asarray(x), th_all, Q, offset, group)):
            row = []
            for n, (eta, A) in enumerate(rows):
                l, la, r = hw._row(FAMILY, eta, Y[n], s)[:3]
                row.append(l + Cn[n])
                b = K * U * (la + abs(r) * A + abs(Cn[n])) + U * abs(Cn[n])
                ll[t, n] = float(l + Cn[n])
                bnd[t, n] = float(b) if mp.isfinite(b) and b < mp.mpf(10) ** 300 else math.inf
            L.append(row)
    return dict(L=L, ll=ll, bound=bnd)


def k_eta(Q, epl):
    return hs.k_eta(hs.HSIG, epl) + 3 * (Q - 1)


def predict_reference(x, theta, Q, epl, offset=None, group=None):
    """dict(eta, mu, v, eta_bound, mu_bound, v_bound), [T, N] each, as hp_hier_scale_reference.predict_reference"""
    th_all = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    T, N = th_all.shape[0], np.asarray(x).shape[0]
    ke = k_eta(Q, epl)
    kmu = ke + hpp.link_depth(FAMILY)[0]
    kv = hpp.K_SCALE_SQ   # (no eta in scale * scale)
    out = {k: np.empty((T, N)) for k in ("eta", "mu", "v", "eta_bound", "mu_bound", "v_bound")}
    with mp.workdps(DPS):
        for t, (sq, s, tau, rows) in enumerate(_etas(np.asarray(x), th_all, Q, offset, group)):
            for n, (eta, A) in enumerate(rows):
                mu, dmu, v, va, dv = hpp._response(FAMILY, eta, s)
                bounds = (ke * U * A, kmu * U * (abs(mu) + abs(dmu) * A), kv * U * (va + abs(dv) * A))
                for name, val, b in zip(hpp.NAMES, (eta, mu, v), bounds):
                    out[name][t, n] = hpp._f(val)
                    out[name + "_bound"][t, n] = hpp._f(b)
    return out


def replicate_probe(lib, mu, s, seed, chain, draw):
    """y_rep of one draw's rows from the sampler probe fed the device's own mu [N] and scale = wnd::dexp(s) with the
    device's bits: fmad(scale, z, mu) (hp_hier_scale_reference.replicate_probe)"""
    scale = hm.math_probe(lib, hm.EXP, np.array([float(s)]))[0]
    return hr.sampler_probe(lib, hr.NORMAL, mu, np.full(len(mu), scale), seed, chain, draw, 0, hr.GATHER)[0]


# ---- the exact posterior by a three-dimensional quadrature ----------------------------------------------------------
S_STEPS = 2   # the grids of s_0 and s_1 take S_STEPS * step: their posteriors are several times wider than that of s


def exact_moments(x, y, group, params, J, step, chunk=1 << 15):
    """Means and variances of [beta (P) | a_0 = tau_0 u_0 (J) | a_1 = tau_1 u_1 (J) | tau_0, tau_1, sigma] at Q = 2, by a
    trapezoid rule over (s_0, s_1, s) of steps (S_STEPS step, S_STEPS step, step): given the three, (beta, a_0, a_1) ~
    N(0, diag(s2, tau_0^2, tau_1^2)) a priori and y = W (beta, a_0, a_1) + e, e ~ N(0, sigma^2), W = [x | onehot(g) |
    onehot(g) x_0], so (beta, a) | s_0, s_1, s, y is Gaussian and
    p(s_0, s_1, s | y) ~ N(y; 0, sigma^2 I + W L W^T) prod_q exp(s_q - tau_q^2 / (2 sigma_q^2)) exp(s - sigma^2 / (2 sigma_0^2)).
    The grid is walked in chunks under a running maximum of the log weight.  -> (mean, var, edge): edge is the largest
    weight on the boundary of the s grid and on the upper boundaries of the s_q grids relative to the largest weight
    (the s_q grids start where the weight falls like tau_q, as hp_hier_scale_reference.exact_moments' does)."""
    N, P = x.shape
    Q = 2
    oh = np.eye(J)[group]
    W = np.concatenate([x, oh, oh * x[:, :1]], axis=1)
    F = P + Q * J
    WtW, Wty, yy = W.T @ W, W.T @ y, y @ y
    q1 = np.arange(-12.0, 2.5 + step / 2, S_STEPS * step)   # tau_q from 6e-6 (weight ~ tau_q) to 12 (exp(-74 / sigma_q^2))
    s1 = np.arange(-3.0, 2.5 + step / 2, step)              # sigma from 0.05 (exp(-RSS / (2 sigma^2))) to 12
    wq1, ws1 = hs.trapezoid_weights(q1), hs.trapezoid_weights(s1)
    G = q1.size * q1.size * s1.size
    top = -np.inf
    norm, edge_top = 0.0, -np.inf
    first, second = np.zeros(F + 3), np.zeros(F + 3)
    logdet_s2 = np.sum(np.log(params[:P]))
    for lo in range(0, G, chunk):
        idx = np.arange(lo, min(lo + chunk, G))
        i0, i1, i2 = np.unravel_index(idx, (q1.size, q1.size, s1.size))
        s0, sb, s = q1[i0], q1[i1], s1[i2]
        t0, tb, sig = np.exp(s0), np.exp(sb), np.exp(s)
        n = idx.size
        diag = np.concatenate([np.broadcast_to(1.0 / params[:P], (n, P)), np.repeat((1.0 / t0 ** 2)[:, None], J, axis=1),
                               np.repeat((1.0 / tb ** 2)[:, None], J, axis=1)], axis=1)
        prec = WtW[None] / (sig * sig)[:, None, None] + diag[:, :, None] * np.eye(F)[None]
        cov = np.linalg.inv(prec)
        m = (cov @ Wty) / (sig * sig)[:, None]
        _, logdet_prec = np.linalg.slogdet(prec)
        logdet_prior = logdet_s2 + 2 * J * (s0 + sb)
        logml = -0.5 * (yy - m @ Wty) / (sig * sig) - 0.5 * (2 * N * s + logdet_prior + logdet_prec)
        logw = (logml + (s0 - t0 ** 2 / (2 * params[F] ** 2)) + (sb - tb ** 2 / (2 * params[F + 1] ** 2))
                + (s - sig ** 2 / (2 * params[F + 2] ** 2)))
        on_edge = (i2 == 0) | (i2 == s1.size - 1) | (i0 == q1.size - 1) | (i1 == q1.size - 1)
        if on_edge.any():
            edge_top = max(edge_top, float(logw[on_edge].max()))
        new_top = max(top, float(logw.max()))
        rescale = math.exp(top - new_top) if np.isfinite(top) else 0.0
        top = new_top
        w = wq1[i0] * wq1[i1] * ws1[i2] * np.exp(logw - top)
        f1 = np.concatenate([m, t0[:, None], tb[:, None], sig[:, None]], axis=1)
        f2 = np.concatenate([np.diagonal(cov, axis1=1, axis2=2) + m * m, (t0 * t0)[:, None], (tb * tb)[:, None],
                             (sig * sig)[:, None]], axis=1)
        norm = norm * rescale + w.sum()
        first = first * rescale + w @ f1
        second = second * rescale + w @ f2
    mean = first / norm
    return mean, second / norm - mean * mean, math.exp(edge_top - top)


def exact_posterior(x, y, group, params, J):
    """exact_moments on a grid that has converged: halving the step moves no value by more than 1e-4 of its posterior
    standard deviation (variances: of the variance), and the grid's edges in s, and its upper edges in s_q, carry no
    weight (hp_hier_scale_reference.exact_posterior's rule and steps)."""
    mean, var, _ = exact_moments(x, y, group, params, J, 0.125)
    mean2, var2, edge = exact_moments(x, y, group, params, J, 0.0625)
    assert edge <= 1e-12, edge
    assert np.all(np.abs(mean2 - mean) <= 1e-4 * np.sqrt(var2)), np.max(np.abs(mean2 - mean) / np.sqrt(var2))
    assert np.all(np.abs(var2 - var) <= 1e-4 * np.minimum(var2, np.sqrt(var2))), np.max(np.abs(var2 - var) / var2)
    return mean2, var2


def exact_case():
    """Q = 2, P = 2, J = 4, 40 rows, every group observed ten times -> (x, y, group, params, P, J, Q)"""
    P, J, Q, N = 2, 4, 2, 40
    rng = np.random.default_rng(37)
    x = rng.normal(size=(N, P))
    group = np.repeat(np.arange(J), N // J).astype(np.int32)
    a0, a1 = 0.8 * rng.normal(size=J), 0.6 * rng.normal(size=J)
    y = x @ np.array([0.7, -0.4]) + a0[group] + a1[group] * x[:, 0] + 0.7 * rng.normal(size=N)
    params = np.concatenate([np.full(P, 4.0), np.ones(Q * J), [1.0, 1.0], [1.0]])
    return x, y, group, params, P, J, Q
