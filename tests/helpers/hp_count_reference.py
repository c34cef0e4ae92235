"""High-precision references for the count models and the linear model with an estimated noise level
(walnuts_amd/csrc/models/glm.h LogLink, models/glm_scale.h) and for their maths (wnd::dlog1p, dsoftplus, dlgamma_diff,
ddigamma_diff in wn_devmath.h), with an error bound per chain in the style of hp_reference.py: K * u * the absolute
version of the computation.

eta_n and A_n = sum_j |x_nj beta_j| are accumulated in np.longdouble (64-bit significand: their own error is below
u / 2 of A_n even at 1 024 columns, and every bound allows (EPL + 6) u A_n for eta); each row's link -- exp, softplus,
lgamma and digamma differences -- is evaluated in mpmath at DPS digits from the float64 inputs and that eta."""
import math

import mpmath as mp
import numpy as np

from hp_reference import U, block_rows

DPS = 60
POIS, NB, LSIG = 24, 25, 26  # walnuts_amd.MODEL_POISSON_REGRESSION / _NEG_BINOMIAL_REGRESSION / _LINEAR_REGRESSION_SIGMA

# The maths functions' stated accuracy, measured worst cases in brackets:
#   dlog1p, dsoftplus: relative, C_REL u (2 u)
#   dlgamma_diff: C_GAMMA u * A_lg(y, phi),  A_lg = y (|log(phi + y)| + 1) + |log phi| + 1   (4.7 u)
#   ddigamma_diff: C_GAMMA u * A_dg(y, phi), A_dg = g + [phi < 16] (1 / phi + log1p(15 / phi)), g the exact value (5.0 u)
C_REL = 4
C_GAMMA = 16
# the rounding of the count models' own row arithmetic, the maths functions inside it and the scale exp(s) (few u):
# ulps per row term, on top of the reduction depths of hp_reference.glm_bound
C_COUNT = 48


def abs_lgamma_diff(y, phi):
    return y * (abs(math.log(phi + y)) + 1.0) + abs(math.log(phi)) + 1.0


def abs_digamma_diff(g, phi):
    return g + ((1.0 / phi + math.log1p(15.0 / phi)) if phi < 16.0 else 0.0)


def _dps(y, phi):
    """digits that keep the difference of two lgamma / digamma values exact: both grow like (y + phi) log(y + phi)"""
    return DPS + int(max(0.0, math.log10(max(float(phi), 1.0) + float(y))))


def lgamma_diff(y, phi):
    """exact lgamma(y + phi) - lgamma(phi) (an mpf)"""
    with mp.workdps(_dps(y, phi)):
        P, Y = mp.mpf(float(phi)), mp.mpf(float(y))
        return mp.loggamma(Y + P) - mp.loggamma(P)


def digamma_diff(y, phi):
    with mp.workdps(_dps(y, phi)):
        P, Y = mp.mpf(float(phi)), mp.mpf(float(y))
        return mp.digamma(Y + P) - mp.digamma(P)


def split(theta, model):
    th = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    if model == POIS:
        return th, np.zeros(th.shape[0])
    return th[:, :-1], th[:, -1]


def count_reference(model, x, y, mp_params, theta):
    """(lp, g, lp_abs, g_abs) [C], [C, D] for one of the three flat models; x has the model's P columns and
    mp_params the user's model_params (prior variances, then sigma_0 for the scale models)."""
    beta, s = split(theta, model)
    C, P = beta.shape
    N = len(y)
    ld = np.longdouble
    X, B = np.asarray(x, dtype=ld), beta.astype(ld)
    ETA = B @ X.T  # [C, N]
    A = np.abs(B) @ np.abs(X).T
    s2 = np.asarray(mp_params[:P], dtype=np.float64)
    lp, lpa = np.zeros(C), np.zeros(C)
    g = np.zeros((C, beta.shape[1] + (0 if model == POIS else 1)))
    ga = np.zeros_like(g)
    with mp.workdps(DPS + 20 + int(max(0.0, float(np.max(np.abs(s))) / 2.3))):
        for c in range(C):
            S = mp.mpf(float(s[c]))
            phi = mp.exp(-S)
            isig2 = mp.exp(-2 * S)
            ll, lla, dsum, dsa = [], [], [], []
            r_all, ra_all = [], []
            for n in range(N):
                hi = float(ETA[c, n])
                eta = mp.mpf(hi) + mp.mpf(float(ETA[c, n] - ld(hi)))  # (the long double, exactly)
                Yn = mp.mpf(float(y[n]))
                An = float(A[c, n])
                if model == POIS:
                    mu = mp.exp(eta)
                    r = Yn - mu
                    l = Yn * eta - mu
                    l_abs = abs(Yn * eta) + mu
                    slope = mu  # |dr / deta|
                    r_abs = Yn + mu  # (the absolute version of r's own computation)
                    ds = ds_abs = dslope = mp.mpf(0)
                elif model == NB:
                    t = eta + S
                    sp = mp.log1p(mp.exp(t))
                    sig = 1 / (1 + mp.exp(-t))
                    lg = mp.loggamma(Yn + phi) - mp.loggamma(phi)
                    dg = mp.digamma(Yn + phi) - mp.digamma(phi)
                    r = Yn - (Yn + phi) * sig
                    l = lg + Yn * t - (Yn + phi) * sp
                    fphi = float(phi)
                    lg_abs = abs_lgamma_diff(float(Yn), fphi) if math.isfinite(fphi) and fphi > 0 else mp.inf
                    dg_abs = abs_digamma_diff(float(dg), fphi) if math.isfinite(fphi) and fphi > 0 else mp.inf
                    l_abs = lg_abs + abs(Yn * t) + (Yn + phi) * sp + phi * (sp + dg_abs)
                    slope = abs(Yn - r)
                    r_abs = Yn + (Yn + phi) * sig
                    ds = r + phi * (sp - dg)
                    ds_abs = Yn + (Yn + phi) * sig + phi * (sp + dg_abs) + Yn
                    dslope = slope + mp.exp(eta)
                else:
                    d = Yn - eta
                    r = d * isig2
                    l = -d * d * isig2 / 2 - S
                    l_abs = d * d * isig2 / 2 + abs(S)
                    slope = isig2
                    r_abs = abs(r)
                    ds = d * d * isig2 - 1
                    ds_abs = d * d * isig2 + 1
                    dslope = 2 * abs(r)
                ll.append(l)
                lla.append(l_abs + abs(r) * An)
                r_all.append(r)
                ra_all.append(r_abs + slope * An)
                dsum.append(ds)
                dsa.append(ds_abs + dslope * An)
            prior = sum(mp.mpf(float(b)) ** 2 / (2 * mp.mpf(float(v))) for b, v in zip(beta[c], s2))
            lpc = mp.fsum(ll) - prior
            lpac = mp.fsum(lla) + prior
            if model != POIS:
                tt = mp.exp(2 * S) / mp.mpf(float(mp_params[-1])) ** 2
                lpc += S - tt / 2
                lpac += abs(S) + tt / 2
                g[c, -1] = float(mp.fsum(dsum) + 1 - tt)
                ga[c, -1] = float(mp.fsum(dsa) + 1 + tt)
            lp[c], lpa[c] = float(lpc), float(lpac)
            for j in range(P):
                col = [mp.mpf(float(v)) for v in x[:, j]]
                g[c, j] = float(mp.fsum(cv * r for cv, r in zip(col, r_all)) - mp.mpf(float(beta[c, j])) / mp.mpf(float(s2[j])))
                ga[c, j] = float(mp.fsum(abs(cv) * ra for cv, ra in zip(col, ra_all)) + abs(float(beta[c, j])) / s2[j])
    return lp, g, lpa, ga


def count_bound(lpa, ga, N, epl):
    """glm_bound's depths (hp_reference.py) with C_COUNT for the row arithmetic; the s gradient's lane sum (cx.sum1)
    and the scale's prior terms fit in the same K."""
    B = block_rows(epl)
    k_lp = -(-N // B) + epl + 6 + 6 + 4 + C_COUNT
    k_g = N + 2 + epl + 6 + 6 + C_COUNT
    return k_lp * U * np.asarray(lpa), k_g * U * np.asarray(ga)


def count_case(model, x, y, mp_params, theta, epl):
    lp, g, lpa, ga = count_reference(model, x, y, mp_params, theta)
    blp, bg = count_bound(lpa, ga, len(y), epl)
    return lp, g, blp, bg


def numpy_logp_grad(model, x, y, mp_params, theta):
    """float64 NumPy restatement: lgamma and digamma differences as the sums sum_k log(phi + k) and sum_k 1 / (phi + k)
    over k < y (small counts only)."""
    beta, s = split(theta, model)
    P = beta.shape[1]
    eta = beta @ np.asarray(x).T
    Y = np.asarray(y, dtype=np.float64)
    s2 = np.asarray(mp_params[:P])
    prior = (beta * beta / (2 * s2)).sum(1)
    gb = -beta / s2
    if model == POIS:
        mu = np.exp(eta)
        r = Y - mu
        return (Y * eta - mu).sum(1) - prior, r @ x + gb
    if model == NB:
        phi = np.exp(-s)[:, None]
        t = eta + s[:, None]
        sp = np.logaddexp(0.0, t)
        sig = 1.0 / (1.0 + np.exp(-t))
        ymax = int(Y.max()) if Y.size else 0
        ks = np.arange(ymax)
        mask = ks[None, :] < Y[:, None]  # [N, ymax]
        lg = np.where(mask[None], np.log(phi[:, :, None] + ks), 0.0).sum(-1)
        dg = np.where(mask[None], 1.0 / (phi[:, :, None] + ks), 0.0).sum(-1)
        r = Y - (Y + phi) * sig
        ll = lg + Y * t - (Y + phi) * sp
        ds = (r + phi * (sp - dg)).sum(1)
    else:
        isig2 = np.exp(-2 * s)[:, None]
        d = Y - eta
        r = d * isig2
        ll = -0.5 * d * d * isig2 - s[:, None]
        ds = (d * d * isig2 - 1).sum(1)
    tt = np.exp(2 * s) / mp_params[-1] ** 2
    lp = ll.sum(1) - prior + s - tt / 2
    g = np.concatenate([r @ x + gb, (ds + 1 - tt)[:, None]], axis=1)
    return lp, g
