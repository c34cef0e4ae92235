"""High-precision reference for the predictions of the data models (walnuts_amd/csrc/wn_predict.h), in the style of
hp_pointwise_reference.py: everything in mpmath at DPS digits from the float64 inputs, and bounds that are K * u * the
absolute version of the computation, K counted from the kernel's order of operations.

    eta_n = fsum_j x_nj beta_j (+ v_{g(n)}) + o_n,      A_n = sum_j |x_nj beta_j| (+ |v_{g(n)}|) + |o_n|
    mu_n  = E[y | theta, x_n],   v_n = Var[y | theta, x_n]   (the table of wn_predict.h, evaluated exactly)

ETA.  K_ETA counts eta as hp_pointwise_reference.k_entry does, without the link and the constant:
    slot-order multiply-adds and the packed butterfly, depth EPL + 6; + 1 for the add of the offset; hierarchical
    models: + 1 for the add of the group effect, whose value tau * z_g carries the K_TAU roundings of dexp(s) and one
    product: + K_TAU + 1.                               |eta_device - eta| <= K_ETA u A_n

MU and V.  A value f(eta) computed from the device's eta carries |f'(eta)| |d eta| plus the roundings of its own
evaluation, relative to the value: the absolute version is |f| + |f'| A_n and K = K_ETA + the link's own depth.  With
C_EXP = 4 (one wnd::dexp: 2 ulp <= 4 u, hp_math_reference.py) the depths are:
    identity     mu = eta: no operation, depth 0 (f' = 1, so the bound is eta's);  v = 1 exactly: bound 0.
    sigma        mu = eta: depth 0;  v = scale * scale, scale = dexp(s) of the exact input s: each factor C_EXP, one
                 rounded product: K_SCALE_SQ = 2 C_EXP + 1 = 9, absolute version exp(2 s), no eta in it.
    logit        mu: e = dexp(-|eta|), d = 1 / (1 + e), mu = d or e * d -- the operations LogitLink::term performs for
                 its residual, so C_LINK = 16 (hp_reference.py) is used; counted directly: e is C_EXP, d adds the rounded
                 sum and the division to e's error attenuated by e / (1 + e) <= 1: C_EXP + 2, e * d one more product:
                 2 C_EXP + 3 = 11 <= C_LINK.  f' = mu (1 - mu).
                 v = (e * d) * d: e * d is 2 C_EXP + 3 as above, the second d adds C_EXP + 2 and the product 1:
                 K_LOGIT_V = 3 C_EXP + 6 = 18.  f' = v (1 - 2 mu).
    log          mu = dexp(eta): C_EXP;  v = mu: the same value.  f' = mu.
    negbin       mu = dexp(eta): C_EXP;  v = mad(kappa * mu, mu, mu), kappa = dexp(s): kappa * mu is C_EXP + C_EXP + 1,
                 the multiply-add rounds its product (when not fused) and its sum, and multiplies by mu once more:
                 + C_EXP + 2: K_NB_V = 3 C_EXP + 3 = 15 relative to v = mu + kappa mu^2 (all terms positive: v is its own
                 absolute version).  f' = mu + 2 kappa mu^2.
K multiplies the whole absolute version (a bound for the sum of the parts' own counts), as in k_entry.  Nothing here was
tuned to an observed error.  Entries that are not finite (an overflowing Poisson link: mu = v = inf) are compared for
non-finiteness, not against a bound.

THE FOLD is replayed exactly by the tests (wn_predict.h states it); welford_mean_bound is the counted bound of the
Welford mean against a mean computed otherwise, 4 (T + C) u max|q| (hp_pointwise_reference.py, "mean").

sensitivity() says how far outside the entry bounds four mistakes land: the offset dropped, the group effect of the
neighbouring group, mu returned for eta, the weights applied (w_n mu_n for mu_n)."""
import math

import mpmath as mp
import numpy as np

import hp_weighted_reference as hw
from hp_pointwise_reference import C_EXP
from hp_reference import C_LINK, U

DPS = 60
K_SCALE_SQ = 2 * C_EXP + 1
K_LOGIT_V = 3 * C_EXP + 6
K_NB_V = 3 * C_EXP + 3
NAMES = ("eta", "mu", "v")


def k_eta(model, epl):
    k = epl + 6 + 1
    if model in hw.HIER:
        k += 1 + hw.K_TAU + 1
    return k


def link_depth(fam):
    """(depth of mu, depth of v) on top of K_ETA"""
    return {"identity": (0, 0), "sigma": (0, K_SCALE_SQ), "logit": (C_LINK, K_LOGIT_V), "log": (C_EXP, C_EXP),
            "negbin": (C_EXP, K_NB_V)}[fam]


def _response(fam, eta, S):
    """(mu, mu', v, |v|_abs, v') exactly; primes are derivatives with respect to eta"""
    one, zero = mp.mpf(1), mp.mpf(0)
    if fam == "identity":
        return eta, one, one, zero, zero
    if fam == "sigma":
        return eta, one, mp.exp(2 * S), mp.exp(2 * S), zero
    if fam == "logit":
        mu = 1 / (1 + mp.exp(-eta))
        v = mp.exp(-abs(eta)) / (1 + mp.exp(-abs(eta))) ** 2
        return mu, v, v, v, v * (1 - 2 * mu)
    mu = mp.exp(eta)
    if fam == "log":
        return mu, mu, mu, mu, mu
    kappa = mp.exp(S)
    v = mu + kappa * mu * mu
    return mu, mu, v, v, mu + 2 * kappa * mu * mu


def _f(v):
    """mpf -> float64, overflow to inf"""
    return float(v) if abs(v) < mp.mpf(2) ** 1024 else math.copysign(math.inf, v)


def reference(model, x, theta, epl, offset=None, group=None):
    """dict(eta, mu, v: float64 [T, N], rounded once from the exact values; eta_bound, mu_bound, v_bound: [T, N])"""
    fam = hw.family(model)
    th_all = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    T, D = th_all.shape
    N, P = x.shape
    hier = model in hw.HIER
    scale = fam in ("negbin", "sigma")
    J = D - P - 1 if hier else 0
    ke = k_eta(model, epl)
    kmu, kv = (ke + d for d in link_depth(fam))
    if fam == "sigma":
        kv = K_SCALE_SQ   # (no eta in scale * scale)
    m = lambda a: mp.mpf(float(a))  # noqa: E731
    out = {k: np.empty((T, N)) for k in ("eta", "mu", "v", "eta_bound", "mu_bound", "v_bound")}
    with mp.workdps(DPS):
        X = [[m(a) for a in row] for row in x]
        O = [m(a) for a in offset] if offset is not None else [mp.mpf(0)] * N
        for t in range(T):
            th = [m(a) for a in th_all[t]]
            s = th[D - 1] if (hier or scale) else mp.mpf(0)
            tau = mp.exp(s)
            if hier:
                ge = [th[P + j] if model in hw.CENTERED else tau * th[P + j] for j in range(J)]
            for n in range(N):
                prods = [X[n][j] * th[j] for j in range(P)]
                vg = ge[int(group[n])] if hier else mp.mpf(0)
                eta = mp.fsum(prods) + vg + O[n]
                A = mp.fsum(abs(p) for p in prods) + abs(vg) + abs(O[n])
                mu, dmu, v, va, dv = _response(fam, eta, s)
                bounds = (ke * U * A, kmu * U * (abs(mu) + abs(dmu) * A), kv * U * (va + abs(dv) * A))
                for name, val, b in zip(NAMES, (eta, mu, v), bounds):
                    out[name][t, n] = _f(val)
                    out[name + "_bound"][t, n] = _f(b)
    return out


def error_ratio(values, ref):
    """max |value - reference| / bound over the finite entries of (eta, mu, v); the others must agree on
    non-finiteness exactly.  An entry whose bound is 0 (identity v = 1) must be exact."""
    worst = 0.0
    for name, got in zip(NAMES, values):
        got = np.asarray(got)
        fin = np.isfinite(ref[name])
        assert np.array_equal(np.isfinite(got), fin), f"device and reference disagree on which entries of {name} are finite"
        assert np.array_equal(got[~fin], ref[name][~fin], equal_nan=True), name
        if fin.any():
            worst = max(worst, float((np.abs(got[fin] - ref[name][fin]) / np.maximum(ref[name + "_bound"][fin], 1e-300)).max()))
    return worst


def sensitivity(model, x, theta, epl, ref, offset=None, group=None, weights=None, num_groups=None):
    """The smallest distance, in entry bounds, between `ref` and what each mistake would have produced -- each only
    where it applies: the offset dropped; every row given the effect of the neighbouring group (g + 1 mod J); mu
    returned for eta (links other than the identity); the weights applied (w_n mu_n for mu_n)."""
    def dist(name, wrong):
        fin = np.isfinite(ref[name]) & np.isfinite(ref[name + "_bound"]) & np.isfinite(wrong)
        d = np.abs(wrong[fin] - ref[name][fin]) / np.maximum(ref[name + "_bound"][fin], 1e-300)
        return float(d.max()) if d.size else math.inf

    def dist_all(other):   # the output a mistake moves least decides whether a test of all three sees it
        return max(dist(name, other[name]) for name in NAMES)

    worst = math.inf
    if offset is not None and np.any(offset != 0):
        worst = min(worst, dist_all(reference(model, x, theta, epl, None, group)))
    if model in hw.HIER:
        worst = min(worst, dist_all(reference(model, x, theta, epl, offset, (np.asarray(group) + 1) % num_groups)))
    if hw.family(model) not in ("identity", "sigma"):
        worst = min(worst, dist("eta", ref["mu"]))
    if weights is not None and not np.all((weights == 1) | (weights == 0)):
        worst = min(worst, dist("mu", ref["mu"] * np.asarray(weights)[None, :]))
    return worst


def welford_mean_bound(T, C, values):
    """4 (T + C) u max|q|: the Welford update and the pairwise merge round 4 operations per draw / chain"""
    return 4 * (T + C) * U * np.abs(np.asarray(values)).max(axis=0)


def replay_fold(eta_chains, mu_chains, v_chains):
    """The fold wn_predict.h states, in plain Python floats (IEEE double, every operation rounded once), on the [len][N]
    matrices of each chain in chain order -> (eta_mean, eta_var, mean, mean_var, noise_var, count), [N] each."""
    N = np.asarray(eta_chains[0]).shape[1]
    outs = [np.empty(N) for _ in range(5)]
    count = np.empty(N, dtype=np.int64)
    for r in range(N):
        state = None
        for E, M, V in zip(eta_chains, mu_chains, v_chains):
            a = [0.0] * 5
            for i in range(len(E)):
                n = float(i + 1)
                for k, q in ((0, float(E[i][r])), (2, float(M[i][r]))):
                    d = q - a[k]
                    a[k] = a[k] + d / n
                    a[k + 1] = a[k + 1] + d * (q - a[k])
                a[4] = a[4] + (float(V[i][r]) - a[4]) / n
            nb = float(len(E))
            if state is None:
                state = (nb, a)
                continue
            na, s = state
            nn = na + nb
            w, cross = nb / nn, na * nb / nn
            for k in (0, 2):
                d = a[k] - s[k]
                s[k] = s[k] + d * w
                s[k + 1] = (s[k + 1] + a[k + 1]) + (d * d) * cross
            s[4] = s[4] + (a[4] - s[4]) * w
            state = (nn, s)
        n, s = state
        outs[0][r], outs[2][r], outs[4][r] = s[0], s[2], s[4]
        outs[1][r] = s[1] / (n - 1.0) if n >= 2 else math.nan
        outs[3][r] = s[3] / (n - 1.0) if n >= 2 else math.nan
        count[r] = int(n)
    return tuple(outs) + (count,)
