"""The posterior summaries in exact arithmetic, with derived bounds on the device's rounding error.  TEST HELPER.

A restatement of the DEFINITIONS behind include/walnutpie/summary.hpp (mean, sample variance and standard deviation,
per-chain biased autocovariance at every lag, R-hat, effective sample size, MCSE, quantiles), not of the device's
operation order: every finite double is an exact rational, so the sums over draws run in scaled Python integers and
everything above them in `fractions.Fraction`; mpmath (PREC bits) serves only the square roots and log10.

Every result is an `Fl`: the exact value `v` and a bound `e` on |device - v|.  The bounds are DERIVED, from the
operation counts of the device's documented order (left-to-right sums over the draws of a chain, runs of 256 chains,
then the run totals) with u = 2^-53, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of
Numerical Algorithms, §3.1, §4.2), and eta = 2^-1075 for a product or quotient that may round in the subnormal range.
No constant is fitted.

Sums over draws (closed forms; N draws, or n of one chain, in all):
  mean      every term passes through at most N roundings (N - 1 additions in whatever grouping, one division):
                |mean^ - mean| <= gamma_N * sum|x| / N                                                    =: em
  variance  two passes.  With d_i = x_i - mean^ (the ROUNDED mean), sum d_i^2 = sum (x_i - mean)^2 + N (mean - mean^)^2
            exactly, and a term d_i^2 passes through at most N + 3 roundings (subtraction, square, N - 1 additions,
            division; counted as N + 3):
                |var^ - var| <= gamma_{N+3} * (var + X) + X + (N + 1) eta,      X = N em^2 / (N - 1)
  autocovariance of one chain at lag t, m = n - t terms, y_i = x_i - ybar:  with eps = ybar - ybar^, |eps| <= em,
            sum d_i d_{i+t} = sum y_i y_{i+t} + eps * sum (y_i + y_{i+t}) + m eps^2, and a term passes through at most
            m + 3 roundings (two subtractions, product, m - 1 additions, division):
                |a^_t - a_t| <= ( gamma_{m+3} * (sum|y_i y_{i+t}| + em * sum(|y_i| + |y_{i+t}|) + m em^2)
                                  + em * |sum (y_i + y_{i+t})| + m em^2 ) / n + (m + 1) eta
Everything above the draws (sums over chains, R-hat, rho, tau, ESS, MCSE, the quantile's interpolation) is propagated
operation by operation by `Fl`'s arithmetic: for computed operands a^, b^ within ea, eb of a, b,
  a^ (+-) b^   p = ea + eb;                                    e = p + u (|v| + p)
  a^ * b^      p = |a| eb + |b| ea + ea eb;                    e = p + u (|v| + p) + eta
  a^ / b^      p = (ea + |v| eb) / (|b| - eb)  (|b| > eb);     e = p + u (|v| + p) + eta
  sqrt(a^)     p = ea / sqrt(a)  (a - ea >= 0, a > 0);         e = p + u (|v| + p)        (correctly rounded)
and e is infinite (no claim) where a divisor's or a radicand's interval reaches zero.  Adding an exact zero is exact.
tau's floor 1 / log10(N) comes from libm: glibc documents log10 within 2 ulp (4u relative), the division adds u: 5u.
Bounds are rounded UP to 64 significant bits after every operation to keep the rationals short.
"""
import math
from fractions import Fraction as F

import mpmath as mp
import numpy as np

PREC = 400
U = F(1, 2 ** 53)
ETA = F(1, 2 ** 1075)
INF = float("inf")
CHAIN_BLOCK = 256
MP_SLACK = F(1, 2 ** 300)   # relative error of an mpmath value at PREC bits, generously


def gamma(n):
    return n * U / (1 - n * U)


def _up(e):
    """e rounded up to 64 significant bits"""
    if e == 0 or e == INF:
        return e
    k = e.numerator.bit_length() - e.denominator.bit_length() - 65
    return F(-((-e.numerator) // (e.denominator << k)), 1) * (1 << k) if k >= 0 else \
        F(-((-(e.numerator << -k)) // e.denominator), 1 << -k)


def _mp_to_fraction(r):
    sign, man, exp, _ = r._mpf_
    f = F(int(man)) * (F(2) ** int(exp))
    return -f if sign else f


def _to_mp(f):
    return mp.mpf(f.numerator) / mp.mpf(f.denominator)


class Fl:
    """exact value v; e bounds |what the device computed - v|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0):
        self.v = v if isinstance(v, F) else F(v)
        self.e = e

    @staticmethod
    def _mk(v, p, under=False):
        if p == INF:
            return Fl(v, INF)
        return Fl(v, _up(p + U * (abs(v) + p) + (ETA if under else 0)))

    def __add__(a, b):
        b = _fl(b)
        if b.v == 0 and b.e == 0:
            return a
        if a.v == 0 and a.e == 0:
            return b
        return Fl._mk(a.v + b.v, INF if INF in (a.e, b.e) else a.e + b.e)

    def __sub__(a, b):
        b = _fl(b)
        if b.v == 0 and b.e == 0:
            return a
        return Fl._mk(a.v - b.v, INF if INF in (a.e, b.e) else a.e + b.e)

    def __mul__(a, b):
        b = _fl(b)
        p = INF if INF in (a.e, b.e) else abs(a.v) * b.e + abs(b.v) * a.e + a.e * b.e
        return Fl._mk(a.v * b.v, p, under=True)

    def __truediv__(a, b):
        b = _fl(b)
        if INF in (a.e, b.e) or abs(b.v) <= b.e:
            return Fl(a.v / b.v if b.v != 0 else F(0), INF)
        v = a.v / b.v
        return Fl._mk(v, (a.e + abs(v) * b.e) / (abs(b.v) - b.e), under=True)

    __radd__ = __add__

    def __rsub__(a, b):
        return _fl(b) - a

    def __rmul__(a, b):
        return _fl(b) * a

    def __rtruediv__(a, b):
        return _fl(b) / a

    def sqrt(a):
        with mp.workprec(PREC):
            s = _mp_to_fraction(mp.sqrt(_to_mp(max(a.v, F(0)))))
        if a.e == INF or a.v - a.e < 0 or (a.v == 0 and a.e != 0):
            return Fl(s, INF)
        if a.v == 0:
            return Fl(0, 0)
        p = a.e / (s * (1 - MP_SLACK))
        return Fl(s, _up(p + U * (s + p) + s * MP_SLACK))

    def __repr__(self):
        return f"Fl({float(self.v)!r} +- {float(self.e):.3e})"


def _fl(x):
    return x if isinstance(x, Fl) else Fl(x)


def ratio(got, want):
    """|got - want.v| / want.e for a device double `got`: the test's figure of merit, <= 1 required.  0 where the
    bound makes no claim (infinite), infinite for a non-finite device value or a miss of an exact value."""
    if want.e == INF:
        return 0.0
    if not math.isfinite(got):
        return INF
    diff = abs(F(float(got)) - want.v)
    if diff == 0:
        return 0.0
    return INF if want.e == 0 else float(diff / want.e)


def chain_sum(terms):
    """sum over chains as the device groups it: runs of 256 left to right, then the run totals left to right"""
    total = Fl(0)
    for b0 in range(0, len(terms), CHAIN_BLOCK):
        s = Fl(0)
        for t in terms[b0:b0 + CHAIN_BLOCK]:
            s = s + t
        total = total + s
    return total


def _scaled(xs):
    """finite doubles -> (integers X, s) with x = X / 2^s"""
    rats = [float(x).as_integer_ratio() for x in xs]
    s = max(den.bit_length() - 1 for _, den in rats)
    return [num << (s - (den.bit_length() - 1)) for num, den in rats], s


class Column:
    """every summary of one column of ragged chains (a list of 1-d arrays), exact, with the device's error bounds"""

    def __init__(self, chains):
        lens = [len(c) for c in chains]
        X, s = _scaled([x for c in chains for x in c])
        self.products = 0
        self.lens = lens
        self.C = C = len(chains)
        self.N = N = sum(lens)
        self.min_len = min(lens)
        self.flat = [float(x) for c in chains for x in c]
        two_s = 1 << s
        # mean and sample variance over all draws
        S = sum(X)
        em = gamma(N) * F(sum(abs(x) for x in X), N * two_s)
        self.mean = Fl(F(S, N * two_s), _up(em))
        q = sum((N * x - S) ** 2 for x in X)
        self.products += N
        self.var = self._var(F(q, N * N * two_s * two_s * (N - 1)), N, em)
        self.sd = self.var.sqrt()
        # per chain: mean, sample variance, biased autocovariance at every lag
        self.cmean, self.cvar, self.acov = [], [], []
        at = 0
        for n in lens:
            Xc = X[at:at + n]
            at += n
            Sc = sum(Xc)
            k = n * two_s                                   # y_i = Y_i / k
            emc = gamma(n) * F(sum(abs(x) for x in Xc), k)
            self.cmean.append(Fl(F(Sc, k), _up(emc)))
            Y = [n * x - Sc for x in Xc]
            absY = [abs(y) for y in Y]
            lags = []
            for t in range(n):
                m = n - t
                prods = [Y[i] * Y[i + t] for i in range(m)]
                self.products += m
                a = F(sum(prods), k * k * n)
                A = F(sum(abs(p) for p in prods), k * k)
                B = F(sum(absY[:m]) + sum(absY[t:]), k)
                Sg = F(abs(sum(Y[:m]) + sum(Y[t:])), k)
                e = (gamma(m + 3) * (A + emc * B + m * emc * emc) + emc * Sg + m * emc * emc) / n + (m + 1) * ETA
                lags.append(Fl(a, _up(e)))
            self.acov.append(lags)
            assert n >= 2
            self.cvar.append(self._var(lags[0].v * n / (n - 1), n, emc))
        # R-hat and the ESS's variances (summary.hpp's W and var_plus)
        self.W = chain_sum(self.cvar) / C
        if C > 1:
            mu = chain_sum(self.cmean) / C
            self.between = chain_sum([(m - mu) * (m - mu) for m in self.cmean]) / (C - 1)
            self.r_hat = (1 + self.between / self.W).sqrt()
            self.var_plus = self.W + self.between
        else:
            self.between = self.r_hat = None
            self.var_plus = self.W
        self.macov = [chain_sum([a[t] for a in self.acov]) / C for t in range(self.min_len)]
        self._ess()
        self.mcse = self.sd / self.ess.sqrt()

    @staticmethod
    def _var(v, n, em):
        if em == INF:
            return Fl(v, INF)
        X = n * em * em / (n - 1)
        return Fl(v, _up(gamma(n + 3) * (v + X) + X + (n + 1) * ETA))

    def _ess(self):
        """Geyer's initial positive and monotone sequence on paired lags, evaluated exactly; `margins` holds, for every
        branch taken, (name, lag, |exact tested quantity - threshold|, bound on the device's error in that quantity)"""
        W, vp, macov, min_len, N = self.W, self.var_plus, self.macov, self.min_len, self.N
        self.margins = margins = []

        def rho_at(t):
            return 1 - (W - macov[t]) / vp

        zero = Fl(0)
        R = [zero] * min_len
        even = Fl(1)
        R[0] = even
        odd = rho_at(1)
        R[1] = odd
        t = 1
        while t < min_len - 4:
            s = even + odd
            margins.append(("positive", t, abs(s.v), s.e))
            if not s.v > 0:
                break
            even, odd = rho_at(t + 1), rho_at(t + 2)
            s = even + odd
            margins.append(("non-negative", t, abs(s.v), s.e))
            if s.v >= 0:
                R[t + 1], R[t + 2] = even, odd
            a, b = R[t + 1] + R[t + 2], R[t - 1] + R[t]
            margins.append(("monotone", t, abs(a.v - b.v), INF if INF in (a.e, b.e) else a.e + b.e))
            if a.v > b.v:
                R[t + 1] = b / 2
                R[t + 2] = R[t + 1]
            t += 2
        self.max_t = max_t = t
        margins.append(("tail", t, abs(even.v), even.e))
        if even.v > 0:
            R[max_t + 1] = even
        head = Fl(0)
        for i in range(max_t):
            head = head + R[i]
        tau = (-1 + 2 * head) + R[max_t + 1]
        with mp.workprec(PREC):
            fv = _mp_to_fraction(1 / mp.log10(N))
        floor = Fl(fv, _up(5 * U * fv))
        margins.append(("floor", t, abs(tau.v - floor.v), INF if tau.e == INF else tau.e + floor.e))
        self.rho = R
        self.tau = floor if tau.v < floor.v else tau
        self.ess = N / self.tau
        self.near_tie = any(margin < bound for _, _, margin, bound in margins)

    def quantile(self, p):
        """h = p (N - 1), floor(h) and frac in double as the reference states them (summary.hpp:507-511); the order
        statistics from an exact sort; the interpolation exact, the bound from the device's three operations"""
        srt = sorted(self.flat)
        h = float(p) * float(self.N - 1)
        lo = int(math.floor(h))
        hi = min(lo + 1, self.N - 1)
        frac = h - float(lo)
        return Fl(F(srt[lo])) + Fl(F(frac)) * (Fl(F(srt[hi])) - Fl(F(srt[lo])))


def columns(chains):
    """[Column] for a list of [n_m, D] arrays"""
    chains = [np.asarray(c, dtype=np.float64) for c in chains]
    return [Column([c[:, d] for c in chains]) for d in range(chains[0].shape[1])]
