"""References for the simulated replicates (walnuts_amd/csrc/wn_devrand.h, wn_replicate.h).

1. The samplers RESTATED in Python from the header's description, independently of the C++: each is fed the uniforms of
   the stated counter layout -- hp_math_reference.philox4x32 and uniform_of under (row, draw, chain, 4 + 256 * call) --
   and evaluates math.exp / math.log / math.lgamma where the device evaluates dexp / dlog / dlgamma_diff; every other
   step is the header's plain binary64 operation in the header's order, so the replay decides as the device decides
   unless a comparison is a NEAR TIE: its two sides within 1e-9 relative, or a floor argument within 1e-9 of an integer.
   Such a case is marked and set aside by the caller (at most 1 in 10 000).
   The Box-Muller normals are the library's own stream_normal_pair on the same counters (wn_internal_stream_probe, whose
   bits tests/test_devmath_sim.py holds against mpmath): a gamma variate d * v is a function of that normal alone, so
   an unboosted gamma is compared bit for bit; a boosted one carries dexp / dlog against math.exp / math.log
   (boost_bound_u).
2. The check's reduction replayed in Python floats: lane-major accumulation over tiles, then wave_sum's butterfly.
3. Binned chi-square against scipy.stats pmfs."""
import ctypes as C
import math

import numpy as np

import hp_math_reference as hm

NORMAL, BERNOULLI, POISSON, GAMMA, NEGBIN = range(5)
ARRAY, GATHER = 0, 2
STREAM_REPLICATE = 4
POISSON_SPLIT = 10.0
POISSON_MU_MAX = 2.0 ** 30
SEARCH_CAP = 64
REJECTION_CAP = 32
THIRD = 1.0 / 3.0   # RN(1/3)
TIE = 1e-9
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def sampler_probe(lib, kind, mu, shape, seed, chain, draw, row0, tab=ARRAY):
    """(samples [n], calls [n]) of wn_internal_sampler_probe: argument i on the stream of row row0 + i"""
    mu = np.ascontiguousarray(mu, dtype=np.float64)
    shape = np.ascontiguousarray(np.broadcast_to(np.asarray(shape, dtype=np.float64), mu.shape))
    out = np.empty(mu.size)
    calls = np.empty(mu.size, dtype=np.intc)
    rc = lib.wn_internal_sampler_probe(kind, mu.ctypes.data_as(_dp), shape.ctypes.data_as(_dp), seed, chain, draw, row0,
                                       mu.size, tab, out.ctypes.data_as(_dp), calls.ctypes.data_as(_ip))
    assert rc == 0, rc
    return out, calls


class Streams:
    """the counter streams of rows row0 .. row0 + n - 1 of one (seed, chain, draw): call index -> arrays over the rows"""

    def __init__(self, lib, seed, chain, draw, row0, n):
        self.lib, self.seed, self.chain, self.draw, self.row0, self.n = lib, seed, chain, draw, row0, n
        self._u, self._z = {}, {}

    def uniforms(self, call):
        if call not in self._u:
            k1, k2 = hm.stream_integers(self.seed, self.chain, self.draw, STREAM_REPLICATE + 256 * call, self.row0, self.n)
            self._u[call] = (hm.uniform_of(k1), hm.uniform_of(k2))
        return self._u[call]

    def normal(self, call):
        if call not in self._z:
            self._z[call] = hm.stream_probe(self.lib, self.seed, self.chain, self.draw, STREAM_REPLICATE + 256 * call,
                                            self.row0, self.n, True)[0]
        return self._z[call]


def _close(a, b):
    return abs(a - b) <= TIE * max(abs(a), abs(b), 1e-300)


def poisson(mu, st, i, call):
    """-> (y, call, near tie)"""
    if not (mu >= 0.0 and mu <= POISSON_MU_MAX):
        return math.nan, call, False
    if mu == 0.0:
        return 0.0, call, False
    near = False
    if mu < POISSON_SPLIT:
        u = float(st.uniforms(call)[0][i])
        call += 1
        p = math.exp(-mu)
        cdf, k = p, 0
        while True:
            near = near or _close(u, cdf)
            if not (u > cdf and k < SEARCH_CAP):
                break
            k += 1
            p = (p * mu) / k
            cdf = cdf + p
        return float(k), call, near
    smu, lmu = math.sqrt(mu), math.log(mu)
    b = 0.931 + 2.53 * smu
    a = -0.059 + 0.02483 * b
    inva = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    linva = math.log(inva)
    for _ in range(REJECTION_CAP):
        u, V = (float(w[i]) for w in st.uniforms(call))
        call += 1
        U = u - 0.5
        us = 0.5 - abs(U)
        arg = (((2.0 * a) / us + b) * U + mu) + 0.43
        k = math.floor(arg)
        near = near or abs(arg - round(arg)) <= TIE
        if k >= 0 and us >= 0.07 and V <= vr:
            return float(k), call, near
        if k < 0 or (us < 0.013 and V > us):
            continue
        lhs = (math.log(V) + linva) - math.log(a / (us * us) + b)
        rhs = (k * lmu - mu) - math.lgamma(k + 1.0)
        near = near or _close(lhs, rhs)
        if lhs <= rhs:
            return float(k), call, near
    return math.nan, call, near


def gamma(shape, st, i, call):
    """-> (G, call, near tie, boosted)"""
    if not (shape > 0.0 and shape < math.inf):
        return math.nan, call, False, False
    boost = shape < 1.0
    d0 = shape + 1.0 if boost else shape
    d = d0 - THIRD
    c = 1.0 / math.sqrt(9.0 * d)
    g, near = math.nan, False
    for _ in range(REJECTION_CAP):
        z = float(st.normal(call)[i])
        u = float(st.uniforms(call + 1)[0][i])
        call += 2
        t = 1.0 + c * z
        v = (t * t) * t
        if not v > 0.0:
            continue
        lhs = math.log(u)
        rhs = (((0.5 * z) * z + d) - d * v) + d * math.log(v)
        near = near or _close(lhs, rhs)
        if lhs < rhs:
            g = d * v
            break
    if boost:
        u = float(st.uniforms(call)[0][i])
        call += 1
        g = g * math.exp((1.0 / shape) * math.log(u))
    return g, call, near, boost


def boost_bound_u(shape, st, i, call_of_boost):
    """the boosted gamma against the replay, in units of u: the factor exp(y log x), y = 1 / shape, carries dlog's C_LOG
    and math.log's 1 on an exponent of size |y log x| (and the product's rounding), dexp's C_EXP and math.exp's 1, and
    the final product's rounding on either side"""
    u = float(st.uniforms(call_of_boost)[0][i])
    return (hm.C_LOG + 3) * abs(math.log(u) / shape) + hm.C_EXP + 3


def negbin(mu, kappa, st, i, call):
    """-> (y, call, near tie)"""
    phi = 1.0 / kappa if kappa != 0.0 else math.inf
    if not (mu >= 0.0 and mu < math.inf and phi > 0.0 and phi < math.inf):
        return math.nan, call, False
    g, call, near, _ = gamma(phi, st, i, call)
    lam = (mu * g) / phi
    y, call, near2 = poisson(lam, st, i, call)
    return y, call, near or near2


def normal(mu, sd, st, i, call):
    z = float(st.normal(call)[i])
    if not (math.isfinite(mu) and math.isfinite(sd)):
        return sd * z + mu, call + 1, False
    return hm._fma(sd, z, mu), call + 1, False


def bernoulli(mu, st, i, call):
    u = float(st.uniforms(call)[0][i])
    return (math.nan if mu != mu else (1.0 if u < mu else 0.0)), call + 1, False


def replay(lib, kind, mu, shape, seed, chain, draw, row0):
    """the restated sampler over arguments i on rows row0 + i -> (samples, calls, near ties, boosted) as arrays"""
    mu = np.asarray(mu, dtype=np.float64)
    shape = np.broadcast_to(np.asarray(shape, dtype=np.float64), mu.shape)
    st = Streams(lib, seed, chain, draw, row0, mu.size)
    out, calls = np.empty(mu.size), np.empty(mu.size, dtype=np.intc)
    near, boosted = np.zeros(mu.size, dtype=bool), np.zeros(mu.size, dtype=bool)
    for i in range(mu.size):
        m, s = float(mu[i]), float(shape[i])
        if kind == NORMAL:
            out[i], calls[i], near[i] = normal(m, s, st, i, 0)
        elif kind == BERNOULLI:
            out[i], calls[i], near[i] = bernoulli(m, st, i, 0)
        elif kind == POISSON:
            out[i], calls[i], near[i] = poisson(m, st, i, 0)
        elif kind == GAMMA:
            out[i], calls[i], near[i], boosted[i] = gamma(s, st, i, 0)
        else:
            out[i], calls[i], near[i] = negbin(m, s, st, i, 0)
    return out, calls, near, boosted, st


# ---- the check's reduction (wn_replicate.h), replayed ------------------------------------------------------------
def wave_sum(lanes):
    """the xor butterfly over 64 values, offsets 32, 1, 2, 4, 8, 16: lane 0's result"""
    v = [float(x) for x in lanes]
    for off in (32, 1, 2, 4, 8, 16):
        v = [v[l] + v[l ^ off] for l in range(64)]
    return v[0]


def check_statistics(q, mu, v, live):
    """the six statistics of one draw: q, mu, v [N] and the live mask -> list of 6 floats (Python-float arithmetic in the
    kernel's order: lane k accumulates rows k, 64 + k, ... in ascending order, then the butterfly)"""
    N = len(q)
    acc = [[0.0, 0.0, math.inf, -math.inf, 0.0, 0.0] for _ in range(64)]
    with np.errstate(all="ignore"):
        for n in range(N):
            if not live[n]:
                continue
            a = acc[n % 64]
            x, m, w = np.float64(q[n]), np.float64(mu[n]), np.float64(v[n])
            a[0] = float(a[0] + x)
            a[1] = float(a[1] + x * x)
            a[2] = float(x) if x < a[2] else a[2]
            a[3] = float(x) if x > a[3] else a[3]
            a[4] = a[4] + (1.0 if x == 0.0 else 0.0)
            d = x - m
            a[5] = float(a[5] + (d * d) / w)
        out = [wave_sum([a[s] for a in acc]) for s in range(6)]
    out[2] = min(a[2] for a in acc)
    out[3] = max(a[3] for a in acc)
    return out


# ---- goodness of fit ---------------------------------------------------------------------------------------------
def chi_square(sample, pmf, cdf):
    """binned chi-square of integer samples against a pmf: bins pooled from the left to expected counts >= 5, the tails
    beyond the sample's range taken from the cdf -> (statistic, degrees of freedom)"""
    sample = np.asarray(sample).astype(np.int64)
    n, lo, hi = sample.size, int(sample.min()), int(sample.max())
    ks = np.arange(lo, hi + 1)
    e = n * pmf(ks)
    e[0] = n * cdf(lo)                # everything at or below the smallest value seen
    e[-1] = e[-1] + n * (1.0 - cdf(hi))   # ... and above the largest
    o = np.bincount(sample - lo, minlength=ks.size).astype(float)
    E, O, ce, co = [], [], 0.0, 0.0
    for ei, oi in zip(e, o):
        ce, co = ce + ei, co + oi
        if ce >= 5.0:
            E.append(ce)
            O.append(co)
            ce = co = 0.0
    if E:
        E[-1] += ce
        O[-1] += co
    E, O = np.array(E), np.array(O)
    return float(np.sum((O - E) ** 2 / E)), len(E) - 1
