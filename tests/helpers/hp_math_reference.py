"""High-precision references, error bounds and argument lists for the device maths of walnuts_amd/csrc/wn_devmath.h
(dexp, dlog, dlog_normal, dexp_weight, dpow_pos, dsincospi, the Philox streams and SharedDivisor), in the style of
hp_count_reference.py.  tests/test_devmath_sim.py holds the host build of the header to these references;
tests/test_devmath_gpu.py compares the device with the host build bit for bit on the same argument lists.

Nothing here is computed by the code under test: exp / log / sin / cos come from mpmath at DPS digits, the random
integers from a NumPy Philox4x32 written from the paper (Salmon et al., SC'11) and checked against the Random123
known answers in test_devmath_sim.py."""
import ctypes as C
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

DPS = 50
U = 2.0 ** -53
DBL_MIN = 2.0 ** -1022  # the smallest normal number
SUB = 2.0 ** -1074      # the spacing of the subnormal numbers

# ---- the bounds: units of u = 2^-53 relative to |exact value|; measured worst cases of the host build in brackets --
# dexp / dlog: the header states "within 2 ulp"; one ulp of a value is at most 2 u of it (just above a power of two),
# so 2 ulp <= 4 u.  (dexp 2.04 u, dlog 2.15 u over the edge lists and fill of this file)
C_EXP = 4
C_LOG = 4
# dsincospi: x = RN(kPi r) carries one rounding (1 u) and kPi's own representation error (pi - kPi = 1.22e-16: 0.4 u);
# a relative error of x enters sin x with the factor x cot x <= 1 and cos x with x tan x <= pi / 4 on |x| <= pi / 4:
# at most 1.4 u; the fdlibm kernels on that interval are good to under 1 ulp <= 2 u; and 2 u more for a result just
# below a power of two, where the kernel's ulp -- measured at the result -- is 2 u of the value.  1.4 + 2 + 2 = 5.4,
# stated as 8.  (sin 2.20 u, cos 2.19 u)
C_TRIG = 8
# stream_normal_pair: z = RN(RN(sqrt(RN(-2 L))) * t) with L = dlog(u1), t a dsincospi member.  -2 L is exact; the root
# halves L's relative error (C_LOG / 2) and rounds once (1 u: sqrt_normal is correctly rounded); t brings C_TRIG; the
# product rounds once more (1 u).  (4.5 u)
C_NORMAL = C_LOG / 2 + 1 + C_TRIG + 1
# dpow_pos(x, y) = dexp(RN(y dlog x)): dlog's relative error C_LOG u is an absolute error C_LOG u |log x| of the
# exponent, scaled by |y|, and an absolute error d of dexp's argument is a relative error d of its result; dexp adds
# C_EXP u: relative (C_EXP + C_LOG |y log x|) u.  The product's own rounding adds half an ulp of y log x, at most
# u |y log x|, so the full derivation gives (C_EXP + (C_LOG + 1) |y log x|) u; the narrower formula above, without that
# term, is the one asserted: it asks more of the code than the derivation promises, never less.
# (0.52 of the bound: 20.6 u where it is 39 u)


def pow_bound(x, y):
    """u-units relative bound of dpow_pos(x, y) away from its three shortcuts"""
    return C_EXP + C_LOG * abs(y * float(mp.log(mp.mpf(float(x)))))


# the domain SharedDivisor is stated on (wn_devmath.h): numerators of magnitude >= 2^SAFE_DIV_EXP, or exactly zero.
# The remainder a - b q0 is a multiple of ulp(b) ulp(q0) >= 2^-104 |a| / 2: exact -- representable -- as long as that is
# a multiple of 2^-1074, which |a| >= 2^-968 guarantees; 2^-960 leaves eight binades.
SAFE_DIV_EXP = -960


# ---- exact functions (mpf in, mpf out; callers convert at the end) ------------------------------------------------
def mpf(v):
    return mp.mpf(float(v))


def exp_exact(x):
    return mp.exp(mpf(x))


def log_exact(x):
    return mp.log(mpf(x))


def pow_exact(x, y):
    return mp.exp(mpf(y) * mp.log(mpf(x)))


def sincospi_exact(a):
    """(sin(pi a), cos(pi a)) with the argument reduced exactly first, so that results near zero keep all their digits"""
    A = mpf(a)
    q = mp.floor(2 * A + mp.mpf(0.5))
    r = A - q / 2  # exact: |r| <= 1/4
    s, c = mp.sin(mp.pi * r), mp.cos(mp.pi * r)
    m = int(q) & 3
    return [(s, c), (c, -s), (-s, -c), (-c, s)][m]


def box_muller_exact(k1, k2):
    """The pair stream_normal_pair forms from two 52-bit integers: u = (k + 1/2) 2^-52, sqrt(-2 log u1) (cos, sin)(2 pi u2)"""
    u1 = (mp.mpf(int(k1)) + mp.mpf(0.5)) * mp.mpf(2) ** -52
    u2 = (mp.mpf(int(k2)) + mp.mpf(0.5)) * mp.mpf(2) ** -52
    rad = mp.sqrt(-2 * mp.log(u1))
    # 2 u2 in (0, 2): reduce like sincospi_exact
    A = 2 * u2
    q = mp.floor(2 * A + mp.mpf(0.5))
    r = A - q / 2
    s, c = mp.sin(mp.pi * r), mp.cos(mp.pi * r)
    sn, cs = [(s, c), (c, -s), (-s, -c), (-c, s)][int(q) & 3]
    return rad * cs, rad * sn


# ---- dsincospi's scheme restated from the published constants, exactly rounded operation by operation -------------
# Sun fdlibm 5.3, k_sin.c S1..S6 and k_cos.c C1..C6, as printed there (each decimal string names one binary64)
FDLIBM_S = [-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04,
            2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10]
FDLIBM_C = [4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05,
            -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11]


def _fma(a, b, c):
    """RN(a b + c) for finite doubles: exact rational arithmetic, one rounding (float(Fraction) rounds correctly)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def sincospi_scheme(a):
    """(sin(pi a), cos(pi a)) by the header's scheme -- quadrant reduction, RN(pi) * r, the two fdlibm kernels as Horner
    chains of fused multiply-adds -- with fdlibm's coefficients: the bits a correct transcription must give (a in (0, 2))"""
    qf = float(math.floor(_fma(a, 2.0, 0.5)))
    r = _fma(-qf, 0.5, a)
    x = math.pi * r   # (math.pi is RN(pi), the header's kPi)
    z = x * x
    ps = FDLIBM_S[5]
    for cf in FDLIBM_S[4::-1]:
        ps = _fma(z, ps, cf)
    s = _fma(x, z * ps, x)
    pc = FDLIBM_C[5]
    for cf in FDLIBM_C[4::-1]:
        pc = _fma(z, pc, cf)
    c = _fma(z * z, pc, _fma(-0.5, z, 1.0))
    return [(s, c), (c, -s), (-s, -c), (-c, s)][int(qf) & 3]


def rel_err_u(got, exact):
    """|got - exact| / (u |exact|) for a float and a non-zero mpf"""
    return float(abs(mp.mpf(float(got)) - exact) / abs(exact) / mp.mpf(U))


# ---- Philox4x32 in NumPy (Salmon et al., SC'11, fig. 2: the multipliers and Weyl key increments of Random123) -----
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32(ctr, key, rounds):
    """ctr [n, 4], key [n, 2] (any integer type, values below 2^32) -> [n, 4] uint32"""
    c = [np.asarray(ctr)[:, i].astype(np.uint64) for i in range(4)]
    k0 = np.asarray(key)[:, 0].astype(np.uint64)
    k1 = np.asarray(key)[:, 1].astype(np.uint64)
    for _ in range(rounds):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=1).astype(np.uint32)


# Random123's kat_vectors for philox4x32: (rounds, counter, key, output)
PHILOX_KATS = [
    (10, (0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    (10, (0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    (10, (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    (7, (0, 0, 0, 0), (0, 0), (0x5f6fb709, 0x0d893f64, 0x4f121f81, 0x4f730a48)),
    (7, (0xffffffff,) * 4, (0xffffffff,) * 2, (0x5207ddc2, 0x45165e59, 0x4d8ee751, 0x8c52f662)),
    (7, (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0x4dfccaba, 0x190a87f0, 0xc47362ba, 0xb6b5242a)),
]
STREAM_ROUNDS = 7
# (seed, chain, transition) of the stream comparisons (the triples of test_portable_math.py)
STREAM_TRIPLES = [(1, 0, 0), (2 ** 40 + 17, 65535, 1234), (2 ** 63 + 5, 2 ** 31, 2 ** 31 + 1)]


def stream_integers(seed, chain, transition, stream, first, n):
    """(k1, k2) [n] uint64: the top 52 bits of the two 64-bit words the engine's counter layout yields for indices
    first .. first + n - 1: counter = (index, transition, chain, stream), key = (seed low word, seed high word)"""
    idx = (np.arange(n, dtype=np.uint64) + np.uint64(first))
    ctr = np.stack([idx, np.full(n, transition, np.uint64), np.full(n, chain, np.uint64), np.full(n, stream, np.uint64)], 1)
    key = np.stack([np.full(n, seed & 0xFFFFFFFF, np.uint64), np.full(n, seed >> 32, np.uint64)], 1)
    o = philox4x32(ctr, key, STREAM_ROUNDS).astype(np.uint64)
    k1 = ((o[:, 1] << np.uint64(32)) | o[:, 0]) >> np.uint64(12)
    k2 = ((o[:, 3] << np.uint64(32)) | o[:, 2]) >> np.uint64(12)
    return k1, k2


def uniform_of(k):
    """(k + 1/2) 2^-52 = (2 k + 1) 2^-53: exact in binary64 for k < 2^52"""
    return (2.0 * k.astype(np.float64) + 1.0) * 2.0 ** -53


# ---- the probes (wn_internal_math_probe / _stream_probe / _philox_probe of either library) ------------------------
EXP, LOG, LOG_NORMAL, EXP_WEIGHT, POW, SINCOSPI, SHARED_DIV = range(7)
ARRAY, UNIFORM, GATHER = range(3)
_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint32)


def math_probe(lib, fn, x, y=None, tab=ARRAY):
    """out0 (and out1 for SINCOSPI); under UNIFORM the arrays are [n, 64]: every lane's result"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    yy = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    shape = (x.size, 64) if tab == UNIFORM else (x.size,)
    o0 = np.empty(shape)
    o1 = np.empty(shape) if fn == SINCOSPI else None
    rc = lib.wn_internal_math_probe(x.ctypes.data_as(_dp), None if yy is None else yy.ctypes.data_as(_dp),
                                    o0.ctypes.data_as(_dp), None if o1 is None else o1.ctypes.data_as(_dp), x.size, fn, tab)
    assert rc == 0, rc
    return (o0, o1) if fn == SINCOSPI else o0


def stream_probe(lib, seed, chain, transition, stream, first, n, normals, tab=ARRAY):
    shape = (n, 64) if tab == UNIFORM else (n,)
    o0 = np.empty(shape)
    o1 = np.empty(shape) if normals else None
    rc = lib.wn_internal_stream_probe(seed, chain, transition, stream, first, n, int(normals), tab, o0.ctypes.data_as(_dp),
                                      None if o1 is None else o1.ctypes.data_as(_dp))
    assert rc == 0, rc
    return (o0, o1) if normals else o0


def philox_probe(lib, ctr, key, rounds):
    c = np.ascontiguousarray(ctr, dtype=np.uint32)
    k = np.ascontiguousarray(key, dtype=np.uint32)
    out = np.empty_like(c)
    assert lib.wn_internal_philox_probe(c.ctypes.data_as(_up), k.ctypes.data_as(_up), out.ctypes.data_as(_up), c.shape[0],
                                        rounds) == 0
    return out


def same_bits(a, b):
    """bit for bit, NaNs by class (the payload and sign of a NaN that an out-of-domain argument produces are not part
    of any function's contract)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


# ---- argument lists: deterministic edges, then a seeded random fill ----------------------------------------------
K_OVER, K_UNDER = 7.09782712893383973096e+02, -7.45133219101941108420e+02  # dexp's thresholds (wn_devmath.h)
SPECIALS = [0.0, -0.0, np.inf, -np.inf, np.nan]


def neighbours(v, k=2):
    """v and the k doubles each side of it"""
    out, lo, hi = [v], v, v
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def exp_edges(rng):
    """dexp: every reduction boundary (j + 1/2) ln2 / 64 of the 64 table cells at result exponents over the whole range
    -- the boundary's double, two neighbours each side, a random point of the cell --, the thresholds, |x| < 2^-54, specials"""
    with mp.workdps(DPS):
        step = mp.log(2) / 64
        out = []
        for e in (-1076, -1074, -1060, -1040, -1023, -1022, -1021, -1000, -700, -300, -60, -2, -1, 0, 1, 2, 60, 300, 700,
                  1000, 1022, 1023):
            for j in range(64):
                k = 64 * e + j
                out += neighbours(float((k + mp.mpf(0.5)) * step))
                out.append(float((k + mp.mpf(float(rng.uniform(-0.5, 0.5)))) * step))
    out += neighbours(K_OVER) + neighbours(K_UNDER) + neighbours(-708.3964185322641)  # (log of the smallest normal)
    out += [s * 2.0 ** -m for m in (55, 56, 60, 100, 500, 1000, 1022, 1023, 1074) for s in (1.0, -1.0)]
    out += [1000.0, -1000.0, 1e308, -1e308] + SPECIALS
    return np.array(out)


def exp_fill(rng, n):
    parts = [rng.uniform(-745.14, -708.39, n // 4), rng.uniform(-708.4, 709.8, n // 2), rng.normal(0, 3, n // 8)]
    parts.append(rng.uniform(-1, 1, n - sum(p.size for p in parts)) * 2.0 ** rng.integers(-60, 1, n - sum(p.size for p in parts)))
    return np.concatenate(parts)


def log_edges(rng):
    """dlog: every table boundary (i +- 1/2) / 64, i = 48..96, +- two doubles at several exponents; 1 +- k ulps and
    1 +- 2^-m; the halving boundary 1.5; every power of two; subnormals; specials"""
    out = []
    for e in (-1074, -1050, -1022, -500, -1, 0, 1, 500, 1023):
        for i in range(48, 97):
            for h in (-0.5, 0.5):
                out += [np.ldexp(v, e) for v in neighbours((i + h) / 64.0)]
        out += [np.ldexp(v, e) for v in neighbours(1.5, 4)]
    out += [1.0 + k * 2.0 ** -52 for k in range(65)] + [1.0 - k * 2.0 ** -53 for k in range(65)]
    out += [1.0 + 2.0 ** -m for m in range(1, 53)] + [1.0 - 2.0 ** -m for m in range(1, 54)]
    out += [np.ldexp(1.0, e) for e in range(-1074, 1024)]
    out += [5e-324, 1e-323, DBL_MIN - SUB, DBL_MIN, DBL_MIN + SUB, np.finfo(np.float64).max]
    out += list(rng.integers(1, 2 ** 52, 300).astype(np.float64) * SUB)  # subnormals of every size
    out += SPECIALS + [-1.0, -5e-324, -DBL_MIN, -1e300]
    return np.array(out)


def log_fill(rng, n):
    return np.concatenate([np.exp(rng.uniform(-744, 709, n // 2)), rng.uniform(0.5, 2.0, n // 4),
                           1.0 + rng.uniform(-1, 1, n - n // 2 - n // 4) * 2.0 ** rng.integers(-50, -3, n - n // 2 - n // 4)])


def positive_normal(x):
    x = np.asarray(x)
    return x[np.isfinite(x) & (x >= DBL_MIN)]


def exp_weight_edges(rng):
    """dexp_weight: the floor and below (all stand at the floor), [-700, 256], the same cell boundaries as dexp"""
    e = exp_edges(rng)
    e = e[~(e > 700.0)]  # (-inf and NaN stay; arguments past the rebase threshold are outside the function's contract)
    return np.concatenate([e, neighbours(-700.0), [256.0, -699.999, 16.0, -16.0, -701.0, -1e6]])


def pow_args(rng, n):
    """Adam's range: x = t in 1 .. 1e6, y in [-1, 0); then the three shortcuts"""
    x = np.concatenate([np.arange(1.0, 201.0), np.floor(np.exp(rng.uniform(0, np.log(1e6), n - 200)))])
    y = np.concatenate([[-1.0, -0.5, -0.7, -0.25, -1e-3, -2.0 ** -30], -rng.uniform(0, 1, n - 6)])
    y[y == 0.0] = -0.5
    return x, y


def trig_edges(rng):
    """dsincospi on [0, 2): the exact points q / 2, the quadrant switches +- four doubles, 2^-m, the top of the range, the
    lattice (2 k + 1) 2^-52 that 2 * open01 produces"""
    out = [0.0, 0.5, 1.0, 1.5]
    for a in (0.25, 0.75, 1.25, 1.75, 0.5, 1.0, 1.5):
        out += neighbours(a, 4)
    out += [2.0 ** -m for m in range(1, 61)] + [2.0 - 2.0 ** -52, 2.0 - 2.0 ** -51, DBL_MIN]
    return np.array(out)


def trig_lattice(rng, n):
    return (2.0 * rng.integers(0, 2 ** 52, n).astype(np.float64) + 1.0) * 2.0 ** -52


def recurrence_weights():
    """the weights the mass estimator's recurrence w <- (1 - 1 / (count + i)) w + 1 takes (adaptive_walnuts.hpp:74-80), as
    test_portable_math.py builds them"""
    ws = []
    for count in (4.0, 1.0, 10.0, 0.5):
        w = count
        for i in range(400):
            ws.append(w)
            w = (1.0 - 1.0 / (count + i)) * w + 1.0
    return np.array(ws)
