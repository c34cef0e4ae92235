"""CPU tier: the device maths of wn_devmath.h (dexp, dlog, dlog_normal, dexp_weight, dpow_pos, dsincospi, the Philox
streams, SharedDivisor) as the host build evaluates them -- wn_internal_math_probe / _stream_probe / _philox_probe of the
emulation library -- against mpmath and a NumPy Philox, within the bounds derived in tests/helpers/hp_math_reference.py,
at the arguments where such schemes go wrong: reduction and table boundaries, thresholds, subnormal arguments and
results, arguments next to 1, quadrant switches, NaN, +-inf, +-0.  tests/test_devmath_gpu.py compares the device with
this build bit for bit on the same lists."""
import ctypes as C
import os
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_math_reference as hm  # noqa: E402
from walnuts_amd import _ffi  # noqa: E402

U = hm.U
TABS = [hm.ARRAY, hm.UNIFORM, hm.GATHER]


@pytest.fixture(scope="module")
def lib():
    return _ffi.load_library(simbuild.build())


def worst_relative(got, exact, bound_u, what):
    """max |got - exact| / (u |exact|) over the entries; asserts each within bound_u (a scalar or one per entry)"""
    bound = np.broadcast_to(np.asarray(bound_u, dtype=np.float64), np.shape(got))
    worst, share = 0.0, 0.0
    for g, e, b, w in zip(got, exact, bound, what):
        r = hm.rel_err_u(g, e)
        assert r <= b, (w, float(g), float(e), r, b)
        worst, share = max(worst, r), max(share, r / b)
    return worst, share


def test_numpy_philox_known_answers():
    for rounds, ctr, key, want in hm.PHILOX_KATS:
        assert tuple(int(v) for v in hm.philox4x32(np.array([ctr]), np.array([key]), rounds)[0]) == want


def test_philox_probe_known_answers_and_random_counters(lib):
    for rounds, ctr, key, want in hm.PHILOX_KATS:
        assert tuple(int(v) for v in hm.philox_probe(lib, np.array([ctr]), np.array([key]), rounds)[0]) == want
    rng = np.random.default_rng(41)
    ctr, key = rng.integers(0, 2 ** 32, (4096, 4)), rng.integers(0, 2 ** 32, (4096, 2))
    for rounds in (7, 10):
        assert np.array_equal(hm.philox_probe(lib, ctr, key, rounds), hm.philox4x32(ctr, key, rounds))


def test_dexp_against_mpmath(lib):
    rng = np.random.default_rng(1)
    x = np.concatenate([hm.exp_edges(rng), hm.exp_fill(rng, 6000)])
    assert x.size <= 20000
    got = hm.math_probe(lib, hm.EXP, x)
    worst = 0.0
    with mp.workdps(hm.DPS):
        for xv, g in zip(x, got):
            if np.isnan(xv):
                assert np.isnan(g)
                continue
            e = hm.exp_exact(xv) if np.isfinite(xv) else (mp.inf if xv > 0 else mp.mpf(0))
            if e > mp.mpf(np.finfo(np.float64).max):   # the exact value rounds to +inf
                assert g == np.inf, xv
            elif e < mp.mpf(hm.DBL_MIN):  # subnormal results: C_EXP u of the smallest normal + half a subnormal spacing
                assert g >= 0.0 and abs(mp.mpf(float(g)) - e) <= hm.C_EXP * U * hm.DBL_MIN + hm.SUB / 2, (xv, g)
                assert xv >= hm.K_UNDER or g == 0.0
            else:
                r = hm.rel_err_u(g, e)
                assert r <= hm.C_EXP, (xv, g, r)
                worst = max(worst, r)
            if abs(xv) < 2.0 ** -54:
                assert g == 1.0, xv
    print("dexp worst", worst, "u")
    assert worst > 0.1 * hm.C_EXP
    assert hm.math_probe(lib, hm.EXP, [hm.K_OVER])[0] < np.inf
    assert hm.math_probe(lib, hm.EXP, [np.nextafter(hm.K_OVER, np.inf)])[0] == np.inf
    assert hm.math_probe(lib, hm.EXP, [np.nextafter(hm.K_UNDER, -np.inf)])[0] == 0.0


def test_dlog_against_mpmath_and_dlog_normal_bitwise(lib):
    rng = np.random.default_rng(2)
    x = np.concatenate([hm.log_edges(rng), hm.log_fill(rng, 6000)])
    assert x.size <= 20000
    got = hm.math_probe(lib, hm.LOG, x)
    worst = 0.0
    with mp.workdps(hm.DPS):
        for xv, g in zip(x, got):
            if np.isnan(xv) or xv < 0:
                assert np.isnan(g), xv
            elif xv == 0:
                assert g == -np.inf
            elif xv == np.inf:
                assert g == np.inf
            elif xv == 1.0:
                assert g == 0.0
            else:
                r = hm.rel_err_u(g, hm.log_exact(xv))   # relative to |log x|: this is what bites next to 1
                assert r <= hm.C_LOG, (xv, g, r)
                worst = max(worst, r)
    print("dlog worst", worst, "u")
    assert worst > 0.1 * hm.C_LOG
    # dlog_normal: dlog's main path, so the same bits on every positive normal argument
    xn = hm.positive_normal(x)
    assert xn.size > 8000
    assert hm.same_bits(hm.math_probe(lib, hm.LOG_NORMAL, xn), hm.math_probe(lib, hm.LOG, xn))


def test_dexp_weight_is_dexp_above_its_floor(lib):
    rng = np.random.default_rng(3)
    x = np.concatenate([hm.exp_weight_edges(rng), rng.uniform(-700, 256, 6000), rng.normal(0, 3, 2000)])
    got = hm.math_probe(lib, hm.EXP_WEIGHT, x)
    inside = x >= -700.0
    assert inside.sum() > 8000
    assert hm.same_bits(got[inside], hm.math_probe(lib, hm.EXP, x[inside]))
    floor = hm.math_probe(lib, hm.EXP, [-700.0])[0]
    assert 0 < floor < 1e-303
    assert np.all(got[~inside] == floor) and (~inside).sum() > 100   # below the floor, -inf and NaN
    assert np.all(hm.math_probe(lib, hm.EXP_WEIGHT, [-np.inf, np.nan, -701.0, np.nextafter(-700.0, -np.inf)]) == floor)


def test_dpow_pos_shortcuts_and_adam_range(lib):
    rng = np.random.default_rng(4)
    xs = np.concatenate([np.arange(1.0, 65.0), np.exp(rng.uniform(-700, 700, 200)), [49.0, 2.0, 1e-300, 5e-324]])
    assert np.all(hm.math_probe(lib, hm.POW, xs, np.zeros_like(xs)) == 1.0)
    assert hm.same_bits(hm.math_probe(lib, hm.POW, xs, np.ones_like(xs)), xs)
    assert hm.same_bits(hm.math_probe(lib, hm.POW, xs, np.full_like(xs, 0.5)), np.sqrt(xs))
    assert hm.math_probe(lib, hm.POW, [49.0], [0.5])[0] == 7.0
    x, y = hm.pow_args(rng, 4000)
    got = hm.math_probe(lib, hm.POW, x, y)
    with mp.workdps(hm.DPS):
        exact = [hm.pow_exact(a, b) for a, b in zip(x, y)]
        bound = [hm.pow_bound(a, b) for a, b in zip(x, y)]
    worst, share = worst_relative(got, exact, bound, zip(x, y))
    print("dpow_pos worst", worst, "u,", share, "of its bound")
    assert share > 0.1


def test_dsincospi_against_mpmath(lib):
    rng = np.random.default_rng(5)
    # the exact points: sin(pi q / 2), cos(pi q / 2), with the zeros' signs the quadrant logic gives (s = +0 at r = 0,
    # then the sign flips of quadrants 1..3: (c, -s), (-s, -c), (-c, s))
    sn, cs = hm.math_probe(lib, hm.SINCOSPI, [0.0, 0.5, 1.0, 1.5])
    assert np.array_equal(sn, [0.0, 1.0, 0.0, -1.0]) and np.array_equal(cs, [1.0, 0.0, -1.0, 0.0])
    assert list(np.signbit(sn)) == [False, False, True, True] and list(np.signbit(cs)) == [False, True, True, False]
    a = np.concatenate([hm.trig_edges(rng), rng.uniform(0, 2, 2000), rng.uniform(0, 1, 500) ** 8])
    ws, wc, wi = check_sincospi(lib, a)
    print("dsincospi worst sin", ws, "u, cos", wc, "u; identity", wi, "of its bound")
    assert ws > 0.1 * hm.C_TRIG and wc > 0.1 * hm.C_TRIG and wi > 0.1


def check_sincospi(lib, a):
    """both members within C_TRIG u RELATIVE (small results are not exempt), |sn^2 + cs^2 - 1| <= 2 C_TRIG u (evaluated
    exactly); -> the worst of each"""
    sn, cs = hm.math_probe(lib, hm.SINCOSPI, a)
    ws = wc = wi = 0.0
    lim = 2 * hm.C_TRIG * U
    with mp.workdps(hm.DPS):
        for k in range(a.size):
            es, ec = hm.sincospi_exact(a[k])
            rs = hm.rel_err_u(sn[k], es) if es != 0 else (0.0 if sn[k] == 0.0 else np.inf)
            rc = hm.rel_err_u(cs[k], ec) if ec != 0 else (0.0 if cs[k] == 0.0 else np.inf)
            assert rs <= hm.C_TRIG and rc <= hm.C_TRIG, (a[k], sn[k], cs[k], rs, rc)
            d = abs(mp.mpf(float(sn[k])) ** 2 + mp.mpf(float(cs[k])) ** 2 - 1)
            assert d <= lim, (a[k], float(d / U))
            ws, wc, wi = max(ws, rs), max(wc, rc), max(wi, float(d / lim))
    return ws, wc, wi


def test_dsincospi_bits_from_the_published_coefficients(lib):
    """the accuracy bound cannot see a wrong last digit of a coefficient (0.15 u at most); the scheme restated from
    fdlibm's printed constants in exactly rounded rational arithmetic can: bit for bit"""
    rng = np.random.default_rng(57)
    e = hm.trig_edges(rng)
    a = np.concatenate([e[(e > 2.0 ** -500) & (e < 2)], hm.trig_lattice(rng, 1500), rng.uniform(0, 2, 500)])
    sn, cs = hm.math_probe(lib, hm.SINCOSPI, a)
    want = np.array([hm.sincospi_scheme(float(v)) for v in a])
    assert np.array_equal(sn, want[:, 0]) and np.array_equal(cs, want[:, 1])


TABLE_SHIM = r'''
#include "wn_math_tables.h"
extern "C" {
const unsigned long long* t_exp2() { return wn_tab_exp2_bits; }
const unsigned long long* t_rcp() { return wn_tab_rcp_bits; }
const unsigned long long* t_logc() { return wn_tab_logc_bits; }
}
'''


def test_tables_are_the_correctly_rounded_values(tmp_path):
    """wn_math_tables.h states exp2[j] = 2^(j/64), rcp[i] = 64/(48+i), logc[i] = log((48+i)/64), correctly rounded: a
    last-bit error of one entry moves its cell's results by up to 2 u, which the 4 u bounds above need not notice"""
    (tmp_path / "shim.cpp").write_text(TABLE_SHIM)
    so = tmp_path / "libtables.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(os.path.dirname(HERE), "walnuts_amd", "csrc"),
                           str(tmp_path / "shim.cpp"), "-o", str(so)])
    L = C.CDLL(str(so))
    with mp.workdps(hm.DPS):
        for name, n, fn in (("t_exp2", 64, lambda j: mp.mpf(2) ** (mp.mpf(j) / 64)), ("t_rcp", 49, lambda i: mp.mpf(64) / (48 + i)),
                            ("t_logc", 49, lambda i: mp.log(mp.mpf(48 + i) / 64))):
            getattr(L, name).restype = C.POINTER(C.c_uint64)
            got = np.array(getattr(L, name)()[:n], dtype=np.uint64).view(np.float64)
            want = np.array([float(fn(i)) for i in range(n)])
            assert hm.same_bits(got, want), name


def test_dsincospi_on_the_generator_lattice(lib):
    """1e4 points (2 k + 1) 2^-52 = 2 * open01, the arguments the generator actually produces"""
    ws, wc, wi = check_sincospi(lib, hm.trig_lattice(np.random.default_rng(56), 10000))
    print("lattice worst sin", ws, "u, cos", wc, "u; identity", wi, "of its bound")
    assert ws > 0.1 * hm.C_TRIG and wc > 0.1 * hm.C_TRIG and wi > 0.1


@pytest.mark.parametrize("triple", hm.STREAM_TRIPLES, ids=["small", "mixed", "high_bits"])
def test_streams_from_integers(lib, oracle, triple):
    """stream_uniform is (k + 1/2) 2^-52 exactly for the NumPy Philox's k; the Box-Muller normals lie within C_NORMAL u
    of the exact pair formed from the same integers (the other two triples' at the top of the index range), and the
    2^12 pairs from index 0 carry the oracle's bits for every triple"""
    seed, chain, t = triple
    n = 1 << 12
    k1, k2 = hm.stream_integers(seed, chain, t, 1, 0, n)
    u = hm.stream_probe(lib, seed, chain, t, 1, 0, n, normals=False)
    assert np.array_equal(u, hm.uniform_of(k1)) and u.min() > 0 and u.max() < 1
    assert u[0] == oracle.stream_uniform(seed, chain, t, 1, 0)
    first = 2 ** 32 - n if chain else 0   # (the top of the index range once)
    k1, k2 = hm.stream_integers(seed, chain, t, 0, first, n)
    z0, z1 = hm.stream_probe(lib, seed, chain, t, 0, first, n, normals=True)
    o0, o1 = (z0, z1) if first == 0 else hm.stream_probe(lib, seed, chain, t, 0, 0, n, normals=True)
    zs = np.asarray(oracle.stream_normals(seed, chain, t, 0, 2 * n))
    assert hm.same_bits(zs[0::2], o0) and hm.same_bits(zs[1::2], o1)
    with mp.workdps(hm.DPS):
        exact = [hm.box_muller_exact(a, b) for a, b in zip(k1, k2)]
    w0, _ = worst_relative(z0, [e[0] for e in exact], hm.C_NORMAL, zip(k1, k2))
    w1, _ = worst_relative(z1, [e[1] for e in exact], hm.C_NORMAL, zip(k1, k2))
    print("normals worst", w0, w1, "u")
    assert max(w0, w1) > 0.1 * hm.C_NORMAL


def test_table_providers_agree(lib):
    """the three providers of the exp / log table entries give the same bits (on the host they are emulated lane reads;
    the device comparison is test_devmath_gpu.py's); every lane of a wave-uniform call returns the same bits"""
    rng = np.random.default_rng(6)
    for fn, x in ((hm.EXP, hm.exp_edges(rng)[::7]), (hm.LOG, hm.log_edges(rng)[::9]),
                  (hm.LOG_NORMAL, hm.positive_normal(hm.log_edges(rng))[::9]), (hm.EXP_WEIGHT, hm.exp_weight_edges(rng)[::7])):
        x = x[:1000]
        base = hm.math_probe(lib, fn, x)
        for n in (1, 63, 65, x.size):
            assert hm.same_bits(hm.math_probe(lib, fn, x[:n], tab=hm.GATHER), base[:n])
        un = hm.math_probe(lib, fn, x[:130], tab=hm.UNIFORM)
        assert hm.same_bits(un, np.repeat(base[:130, None], 64, axis=1))
    x, y = hm.pow_args(rng, 640)
    y = np.repeat(y[::64], 64)
    base = hm.math_probe(lib, hm.POW, x, y)
    assert hm.same_bits(hm.math_probe(lib, hm.POW, x[:600], y[:600], tab=hm.GATHER), base[:600])
    assert hm.same_bits(hm.math_probe(lib, hm.POW, x[::5], y[::5], tab=hm.UNIFORM)[:, 17], base[::5])
    seed, chain, t = hm.STREAM_TRIPLES[1]
    z = hm.stream_probe(lib, seed, chain, t, 0, 5, 200, normals=True)
    zg = hm.stream_probe(lib, seed, chain, t, 0, 5, 200, normals=True, tab=hm.GATHER)
    zu = hm.stream_probe(lib, seed, chain, t, 0, 5, 70, normals=True, tab=hm.UNIFORM)
    assert hm.same_bits(z[0], zg[0]) and hm.same_bits(z[1], zg[1])
    assert hm.same_bits(zu[0], np.repeat(z[0][:70, None], 64, axis=1)) and hm.same_bits(zu[1], np.repeat(z[1][:70, None], 64, axis=1))


def test_probe_rejects_bad_arguments(lib):
    x = np.ones(4)
    o = np.empty(4)
    dp = _ffi._dp
    assert lib.wn_internal_math_probe(x.ctypes.data_as(dp), None, o.ctypes.data_as(dp), None, 4, 99, 0) == -2
    assert lib.wn_internal_math_probe(x.ctypes.data_as(dp), None, o.ctypes.data_as(dp), None, 4, hm.EXP, 3) == -2
    assert lib.wn_internal_math_probe(x.ctypes.data_as(dp), None, o.ctypes.data_as(dp), None, 4, hm.POW, 0) == -2
    assert lib.wn_internal_math_probe(x.ctypes.data_as(dp), None, o.ctypes.data_as(dp), None, 4, hm.SINCOSPI, 0) == -2
    assert lib.wn_internal_stream_probe(1, 0, 0, 0, 2 ** 32 - 2, 4, 0, 0, o.ctypes.data_as(dp), None) == -2
    assert lib.wn_internal_math_probe(x.ctypes.data_as(dp), None, o.ctypes.data_as(dp), None, 0, hm.EXP, 0) == 0


def shared_divisor_cases(rng, n, divisors):
    """numerators 2^e [1, 2) in both signs, e over [-1022, 1023] with half of them below -950; divisors from the pool"""
    e = np.where(rng.random(n) < 0.5, rng.integers(-1022, -949, n), rng.integers(-949, 1024, n))
    a = np.ldexp(rng.uniform(1.0, 2.0, n), e) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return a, e, divisors[rng.integers(0, divisors.size, n)]


def test_shared_divisor_domain(lib):
    """2e7 quotients a / SharedDivisor(b) against IEEE division: equal bit for bit wherever |a| >= 2^SAFE_DIV_EXP and the
    quotient is a normal number; below that (the remainder a - b q0 is no longer representable) they may differ in the
    last bit, counted per numerator exponent and printed.  Exact zeros divide exactly; a non-finite numerator gives NaN."""
    rng = np.random.default_rng(23)
    pool = np.concatenate([hm.recurrence_weights(), np.exp(rng.uniform(-50, 50, 1200))])
    per_exponent = {}
    total = bad_inside = 0
    for _ in range(10):
        a, e, b = shared_divisor_cases(rng, 2_000_000, pool)
        got = hm.math_probe(lib, hm.SHARED_DIV, a, b)
        with np.errstate(over="ignore", under="ignore"):
            want = a / b
        normal = np.isfinite(want) & (np.abs(want) >= hm.DBL_MIN)
        miss = (got.view(np.uint64) != want.view(np.uint64)) & normal
        total += int(normal.sum())
        bad_inside += int(np.sum(miss & (e >= hm.SAFE_DIV_EXP)))
        for ex in e[miss]:
            per_exponent[int(ex)] = per_exponent.get(int(ex), 0) + 1
        # a mismatch is one unit in the last place, never more
        assert np.all(np.abs(got[miss].view(np.int64) - want[miss].view(np.int64)) == 1)
    print("SharedDivisor: quotients in the normal range", total, "mismatches by numerator exponent", sorted(per_exponent.items()))
    assert total > 1.5e7
    assert bad_inside == 0
    assert all(ex < hm.SAFE_DIV_EXP for ex in per_exponent)
    zeros = hm.math_probe(lib, hm.SHARED_DIV, np.tile([0.0, -0.0], pool.size), np.repeat(pool, 2))
    assert np.all(zeros == 0.0) and not np.any(np.signbit(zeros))   # (a zero of either sign gives +0)
    special = hm.math_probe(lib, hm.SHARED_DIV, [np.inf, -np.inf, np.nan], [3.0, 3.0, 3.0])
    assert np.all(np.isnan(special))   # (documented: NaN where `/` gives +-inf)
