"""GPU tier: the device maths of wn_devmath.h on the MI355X against the host build of the same header (the emulation
library's probes, which tests/test_devmath_sim.py holds to mpmath): bit for bit through view(np.uint64), NaNs by class.

Every function under every provider of the exp / log table entries it takes -- ArrayTables, UniformTab (v_readlane of a
wave-uniform index), GatherTab (a lane gather, with a clamped partial last wavefront) --, on the edge lists of
tests/helpers/hp_math_reference.py plus a seeded random fill; Philox on the device (the v_bitop3 form of xor3) against
the Random123 known answers and a NumPy Philox; the uniform and normal streams; SharedDivisor."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_math_reference as hm  # noqa: E402
from walnuts_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu
N_FILL = 1 << 18
N_UNIFORM = 1 << 12


@pytest.fixture(scope="module")
def host():
    return _ffi.load_library(simbuild.build())


@pytest.fixture(scope="module")
def dev(gpu):
    return gpu.load_library()


SHORTCUTS = (0.0, 1.0, 0.5)   # the exponents dpow_pos answers without its tables (1, x, sqrt x)


def arguments(fn, rng, n):
    """(x, the exponent lists, number of edge arguments): the edge list of the function first, then the seeded fill to n.
    dpow_pos has two exponent lists: one where every run of 64 arguments shares its first exponent (what the lane tables
    need: the function returns on y ahead of its table reads) with the runs 1, 2 and 3 standing at the three shortcuts
    (run 0 keeps y = -1, so the launches of 1 and 63 arguments read the tables), and one with an exponent per argument,
    the shortcuts among them, for the providers that do not gather."""
    if fn == hm.POW:
        x, each = hm.pow_args(rng, n)
        each[200:264] = np.repeat(SHORTCUTS + (-0.5,), 16)
        runs = np.repeat(each[::64], 64)[:n]
        for k, v in enumerate(SHORTCUTS):
            runs[64 * (k + 1):64 * (k + 2)] = v
        return x, [runs, each], 264
    if fn == hm.EXP:
        e, f = hm.exp_edges(rng), hm.exp_fill(rng, n)
    elif fn == hm.LOG:
        e, f = hm.log_edges(rng), hm.log_fill(rng, n)
    elif fn == hm.LOG_NORMAL:   # its contract: positive normal arguments
        e, f = hm.positive_normal(hm.log_edges(rng)), hm.positive_normal(hm.log_fill(rng, n + n // 8))
    else:
        e, f = hm.exp_weight_edges(rng), np.concatenate([rng.uniform(-700, 256, n // 2), rng.normal(0, 3, n // 2)])
    return np.concatenate([e, f[:n - e.size]]), [None], e.size


def launched(y, idx):
    """the exponents of one launch; a dpow_pos launch that takes in the planted ones holds each of the three shortcuts"""
    if y is None:
        return None
    y = y[idx]
    assert y.size < 264 or all(np.any(y == v) for v in SHORTCUTS)
    return y


@pytest.mark.parametrize("fn", [hm.EXP, hm.LOG, hm.LOG_NORMAL, hm.EXP_WEIGHT, hm.POW],
                         ids=["dexp", "dlog", "dlog_normal", "dexp_weight", "dpow_pos"])
def test_table_functions_device_equals_host_under_every_provider(dev, host, fn):
    x, ys, edges = arguments(fn, np.random.default_rng(100 + fn), N_FILL)
    assert x.size == N_FILL
    everything = slice(None)
    # one argument per wavefront iteration: the edge list and 2^12 of the fill
    pick = np.concatenate([np.arange(edges), N_FILL - 1 - np.arange(N_UNIFORM)])
    for y in ys:
        want = hm.math_probe(host, fn, x, launched(y, everything))
        for tab in (hm.ARRAY, hm.GATHER) if y is ys[0] else (hm.ARRAY,):   # (ys[0]: a run of 64 shares its exponent)
            assert hm.same_bits(hm.math_probe(dev, fn, x, launched(y, everything), tab=tab), want), (fn, tab)
            for n in (1, 63, 65):   # (one lane, a partial wavefront, one wavefront and one lane)
                assert hm.same_bits(hm.math_probe(dev, fn, x[:n], launched(y, slice(n)), tab=tab), want[:n]), (fn, tab, n)
        got = hm.math_probe(dev, fn, x[pick], launched(y, pick), tab=hm.UNIFORM)
        assert hm.same_bits(got, np.repeat(want[pick][:, None], 64, axis=1)), fn   # all 64 lanes return the same bits


def test_sincospi_device_equals_host(dev, host):
    rng = np.random.default_rng(110)
    e = hm.trig_edges(rng)
    a = np.concatenate([e, hm.trig_lattice(rng, N_FILL // 2), [np.nan, np.inf, -np.inf, -0.0, 5e-324],
                        rng.uniform(0, 2, N_FILL - N_FILL // 2 - e.size - 5)])
    want = hm.math_probe(host, hm.SINCOSPI, a)
    for n in (1, 63, 65, a.size):
        for tab in (hm.ARRAY, hm.GATHER):
            got = hm.math_probe(dev, hm.SINCOSPI, a[:n], tab=tab)
            assert hm.same_bits(got[0], want[0][:n]) and hm.same_bits(got[1], want[1][:n]), (n, tab)


def test_philox_device_known_answers_and_numpy(dev):
    """the first time the device's xor3 (v_bitop3_b32, truth table 0x96) meets a known answer"""
    for rounds, ctr, key, want in hm.PHILOX_KATS:
        assert tuple(int(v) for v in hm.philox_probe(dev, np.array([ctr]), np.array([key]), rounds)[0]) == want
    rng = np.random.default_rng(111)
    ctr, key = rng.integers(0, 2 ** 32, (1 << 16, 4)), rng.integers(0, 2 ** 32, (1 << 16, 2))
    for rounds in (7, 10):
        assert np.array_equal(hm.philox_probe(dev, ctr, key, rounds), hm.philox4x32(ctr, key, rounds))


@pytest.mark.parametrize("triple", hm.STREAM_TRIPLES, ids=["small", "mixed", "high_bits"])
def test_streams_device_equal_host(dev, host, triple):
    seed, chain, t = triple
    n = 1 << 16
    want_u = hm.stream_probe(host, seed, chain, t, 1, 0, n, normals=False)
    assert np.array_equal(want_u, hm.uniform_of(hm.stream_integers(seed, chain, t, 1, 0, n)[0]))
    assert hm.same_bits(hm.stream_probe(dev, seed, chain, t, 1, 0, n, normals=False), want_u)
    w0, w1 = hm.stream_probe(host, seed, chain, t, 0, 0, n, normals=True)
    for tab, m in ((hm.ARRAY, n), (hm.GATHER, n), (hm.GATHER, 65), (hm.GATHER, 63), (hm.GATHER, 1)):
        z0, z1 = hm.stream_probe(dev, seed, chain, t, 0, 0, m, normals=True, tab=tab)
        assert hm.same_bits(z0, w0[:m]) and hm.same_bits(z1, w1[:m]), (tab, m)
    z0, z1 = hm.stream_probe(dev, seed, chain, t, 0, 0, N_UNIFORM, normals=True, tab=hm.UNIFORM)
    assert hm.same_bits(z0, np.repeat(w0[:N_UNIFORM, None], 64, axis=1))
    assert hm.same_bits(z1, np.repeat(w1[:N_UNIFORM, None], 64, axis=1))


def test_shared_divisor_device_equals_host(dev, host):
    """the estimator's weights times 2^12 numerators each: every exponent, subnormals, zeros, +-inf and NaN"""
    rng = np.random.default_rng(112)
    w = hm.recurrence_weights()
    m = 1 << 12
    a = np.ldexp(rng.uniform(1.0, 2.0, (w.size, m)), rng.integers(-1074, 1024, (w.size, m))) * rng.choice([-1.0, 1.0], (w.size, m))
    a[:, :8] = [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, hm.DBL_MIN - hm.SUB]
    a[:, 8:264] = rng.normal(size=(w.size, 256))
    b = np.repeat(w[:, None], m, axis=1)
    want = hm.math_probe(host, hm.SHARED_DIV, a.ravel(), b.ravel())
    assert hm.same_bits(hm.math_probe(dev, hm.SHARED_DIV, a.ravel(), b.ravel()), want)
    assert hm.same_bits(hm.math_probe(dev, hm.SHARED_DIV, a.ravel()[:65], b.ravel()[:65], tab=hm.GATHER), want[:65])
