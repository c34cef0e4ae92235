"""GPU tier: the samplers of walnuts_amd/csrc/wn_devrand.h on the device, through wn_internal_sampler_probe: the arguments
of tests/test_devrand_sim.py -- the replay cases and the one wavefront of mixed work -- must give the host build's bits,
samples and call counts, under the lane tables and under the memory tables.  What the host build's bits are worth is the
CPU tier's business (the exact replay, the goodness of fit)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import build as simbuild  # noqa: E402
import hp_math_reference as hm  # noqa: E402
import hp_replicate_reference as hr  # noqa: E402
from walnuts_amd import _ffi  # noqa: E402
from test_devrand_sim import MIXED, NAMES, REPLAY_CASES, SEED, check_mixed_wavefront  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return _ffi.load_library(simbuild.build())


@pytest.fixture(scope="module")
def device():
    return _ffi.load_library()


@pytest.mark.parametrize("case", REPLAY_CASES, ids=[NAMES[c[0]] for c in REPLAY_CASES])
def test_device_equals_host_build(gpu, host, device, case):
    kind, mu, shape, chain, draw, row0 = case
    want, want_calls = hr.sampler_probe(host, kind, mu, shape, SEED, chain, draw, row0, hr.GATHER)
    for tab in (hr.GATHER, hr.ARRAY):
        got, calls = hr.sampler_probe(device, kind, mu, shape, SEED, chain, draw, row0, tab)
        assert hm.same_bits(got, want) and np.array_equal(calls, want_calls), (NAMES[kind], tab)


def test_one_wavefront_of_mixed_work(gpu, host, device):
    """the divergence handling on the device: together equals alone, and both equal the host build"""
    assert check_mixed_wavefront(device)
    mu, kappa = MIXED
    for kind in (hr.POISSON, hr.NEGBIN, hr.GAMMA):
        shape = 1.0 / kappa if kind == hr.GAMMA else kappa
        got, calls = hr.sampler_probe(device, kind, mu, shape, SEED, 5, 6, 128, hr.GATHER)
        want, want_calls = hr.sampler_probe(host, kind, mu, shape, SEED, 5, 6, 128, hr.GATHER)
        assert hm.same_bits(got, want) and np.array_equal(calls, want_calls), kind
