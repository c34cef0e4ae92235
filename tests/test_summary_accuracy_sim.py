"""CPU tier: the device summaries (walnuts_amd/csrc/wn_summary.hip) under the workgroup emulation against the
exact-arithmetic reference (tests/helpers/hp_summary_reference.py) within its derived bounds, the stated rule for
non-finite draws, and the guard of the two-columns-per-lane kernels.  The shared body is tests/summary_accuracy.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpusim"))
import build as simbuild  # noqa: E402
import summary_accuracy as sa  # noqa: E402


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


def test_committed_seeds_have_no_near_tie():
    """The exact reference alone: with the committed seeds no column's ESS has a branch margin below the propagated
    bound on the tested quantity (the count is printed), and no case spends more than 2e5 exact products."""
    total = 0
    for name in sa.CASES:
        near = sa.near_ties(name)
        print(name, "near ties", len(near), "exact products", sum(c.products for c in sa.reference(name)))
        total += len(near)
    assert total == 0


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", sorted(sa.CASES))
def test_emulated_summaries_within_derived_bounds(sim, oracle, name):
    sa.check_case(name, lib_path=sim)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("lens", [[12, 9, 20], [40, 9, 20]], ids=["wide", "column_loops"])
def test_emulated_nonfinite_moments(sim, oracle, lens):
    sa.check_nonfinite_moments(lens, lib_path=sim)


@pytest.mark.timeout(600)
def test_emulated_nan_sign_does_not_move_quantiles(sim, oracle):
    sa.check_nan_sign_quantiles(lib_path=sim)


@pytest.mark.timeout(600)
def test_emulated_quantiles_among_many_nans(sim, oracle):
    sa.check_many_nans_quantiles(lib_path=sim)


def place_on_host(flat, off):
    """the emulation reads host memory: a copy of `flat` whose first element is `off` doubles past a 16-byte boundary"""
    buf = np.empty(flat.size + 3)
    start = (buf.ctypes.data // 8 + off) % 2          # doubles from the buffer's start to the wanted address
    view = buf[start:start + flat.size]
    view[:] = flat
    return view.ctypes.data, buf


@pytest.mark.timeout(600)
def test_emulated_wide_kernel_guard(sim, oracle):
    sa.check_wide_guard(place_on_host, lib_path=sim)
