"""GPU tier: the device summaries against the exact-arithmetic reference (tests/helpers/hp_summary_reference.py)
within its derived bounds, the stated rule for non-finite draws, and the guard of the two-columns-per-lane kernels.
The shared body is tests/summary_accuracy.py; the worst error / bound per summary is recorded in DESIGN §3.6."""
import pytest

import summary_accuracy as sa

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu):
    yield gpu
    print("\nworst error / bound over all cases:", {k: float("%.3g" % v) for k, v in WORST.items()})


@pytest.mark.parametrize("name", sorted(sa.CASES))
def test_summaries_within_derived_bounds(name):
    for k, v in sa.check_case(name).items():
        WORST[k] = max(WORST.get(k, 0.0), v)


@pytest.mark.parametrize("lens", [[12, 9, 20], [40, 9, 20]], ids=["wide", "column_loops"])
def test_nonfinite_moments(lens):
    sa.check_nonfinite_moments(lens)


def test_nan_sign_does_not_move_quantiles():
    sa.check_nan_sign_quantiles()


def test_quantiles_among_many_nans():
    sa.check_many_nans_quantiles()


def place_on_device(flat, off):
    import torch

    buf = torch.empty(flat.size + 2, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[off:off + flat.size] = torch.from_numpy(flat)
    torch.cuda.synchronize()
    return buf.data_ptr() + 8 * off, buf


def test_wide_kernel_guard():
    sa.check_wide_guard(place_on_device)
