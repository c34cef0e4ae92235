"""GPU tier: the data models across elements per lane on the MI355X -- the checks of test_lane_widths_sim.py run on the
device: narrow grouped rows (1 < nx < EPL / 2) through the pointwise, predict and replicate hooks against the
high-precision references, and one problem per family forced onto (1, 2), (1, 4), (1, 8) and (1, 16), every real-valued
output within its geometry's counted bound of one shared reference, integer-valued outputs and the count families'
replicates identical."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_lane_widths_sim import (FAMILIES, FAMILY_IDS, NARROW, NARROW_IDS, NARROW_MODEL_IDS, NARROW_MODELS,  # noqa: E402
                                  check_all_widths, check_narrow_rows)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("model", NARROW_MODELS, ids=NARROW_MODEL_IDS)
@pytest.mark.parametrize("geometry,P", NARROW, ids=NARROW_IDS)
def test_narrow_grouped_rows_through_the_hooks(gpu, model, geometry, P, record_property):
    record_property("max_error_over_bound", check_narrow_rows(None, model, geometry, P))


@pytest.mark.parametrize("model", FAMILIES, ids=FAMILY_IDS)
def test_one_problem_at_every_width(gpu, model, record_property):
    """The replicates are compared for equality with no row set aside: test_lane_widths_sim.check_all_widths says why,
    and asserts on every run that the replay reports no near tie for the seed in use."""
    for epl, ratio in check_all_widths(None, model).items():
        record_property(f"max_error_over_bound_epl{epl}", ratio)
