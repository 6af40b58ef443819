"""GPU tier of the ESDF where the nearest site is far away: the cases of tests/esdf_far_case.py on the real device, the same
sizes as on the functional model.  What the device adds to that tier: its sqrtf and f32 rounding at d2 up to 65 000 in the
final rule, LDS and real concurrency.  The checker is tests/esdf_model.py; every comparison is exact and covers every voxel of
every block."""
import pytest

from tests import esdf_far_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(esdf_far_case.SPECS))
def test_esdf_far_equals_model(name):
    print(name, esdf_far_case.run_case(esdf_far_case.SPECS[name]))
