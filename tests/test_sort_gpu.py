"""GPU tier of the radix sort's own tests (csrc/ks_radix_sort.h): every spec of tests/sort_case.py on the real device — the specs of
the functional model at the same sizes, and those only the device can run: the 8192-key tile and the LDS-reordering variant at
2^20 + 1 keys, the 16384-key tile at 2^24 + 1, the sequence with frame-sized sorts, the batch at 2^20 + 1 keys per sort.  The
yardstick is NumPy's stable argsort of the sorted bits alone; every comparison is exact."""
import pytest

from tests import sort_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(sort_case.SPECS))
def test_sort_equals_yardstick(name):
    sort_case.run_case(sort_case.SPECS[name])
