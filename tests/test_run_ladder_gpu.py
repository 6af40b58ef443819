"""-m gpu: the voxel update at every run-length hand-over between its kernels, on the device.  The cases are those of
tests/run_ladder_case.py (hand-built clouds, the precondition proved on the CPU with the oracle's ray caster, the oracle's map bit for
bit, a failure names the length): the ladder 1 .. 2049 twice under each of the five routes (which kernel takes which lengths), in both
colour modes and with constant and 1/z^2 weights; the same two ladders with frames in flight (pipeline_frames = 2, each frame's tail
on its own: device only); `merged`'s sub-ladder and its mixed-label bundles; the bundle merge's own hand-over at 32 / 33 points; the
batched tail with combined lengths of 32, 33, 1024 and 1025 over batches of four and of eight frames; and the run that ends the sorted
pair list, inside a single tile — with its head on the last pair of a k_apply_runs tile as well."""
import pytest

from tests import run_ladder_case as R

pytestmark = pytest.mark.gpu

SPECS = R.gpu_specs()


@pytest.mark.parametrize("name", list(SPECS))
def test_run_lengths_at_the_hand_over_equal_oracle(name):
    out = R.run_case(SPECS[name])
    print(name, out)
