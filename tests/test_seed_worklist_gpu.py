"""GPU tier: the early-out seed's work list (k_seed_list -> k_test) against the oracle — the cases of tests/seed_case.py (frames of
1 .. 5000 points, all rays live, none live, in a context of 7000 points; the ordered-phase mode against its CPU restatement, the
default mode against the reference's serial loop; unpipelined, in batches of four and of eight frames), one full 640x480
sequence with pipeline_frames = 12, and the guard for a list that does not fit its launch."""
import os

import pytest

from tests import seed_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pipeline", [0, 2, 8, 16])
@pytest.mark.parametrize("mode", ["phased", "serial"])
def test_seed_work_list_equals_oracle(mode, pipeline):
    print(seed_case.run(dict(mode=mode, pipeline=pipeline)))


@pytest.mark.parametrize("order", [1, 2])
def test_seed_work_list_in_the_other_orders_equals_oracle(order):
    print(seed_case.run(dict(mode="phased", pipeline=0, order=order)))


@pytest.mark.parametrize("mode", ["phased", "serial"])
def test_full_frames_twelve_in_flight_equal_oracle(mode):
    """640x480 at the context's own capacity (307 200; the frames have a few points fewer: capacity != n), pipeline_frames = 12:
    batches of four frames per launch, the lists of a slot rebuilt while the batches before it are in flight."""
    rep = seed_case.run(dict(mode=mode, pipeline=12, capacity=640 * 480, max_tiles=1 << 15, sizes=[], all_live=False, none_live=False,
                             full_frames=[[640, 480, 9]]))
    print(rep)
    assert rep["rays"] > 9 * 30000


@pytest.mark.parametrize("mode", ["phased", "serial"])
def test_a_list_that_does_not_fit_its_launch_is_an_error_not_a_wrong_map(mode, monkeypatch):
    monkeypatch.setenv("KS_DEBUG", "1")
    monkeypatch.setenv("KS_SEED_CAP_ITEMS", "4")
    print(seed_case.run_overflow(dict(mode=mode)))
