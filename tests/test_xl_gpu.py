"""-m gpu: the integer-sum voxel update (csrc/ks_k_apply_xl.h) at ties, binade edges and clamps, on the device.  The cases are those of
the CPU tier, unchanged (tests/xl_case.py: hand-built clouds, the model's precondition, the oracle's map bit for bit, the path through
update_stats()), plus three that a serial functional model cannot judge: the run-edge clouds as six frames IN FLIGHT (the single set of
XL buffers is used by all of them) with pipeline_frames = 2, with pipeline_frames = 8 (the batched stage B), and with the long-run chain
on a stream of its own (KS_DEBUG=1 KS_HW_QUEUES=8) beside the plan for the environment's budget.

The merged_lanes_* cases are the only DIRECT check of the DPP wavefront sum (wave_sum_i32_dpp): bundles of 1..5 points, mixed labels and
points of label 0 put a different integer into every lane and row of every sum, where the uniform runs put the same one (a reduction
that counted one row twice and dropped another would go unnoticed there); the functional model of the CPU tier replaces that function
by its own."""
import os

import pytest

from tests import xl_case
from tests.util import compare_maps

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(xl_case.SPECS))
def test_xl_edge_case_equals_oracle_and_model(name):
    out = xl_case.run_case(xl_case.SPECS[name])
    print(name, out)


def _in_flight(pipeline, env=None):
    o, g, want, st = xl_case.run_sequence(pipeline, env)
    compare_maps(o, g, exact=True)
    assert g.block_indices().tobytes() == o.block_indices().tobytes()
    assert st == want, (st, want)                 # uniform runs: the totals are the model's, whatever was in flight
    assert st["walked"] == 4 and st["serial"] == 1 and st["chunks"] == 5 + 5 + 6 + 5, st   # (1024 is not listed, the fresh voxel refused)
    return g


def test_frames_in_flight_share_the_xl_buffers():
    g = _in_flight(2)
    assert g.pipeline_shape()["lag"] == 2, g.pipeline_shape()


def test_batched_stage_b_shares_the_xl_buffers():
    g = _in_flight(8)
    assert g.pipeline_shape()["batch"] >= 2 and g.pipeline_shape()["lag"] == 8, g.pipeline_shape()


def test_long_run_chain_on_a_stream_of_its_own_on_the_tail_stream_and_on_the_plan_of_the_environment():
    """KS_DEBUG=1 KS_HW_QUEUES=8: every chain on a stream of its own; =3: the long-run chain folded onto the stage-T stream, behind
    k_apply (contexts without an early-out hold four streams: nothing folds at the runtime's default of four queues); without the
    switch the plan for the budget the environment gives (GPU_MAX_HW_QUEUES is only read).  The same map and the same path."""
    own = _in_flight(8, {"KS_HW_QUEUES": "8"})
    assert own.stream_plan()["budget"] == 8 and own.stream_plan()["xlong"] == "own", own.stream_plan()
    folded = _in_flight(8, {"KS_HW_QUEUES": "3"})
    assert folded.stream_plan()["xlong"] == "tail", folded.stream_plan()
    env = _in_flight(8)
    try:
        budget = min(32, max(1, int(os.environ.get("GPU_MAX_HW_QUEUES", ""))))
    except ValueError:
        budget = 4
    print("plans", own.stream_plan(), folded.stream_plan(), env.stream_plan())
    assert env.stream_plan()["budget"] == budget, env.stream_plan()
    assert env.stream_plan()["xlong"] == ("own" if budget >= 4 else "tail"), env.stream_plan()
    compare_maps(own, env, exact=True)
    compare_maps(own, folded, exact=True)
