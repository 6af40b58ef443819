"""GPU tier: the stream plan (ks_stream_plan) on the device.  640x480 frames through the pipelined default mode with the process's
hardware queues as the environment gives them (four unless GPU_MAX_HW_QUEUES says otherwise: the side chains of stage T run on
the stage-T stream) and with KS_DEBUG=1 KS_HW_QUEUES=8 (every chain on a stream of its own, the layout as it always was): the map
and the summed frame statistics equal the unpipelined context's, bit for bit.  `merged` and `fast` at 2 cm voxels, whose contexts
never had more than four streams: the same plan at both budgets, the same maps.  The tests only READ GPU_MAX_HW_QUEUES."""
import os

import pytest

from kimera_semantics_amd import binding as B
from kimera_semantics_amd import synth
from tests.util import COMMON, compare_maps

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("n_points", "n_valid_points", "n_rays_cast", "n_voxel_updates", "n_blocks_allocated")


def env_budget():
    """What the library makes of the environment as it is: 4 when the variable is unset or no number, 1 .. 32."""
    try:
        return min(32, max(1, int(os.environ.get("GPU_MAX_HW_QUEUES", ""))))
    except ValueError:
        return 4


def frames(count, w=640, h=480, scene="room", **kw):
    sc = synth.make_scene(scene)
    return [synth.render_frame(sc, synth.trajectory_pose(2 * k, **kw), w, h, seed=900 + k) for k in range(count)]


def through(fr, monkeypatch, budget, **cfg):
    """(context, summed statistics) after the frames; budget None = the environment as it is."""
    monkeypatch.delenv("KS_HW_QUEUES", raising=False)
    if budget is not None:
        monkeypatch.setenv("KS_DEBUG", "1")
        monkeypatch.setenv("KS_HW_QUEUES", str(budget))
    g = B.HipIntegrator(B.default_config(**dict(COMMON, **cfg)))
    if budget is not None:
        monkeypatch.delenv("KS_HW_QUEUES")
        monkeypatch.delenv("KS_DEBUG")
    tot = dict.fromkeys(STAT_FIELDS, 0)
    for f in fr:
        st = g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        for k in STAT_FIELDS:
            tot[k] += getattr(st, k)
    st = g.flush()
    for k in STAT_FIELDS:
        tot[k] += getattr(st, k)
    return g, tot


def same_map(ref, tot_ref, g, tot):
    assert tot == tot_ref, (tot, tot_ref)
    rep = compare_maps(ref, g, exact=True)
    assert ref.block_indices().tobytes() == g.block_indices().tobytes()
    return rep


@pytest.fixture(scope="module")
def c2_frames():
    return frames(16)


@pytest.mark.parametrize("pipeline", [12, 16])
def test_pipelined_default_mode_at_the_budget_of_the_environment_and_at_8_equals_unpipelined(c2_frames, monkeypatch, pipeline):
    cfg = dict(method=0, max_tiles=1 << 13, max_points=640 * 480)
    ref, tot_ref = through(c2_frames, monkeypatch, 8, pipeline_frames=0, **cfg)
    assert ref.stream_plan()["streams"] == 3 and tot_ref["n_voxel_updates"] > 16 * 100000, (ref.stream_plan(), tot_ref)
    b = env_budget()
    for budget, want in ((None, dict(budget=b, streams=min(6, max(4, b)) if b < 8 else 6)), (8, dict(budget=8, streams=6, long="own", xlong="own"))):
        g, tot = through(c2_frames, monkeypatch, budget, pipeline_frames=pipeline, **cfg)
        plan = g.stream_plan()
        print("pipeline", pipeline, "budget", budget, plan)
        assert {k: plan[k] for k in want} == want, (plan, want)
        assert plan["march_streams"] == 2 and plan["streams_held"] == plan["streams"], plan
        assert (plan["long"], plan["xlong"]) == {4: ("tail", "tail"), 5: ("own", "tail"), 6: ("own", "own")}[plan["streams"]], plan
        rep = same_map(ref, tot_ref, g, tot)
        assert rep["oracle_touched"] > 100000, rep
        g.close()
    ref.close()


def test_merged_keeps_its_plan_and_its_map(monkeypatch):
    fr = frames(10)
    cfg = dict(method=1, max_tiles=1 << 13, max_points=640 * 480)
    ref, tot_ref = through(fr, monkeypatch, 8, pipeline_frames=0, **cfg)
    at8, tot8 = through(fr, monkeypatch, 8, pipeline_frames=8, **cfg)
    g, tot = through(fr, monkeypatch, None, pipeline_frames=8, **cfg)
    plan, plan8 = g.stream_plan(), at8.stream_plan()
    print(plan, plan8)
    assert plan8["streams"] == 4 and (plan8["long"], plan8["xlong"], plan8["march"]) == ("own", "own", "A"), plan8
    if env_budget() >= 4:
        assert {k: v for k, v in plan.items() if k != "budget"} == {k: v for k, v in plan8.items() if k != "budget"}, (plan, plan8)
    same_map(ref, tot_ref, at8, tot8)
    same_map(ref, tot_ref, g, tot)
    for h in (g, at8, ref):
        h.close()


def test_fast_at_2_cm_keeps_its_plan_and_its_map(monkeypatch):
    """2 cm voxels, 10 m rays: the default mode runs one frame at a time there whatever pipeline_frames asks for: three streams."""
    fr = frames(3, w=320, h=240, scene="hall", radius=3.0)
    cfg = dict(method=0, max_tiles=1 << 16, max_points=320 * 240, voxel_size=0.02, truncation_distance=0.08, max_ray_length_m=10.0)
    at8, tot8 = through(fr, monkeypatch, 8, pipeline_frames=12, **cfg)
    g, tot = through(fr, monkeypatch, None, pipeline_frames=12, **cfg)
    plan, plan8 = g.stream_plan(), at8.stream_plan()
    print(plan, plan8)
    assert g.pipeline_shape()["lag"] == 0 and plan8["streams"] == 3 and (plan8["long"], plan8["xlong"]) == ("own", "own"), (g.pipeline_shape(), plan8)
    if env_budget() >= 3:
        assert {k: v for k, v in plan.items() if k != "budget"} == {k: v for k, v in plan8.items() if k != "budget"}, (plan, plan8)
    assert tot["n_voxel_updates"] > 1000000, tot
    same_map(at8, tot8, g, tot)
    g.close()
    at8.close()
