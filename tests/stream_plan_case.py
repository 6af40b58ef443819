"""The stream plan (csrc/ks_hip.hip: stream_plan; ks_stream_plan) on the host functional model, whose runtime stand-in keeps a
ledger of the live streams (tools/emu/README.md).  One child process per case of tests/test_stream_plan_emu.py:
KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.stream_plan_case '<json spec>'.

{"table": 1}:  every context of CONTEXTS at every budget of BUDGETS: ks_stream_plan equals TABLE, the ledger's live-stream count
               equals the plan's distinct-stream count after ks_create, the ledger is back where it was after ks_destroy.
{"stream": {"pipeline": p, "budget": b}}:  a stream of frames through a pipelined default-mode context at that budget leaves
               the map and the frame statistics of the unpipelined context, bit for bit (tests.util.compare_maps)."""
import json
import os
import sys

BUDGETS = (1, 3, 4, 5, 6, 8, 32)

CONTEXTS = {
    "fast_p0": dict(method=0, pipeline_frames=0),
    "fast_p4": dict(method=0, pipeline_frames=4),
    "fast_p8": dict(method=0, pipeline_frames=8),
    "fast_p12": dict(method=0, pipeline_frames=12),
    "fast_p16": dict(method=0, pipeline_frames=16),
    "phased_p4": dict(method=0, pipeline_frames=4, early_out_phase_growth=32),
    "phased_p12": dict(method=0, pipeline_frames=12, early_out_phase_growth=32),
    "merged_p0": dict(method=1, pipeline_frames=0),
    "merged_p8": dict(method=1, pipeline_frames=8),
}

# Written out by hand from the rule (stage A, the march streams and stage T keep their streams; below a budget of 8, while the
# context would need more streams than the budget, xlong and then long run on the stage-T stream).
# context -> (march streams, march, tail, {budget: (distinct streams, long, xlong)})
_ALL = ("own", "own")
_X = ("own", "tail")      # xlong folded
_LX = ("tail", "tail")    # both folded
TABLE = {
    # unpipelined: A (= B = T), long, xlong
    "fast_p0": (1, "A", "A", {1: (1,) + _LX, 3: (3,) + _ALL, 4: (3,) + _ALL, 5: (3,) + _ALL, 6: (3,) + _ALL, 8: (3,) + _ALL, 32: (3,) + _ALL}),
    "merged_p0": (1, "A", "A", {1: (1,) + _LX, 3: (3,) + _ALL, 4: (3,) + _ALL, 5: (3,) + _ALL, 6: (3,) + _ALL, 8: (3,) + _ALL, 32: (3,) + _ALL}),
    # a frame's stage B as its own launch sequence, four of them side by side: A, 4 x B, T, long, xlong
    "fast_p4": (4, "own", "own", {1: (6,) + _LX, 3: (6,) + _LX, 4: (6,) + _LX, 5: (6,) + _LX, 6: (6,) + _LX, 8: (8,) + _ALL, 32: (8,) + _ALL}),
    "phased_p4": (4, "own", "own", {1: (6,) + _LX, 3: (6,) + _LX, 4: (6,) + _LX, 5: (6,) + _LX, 6: (6,) + _LX, 8: (8,) + _ALL, 32: (8,) + _ALL}),
    # the default mode in batches (four frames per launch sequence, eight at a lag of 16), two batches alternating: A, 2 x B, T, long, xlong
    "fast_p8": (2, "own", "own", {1: (4,) + _LX, 3: (4,) + _LX, 4: (4,) + _LX, 5: (5,) + _X, 6: (6,) + _ALL, 8: (6,) + _ALL, 32: (6,) + _ALL}),
    "fast_p12": (2, "own", "own", {1: (4,) + _LX, 3: (4,) + _LX, 4: (4,) + _LX, 5: (5,) + _X, 6: (6,) + _ALL, 8: (6,) + _ALL, 32: (6,) + _ALL}),
    "fast_p16": (2, "own", "own", {1: (4,) + _LX, 3: (4,) + _LX, 4: (4,) + _LX, 5: (5,) + _X, 6: (6,) + _ALL, 8: (6,) + _ALL, 32: (6,) + _ALL}),
    # ordered phases in batches: one march stream: A, B, T, long, xlong
    "phased_p12": (1, "own", "own", {1: (3,) + _LX, 3: (3,) + _LX, 4: (4,) + _X, 5: (5,) + _ALL, 6: (5,) + _ALL, 8: (5,) + _ALL, 32: (5,) + _ALL}),
    # `merged` has no early-out: stage B follows stage A on its stream: A (= B), T, long, xlong
    "merged_p8": (1, "A", "own", {1: (2,) + _LX, 3: (3,) + _X, 4: (4,) + _ALL, 5: (4,) + _ALL, 6: (4,) + _ALL, 8: (4,) + _ALL, 32: (4,) + _ALL}),
}


def ledger():
    from tests.ownership_case import ledger as L
    return L()[0]   # (live blocks, live bytes, live events, live streams)


def config(**kw):
    from kimera_semantics_amd import binding as B
    from tests.util import COMMON
    base = dict(COMMON, max_tiles=64, max_points=1024)
    base.update(kw)
    return B.default_config(**base)


def ambient_budget():
    """What the library makes of the runtime's own variable as this process inherited it (the tests never write it): 4 when it is
    unset or no number, 1 .. 32."""
    try:
        return min(32, max(1, int(os.environ.get("GPU_MAX_HW_QUEUES", ""))))
    except ValueError:
        return 4


def set_budget(b):
    """The budget of the NEXT ks_create, through the debug switch (None: the environment as the process inherited it)."""
    for k in ("KS_DEBUG", "KS_HW_QUEUES"):
        os.environ.pop(k, None)
    if b is not None:
        os.environ["KS_DEBUG"] = "1"
        os.environ["KS_HW_QUEUES"] = str(b)


def run_table():
    from kimera_semantics_amd import binding as B
    checked = 0
    for name, kw in CONTEXTS.items():
        n_march, march, tail, rows = TABLE[name]
        for b in BUDGETS:
            set_budget(b)
            before = ledger()
            g = B.HipIntegrator(config(**kw))
            plan = g.stream_plan()
            streams, long_, xlong = rows[b]
            want = dict(budget=b, streams=streams, march_streams=n_march, long=long_, xlong=xlong, march=march, tail=tail, streams_held=streams)
            assert plan == want, (name, b, plan, want)
            assert g.pipeline_shape()["march_streams"] == n_march, (name, b)
            live = ledger()
            assert live[3] - before[3] == plan["streams"], (name, b, live, before, plan)
            g.close()
            assert ledger() == before, (name, b, ledger(), before)
            checked += 1
    # the budget itself: the runtime's variable as inherited when nothing overrides it; the override only behind the KS_DEBUG gate;
    # no number = no override; clamped to 1 .. 32
    amb = ambient_budget()
    for env, want in (({}, amb), ({"KS_HW_QUEUES": "7"}, amb), ({"KS_HW_QUEUES": "7", "KS_DEBUG": "1"}, 7), ({"KS_HW_QUEUES": "x", "KS_DEBUG": "1"}, amb),
                      ({"KS_HW_QUEUES": "", "KS_DEBUG": "1"}, amb), ({"KS_HW_QUEUES": "0", "KS_DEBUG": "1"}, 1), ({"KS_HW_QUEUES": "-3", "KS_DEBUG": "1"}, 1),
                      ({"KS_HW_QUEUES": "64", "KS_DEBUG": "1"}, 32)):
        set_budget(None)
        os.environ.update(env)
        g = B.HipIntegrator(config(**CONTEXTS["fast_p12"]))
        assert g.stream_plan()["budget"] == want, (env, g.stream_plan())
        g.close()
    set_budget(None)
    # KS_XLONG=0 (diagnostics): no such kernel, nothing to fold
    os.environ.update(KS_DEBUG="1", KS_XLONG="0", KS_HW_QUEUES="4")
    g = B.HipIntegrator(config(**CONTEXTS["fast_p12"]))
    assert g.stream_plan() == dict(budget=4, streams=4, march_streams=2, long="tail", xlong="none", march="own", tail="own", streams_held=4), g.stream_plan()
    g.close()
    return {"plans": checked}


BIG = (20,)   # the frame of the stream that outgrows max_points and KS_EXACT_CAP_MARKS


def stream_frames(count):
    """count small frames (16 x 12) that fit the context's max_points and its marks; the one of BIG (48 x 36) outgrows max_points
    (ensure_points grows every slot's buffers in mid-stream) and brings more marks than KS_EXACT_CAP_MARKS holds (the fallback
    to the host-driven loop — and, with it, of the frames in flight behind it — then the growth of the mark buffers)."""
    from kimera_semantics_amd import synth
    sc = synth.make_scene("room")
    out = []
    for i in range(count):
        w, h = (48, 36) if i in BIG else (16, 12)
        f = synth.render_frame(sc, synth.trajectory_pose(3 * i), w, h, seed=700 + i)
        out.append((f.T_G_C, f.xyz, f.rgba, f.labels))
    return out


STAT_FIELDS = ("n_points", "n_valid_points", "n_rays_cast", "n_voxel_updates", "n_blocks_allocated")


def run_stream(spec):
    from kimera_semantics_amd import binding as B
    from tests.util import compare_maps
    n_frames = spec.get("frames", 32)
    fr = stream_frames(n_frames)
    assert len(fr) >= 30 and max(len(f[1]) for i, f in enumerate(fr) if i not in BIG) <= 1024 < min(len(fr[i][1]) for i in BIG)

    def through(pipeline, budget):
        set_budget(budget)
        os.environ["KS_EXACT_CAP_MARKS"] = str(spec.get("cap_marks", 30000))   # (behind KS_DEBUG=1, which set_budget has set)
        g = B.HipIntegrator(config(method=0, max_tiles=4096, pipeline_frames=pipeline))
        os.environ.pop("KS_EXACT_CAP_MARKS")
        tot = dict.fromkeys(STAT_FIELDS, 0)
        for T, xyz, rgba, labels in fr:
            st = g.integrate(T, xyz, rgba, labels)
            for k in STAT_FIELDS:
                tot[k] += getattr(st, k)
        st = g.flush()
        for k in STAT_FIELDS:
            tot[k] += getattr(st, k)
        return g, tot

    ref, tot_ref = through(0, 8)
    assert ref.stream_plan()["streams"] == 3
    g, tot = through(spec["pipeline"], spec["budget"])
    plan = g.stream_plan()
    assert plan["budget"] == spec["budget"] and plan["streams"] == spec["streams"], plan
    eo = g.early_out_stats()
    assert eo["fallbacks"] >= spec.get("min_fallbacks", 1), eo   # (a frame went through the host-driven loop: the pipeline was drained for it)
    assert tot == tot_ref, (tot, tot_ref)
    assert tot["n_voxel_updates"] > 20000, tot
    rep = compare_maps(ref, g, exact=True)
    assert rep["oracle_touched"] > 2000, rep
    assert ref.block_indices().tobytes() == g.block_indices().tobytes()   # (the blocks, in the same order)
    g.close()
    ref.close()
    return {"updates": tot["n_voxel_updates"], "voxels": rep["oracle_touched"], "fallbacks": eo["fallbacks"], "plan": plan}


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    rep = run_table() if "table" in spec else run_stream(spec["stream"])
    print("STREAM_PLAN_OK", json.dumps(rep))


if __name__ == "__main__":
    main()
