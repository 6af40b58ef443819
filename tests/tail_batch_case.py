"""The tail of a batch of frames in one pass (csrc/ks_hip.hip: tail_batch; ks_tail_batch_stats): one sort and one voxel update for
the frames whose stage B went out together.  The cases of tests/test_tail_batch_gpu.py (in process, on the device) and of
tests/test_tail_batch_emu.py (one child process per case on the host functional model, tools/emu/README.md):
KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.tail_batch_case '<json spec>'.

A case runs the same frames through the same pipelined `fast` context twice — with the default tail and with KS_DEBUG=1
KS_TAIL_BATCH=0, every frame's tail on its own — and asserts: the same blocks in the same order, the same set of tile keys, every voxel
record of every block equal byte for byte, the same ks_frame_stats (or error code) at every call, ks_tail_batch_stats says that
the path the case means to test was taken, and (spec["oracle"]) both maps equal the serial CPU oracle's bit for bit
(tests.util.compare_maps).

spec: size [w, h]; frames; pipeline; stride (trajectory_pose(stride * i); 0: every frame from one pose); subsample (point
counts, cycled over the frames); color_mode; growth (early_out_phase_growth: 0 = the reference's serial order, 32 = ordered
phases); bad_label (index of a frame that carries a label outside the table); big (index of a frame of 3 x the size, with
cap_marks: the marks of that frame do not fit KS_EXACT_CAP_MARKS, its fix point falls back to the host-driven loop);
no_early_out (max_consecutive_ray_collisions = 2^30: every ray reaches the sensor, whose voxel collects a run per frame);
min_batches / min_per_frame: what ks_tail_batch_stats has to report for the default run at least."""
import json
import os
import sys

import numpy as np

STAT_FIELDS = ("n_points", "n_valid_points", "n_rays_cast", "n_voxel_updates", "n_blocks_allocated")
KNOBS = ("KS_DEBUG", "KS_TAIL_BATCH", "KS_EXACT_CAP_MARKS")


def frames_of(spec):
    from kimera_semantics_amd import synth
    sc = synth.make_scene("room")
    w, h = spec.get("size", (64, 48))
    stride = spec.get("stride", 3)
    sub = spec.get("subsample")
    rng = np.random.default_rng(11)
    out = []
    for i in range(spec["frames"]):
        big = i == spec.get("big", -1)
        pose = synth.trajectory_pose(stride * i) if stride else synth.single_pose()
        f = synth.render_frame(sc, pose, 3 * w if big else w, 3 * h if big else h, seed=900 + i)
        xyz, rgba, labels = f.xyz, f.rgba, f.labels.copy()
        if sub:
            keep = np.sort(rng.choice(len(xyz), size=min(len(xyz), sub[i % len(sub)]), replace=False))
            xyz, rgba, labels = xyz[keep], rgba[keep], labels[keep]
        if i == spec.get("bad_label", -1):
            labels[len(labels) // 2] = 200
        out.append((f.T_G_C, xyz, rgba, labels))
    return out


def config(spec, **kw):
    from kimera_semantics_amd import binding as B
    from tests.util import COMMON
    cfg = dict(COMMON, method=0, color_mode=spec.get("color_mode", 1))
    growth = spec.get("growth", 0)
    cfg["early_out_phase_growth"] = growth if growth else B.KS_EARLY_OUT_EXACT
    if spec.get("no_early_out"):
        cfg["max_consecutive_ray_collisions"] = 1 << 30   # every ray walks back to the sensor: the voxels around it collect the long runs
    cfg.update(kw)
    return cfg


def through(spec, frames, batched):
    """The frames through a pipelined context; returns (integrator, what every call returned, ks_tail_batch_stats)."""
    from kimera_semantics_amd import binding as B
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    if not batched or spec.get("cap_marks"):
        os.environ["KS_DEBUG"] = "1"
    if not batched:
        os.environ["KS_TAIL_BATCH"] = "0"
    if spec.get("cap_marks"):
        os.environ["KS_EXACT_CAP_MARKS"] = str(spec["cap_marks"])
    try:
        g = B.HipIntegrator(B.default_config(max_tiles=spec.get("max_tiles", 4096), max_points=spec.get("max_points", 1 << 16),
                                             pipeline_frames=spec["pipeline"], **config(spec)))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    calls = []
    for T, xyz, rgba, labels in frames:
        try:
            st = g.integrate(T, xyz, rgba, labels)
            calls.append(tuple(getattr(st, k) for k in STAT_FIELDS))
        except B.KsError as e:
            calls.append(("error", e.code))
    while True:   # (a flush reports the first error of the frames it completes and is called again for the rest)
        try:
            st = g.flush()
            calls.append(tuple(getattr(st, k) for k in STAT_FIELDS))
            break
        except B.KsError as e:
            calls.append(("error", e.code))
    return g, calls, g.tail_batch_stats()


def same_maps(a, b):
    ia, ib = a.block_indices(), b.block_indices()
    assert ia.tobytes() == ib.tobytes(), "the block lists differ"
    # (the same tiles; which pool slot a tile got is decided by an atomic counter among the lanes that allocate in one launch)
    assert np.sort(a.tile_keys()).tobytes() == np.sort(b.tile_keys()).tobytes(), "the tile keys differ"
    _, ta, sa = a.download(ia)
    _, tb, sb = b.download(ib)
    assert ta.tobytes() == tb.tobytes() and sa.tobytes() == sb.tobytes(), "voxel records differ"
    return len(ia)


def run(spec):
    from tests.util import compare_maps
    frames = frames_of(spec)
    g1, calls1, st1 = through(spec, frames, batched=True)
    g0, calls0, st0 = through(spec, frames, batched=False)
    rep = {"default": st1, "switch": st0}
    assert st0["batches"] == 0 and st0["frames"] == 0 and st0["pairs"] == 0, st0
    assert st1["batches"] >= spec.get("min_batches", 0), st1
    assert st1["per_frame_batches"] >= spec.get("min_per_frame", 0), st1
    if "batches" in spec:
        assert (st1["batches"], st1["frames"]) == tuple(spec["batches"]), st1
    assert calls1 == calls0, (calls1, calls0)
    rep["blocks"] = same_maps(g1, g0)
    rep["updates"] = sum(c[3] for c in calls1 if c[0] != "error")
    if st1["batches"] and not any(c[0] == "error" for c in calls1) and not st1["per_frame_batches"]:
        assert st1["pairs"] == rep["updates"], (st1, rep)
    if spec.get("oracle", True):
        from oracle import oracle_py as O
        ocfg = config(spec)
        ocfg["early_out_phase_growth"] = spec.get("growth", 0)
        o = O.Oracle(O.default_config(integrator_threads=1, **ocfg))
        for T, xyz, rgba, labels in frames:
            o.integrate(T, xyz, rgba, labels)
        for g in (g1, g0):
            r = compare_maps(o, g, exact=True)
        assert r["oracle_touched"] > spec.get("min_voxels", 500), r
        rep["voxels"] = r["oracle_touched"]
        o.close()
    g1.close()
    g0.close()
    return rep


# name -> spec: the cases of the GPU tier (frames of 160 x 120 at most) ...
GPU_CASES = {
    "default_against_switch": dict(size=(96, 72), frames=11, pipeline=12, batches=(3, 11)),
    "batches_of_eight": dict(size=(64, 48), frames=19, pipeline=16, batches=(3, 19)),
    "across_a_power_of_two": dict(size=(96, 72), frames=11, pipeline=12, subsample=(4000, 4200, 4096, 4097), batches=(3, 11)),
    "long_only_when_merged": dict(size=(32, 24), frames=8, pipeline=16, stride=0, no_early_out=True, batches=(1, 8)),
    "color_mode_color": dict(size=(64, 48), frames=11, pipeline=12, color_mode=0, batches=(3, 11)),
    "ordered_phases": dict(size=(64, 48), frames=11, pipeline=12, growth=32, batches=(3, 11)),
    "error_in_a_batch": dict(size=(64, 48), frames=11, pipeline=12, bad_label=5, oracle=False, min_per_frame=1, min_batches=1),
    "fallback_in_a_batch": dict(size=(16, 12), frames=16, pipeline=12, big=5, cap_marks=30000, max_points=1 << 13, min_per_frame=1, min_batches=1),
    "slot_reuse": dict(size=(48, 36), frames=30, pipeline=12, max_tiles=1 << 15, batches=(8, 30)),   # (max_tiles: the pool never grows — growing drains the pipeline in mid-batch)
}
# ... and of the CPU tier, on the functional model (the first, third and seventh at 64 x 48)
EMU_CASES = {
    "default_against_switch": dict(GPU_CASES["default_against_switch"], size=(64, 48)),
    "across_a_power_of_two": dict(GPU_CASES["across_a_power_of_two"], size=(64, 48), subsample=(2000, 2100, 2048, 2049)),
    "error_in_a_batch": dict(GPU_CASES["error_in_a_batch"], size=(64, 48)),
}


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("TAIL_BATCH_OK", json.dumps(run(spec)))


if __name__ == "__main__":
    main()
