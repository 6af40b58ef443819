"""The early-out seed's work list (k_seed_list -> k_test, csrc/ks_k_march.h) against the oracle, on frames whose sizes sit at the
edges of the ordered-phase schedule, integrated into contexts whose CAPACITY is larger than the frame (the seed's launches are
sized by the capacity, ks_seed_launch_shape).  Shared by tests/test_seed_worklist_emu.py (a subprocess on the host functional
model: KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.seed_case '<json spec>') and tests/test_seed_worklist_gpu.py
(in process, on the GPU).  The checker is the oracle: update counts frame by frame, then the maps bit for bit."""
import json
import os
import sys

import numpy as np

# 1 = the smallest frame; 1023 / 1024 = one generation of 1024 chains / 1024 generations of one chain in the default order;
# 2047 = the most generations any frame has (one chain); 2048 = two chains; 3047 = two chains, the frame that reaches furthest
# into the generations beyond 1024 with more than one chain; 5000 = no multiple of 1024
SIZES = (1, 1023, 1024, 2047, 2048, 3047, 5000)
CAPACITY = 7000   # > every frame above


def lattice_frame(n_side=(40, 30), spacing=0.12, depth=2.0, seed=0):
    """Points 12 cm apart on a plane in front of the camera: every point has a start voxel of its own, so every ray survives
    the start-voxel dedup (all live)."""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(n_side[0]), np.arange(n_side[1]))
    xyz = np.stack([(u - n_side[0] / 2) * spacing + 0.01, (v - n_side[1] / 2) * spacing + 0.01, np.full(u.shape, depth)], axis=-1)
    xyz = xyz.reshape(-1, 3).astype(np.float32)
    labels = rng.integers(0, 20, size=len(xyz), dtype=np.uint8)
    return xyz, labels


def frames_of(spec):
    """[(T_G_C, xyz, rgba, labels, what)] of a spec: one frame per size, then the all-live and the none-live frame."""
    from kimera_semantics_amd import synth
    colors = synth.default_label_colors()
    sc = synth.make_scene("room")
    out = []
    for k, n in enumerate(spec.get("sizes", SIZES)):
        f = synth.render_frame(sc, synth.trajectory_pose(7 * k), 96, 72, seed=90 + k)
        assert len(f.xyz) >= n, (len(f.xyz), n)
        out.append((f.T_G_C, f.xyz[:n].copy(), f.rgba[:n].copy(), f.labels[:n].copy(), "n=%d" % n))
    if spec.get("all_live", True):
        xyz, labels = lattice_frame()
        out.append((synth.pose_to_T((-1.0, 0.2, 1.4), 0.3), xyz, colors[labels], labels, "all live"))
    if spec.get("none_live", True):
        f = synth.render_frame(sc, synth.trajectory_pose(3), 64, 48, seed=77)
        labels = np.full(len(f.xyz), 20, np.uint8)   # tests.util.COMMON: label 20 is dynamic — no point of the frame casts a ray
        out.append((f.T_G_C, f.xyz, colors[labels], labels, "none live"))
    for w, h, k in spec.get("full_frames", []):   # e.g. [640, 480, 12]: a frame sequence at the context's own capacity
        for i in range(k):
            f = synth.render_frame(sc, synth.trajectory_pose(5 * i), w, h, seed=300 + i)
            out.append((f.T_G_C, f.xyz, f.rgba, f.labels, "%dx%d #%d" % (w, h, i)))
    return out


def run(spec):
    """spec: mode = "phased" (early_out_phase_growth = 32 against the oracle's restatement integrate_fast_phased) | "serial" (the
    default: the reference's serial result); pipeline = ks_config.pipeline_frames; capacity; sizes / all_live / none_live /
    full_frames as in frames_of; order = integration_order_mode."""
    from kimera_semantics_amd import binding as B
    from oracle import oracle_py as O
    from tests.util import COMMON, compare_maps
    cfg = dict(COMMON, method=0, integration_order_mode=spec.get("order", 0))
    ocfg, hcfg = dict(cfg), dict(cfg)
    if spec["mode"] == "phased":
        ocfg["early_out_phase_growth"] = hcfg["early_out_phase_growth"] = 32
    else:
        ocfg["early_out_phase_growth"] = 0
        hcfg["early_out_phase_growth"] = B.KS_EARLY_OUT_EXACT
    o = O.Oracle(O.default_config(integrator_threads=1, **ocfg))
    g = B.HipIntegrator(B.default_config(max_tiles=spec.get("max_tiles", 8192), max_points=spec.get("capacity", CAPACITY),
                                         pipeline_frames=spec.get("pipeline", 0), **hcfg))
    tot_o = tot_g = rays_o = rays_g = 0
    for T, xyz, rgba, labels, what in frames_of(spec):
        so = o.integrate(T, xyz, rgba, labels)
        sg = g.integrate(T, xyz, rgba, labels)
        if what == "all live":
            assert so.n_rays_cast == len(xyz), (what, so.n_rays_cast, len(xyz))
        if what == "none live":
            assert so.n_rays_cast == 0, (what, so.n_rays_cast)
        if not spec.get("pipeline", 0):   # (a pipelined call reports the frame that completed, not the one it was given)
            assert (so.n_rays_cast, so.n_voxel_updates) == (sg.n_rays_cast, sg.n_voxel_updates), (what, so.n_rays_cast, sg.n_rays_cast, so.n_voxel_updates, sg.n_voxel_updates)
        tot_o += so.n_voxel_updates
        rays_o += so.n_rays_cast
        tot_g += sg.n_voxel_updates
        rays_g += sg.n_rays_cast
    sf = g.flush()
    tot_g += sf.n_voxel_updates
    rays_g += sf.n_rays_cast
    assert (tot_o, rays_o) == (tot_g, rays_g), (tot_o, tot_g, rays_o, rays_g)
    rep = compare_maps(o, g, exact=True)
    assert rep["oracle_touched"] > 500, rep
    g.close()
    o.close()
    return {"updates": tot_g, "rays": rays_g, "voxels": rep["oracle_touched"]}


def run_overflow(spec):
    """KS_DEBUG=1 KS_SEED_CAP_ITEMS=<few> (set by the caller before the context is created): a frame with more work items than a
    phase's launch covers ends in the error path — KS_ERR_INDEX_RANGE, nothing of the frame applied — and not in a map that
    lacks the rays beyond the launch."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    from tests.util import COMMON
    assert os.environ.get("KS_DEBUG") == "1" and os.environ.get("KS_SEED_CAP_ITEMS")
    cfg = dict(COMMON, method=0)
    cfg["early_out_phase_growth"] = 32 if spec["mode"] == "phased" else B.KS_EARLY_OUT_EXACT
    g = B.HipIntegrator(B.default_config(max_tiles=2048, max_points=CAPACITY, pipeline_frames=0, **cfg))
    f = synth.render_frame(synth.make_scene("room"), synth.single_pose(), 64, 48, seed=5)
    try:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    except B.KsError as e:
        assert e.code == -6, e.code   # KS_ERR_INDEX_RANGE
    else:
        raise AssertionError("a frame whose work list does not fit its launch was integrated")
    assert len(g.block_indices()) == 0   # the map is what it was: empty
    g.close()
    return {"error": -6}


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    rep = run_overflow(spec) if spec.get("overflow") else run(spec)
    print("SEED_CASE_OK", json.dumps(rep))


if __name__ == "__main__":
    main()
