"""GPU tier of the navigation field: the cases of tests/nav_case.py on the real device (the same sizes as on the functional model),
one larger map planned while a frame is in flight, the device-pointer calls on torch tensors, the adapter, and two updates in one
process.  The checker is tests/nav_model.py on the stored ESDF as the library hands it out; every comparison is exact, the five
contractual statistics included."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import esdf_model, nav_case
from tests import esdf_read_model as E
from tests import nav_model as M

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.mark.parametrize("name", sorted(nav_case.SPECS))
def test_nav_equals_model(name, monkeypatch):
    spec, env = nav_case.SPECS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nav_case.run_case(spec)


def test_larger_map_planned_with_a_frame_in_flight_equals_model():
    """Four 160x120 frames at 5 cm through the frame pipeline (pipeline_frames = 12).  The ESDF is made after two frames and refreshed
    after the third; the fourth is in flight when the field is made from the store as the refresh left it.  Two goals, 2000 starts."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    from tests.util import COMMON
    sc = synth.make_scene("room")
    frames = [synth.render_frame(sc, synth.trajectory_pose(k, radius=1.5), 160, 120, hfov_deg=90.0, seed=k) for k in range(4)]
    g = B.HipIntegrator(B.default_config(method=0, voxel_size=0.05, voxels_per_side=16, truncation_distance=0.2, max_ray_length_m=5.0,
                                         max_tiles=1 << 13, max_points=160 * 120, pipeline_frames=12, **COMMON))
    for f in frames[:2]:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.esdf_update(min_distance_m=0.1, max_distance_m=1.0)
    g.integrate(frames[2].T_G_C, frames[2].xyz, frames[2].rgba, frames[2].labels)
    g.esdf_refresh()
    g.integrate(frames[3].T_G_C, frames[3].xyz, frames[3].rgba, frames[3].labels)
    goals = np.array([frames[0].T_G_C[4:7], frames[2].T_G_C[4:7]], F)
    full = g.nav_update(goals, radius_m=0.15)
    M.assert_field(g, full, M.model_of(g, goals, radius_m=0.15), "larger map, no cap")
    # ... and with a cap of about 2.5 m of travel, which leaves the far side of the room unreached
    stats = g.nav_update(goals, radius_m=0.15, max_cost=500)
    model = M.model_of(g, goals, radius_m=0.15, max_cost=500)
    idx, blocks = M.assert_field(g, stats, model, "larger map")
    assert stats["voxels_traversable"] == full["voxels_traversable"] and stats["voxels_reached"] < full["voxels_reached"] and stats["largest_cost"] <= 500
    rng = np.random.default_rng(13)
    free = np.argwhere(blocks != M.BLOCKED)                                      # half of the starts in traversable voxels, half anywhere
    pick = free[rng.choice(len(free), 1000, replace=False)]
    local = np.stack([pick[:, 1] % 16, (pick[:, 1] // 16) % 16, pick[:, 1] // 256], axis=1)
    side = 16 * 0.05
    lo, hi = idx.min(axis=0) * side, (idx.max(axis=0) + 1) * side
    starts = np.concatenate([(idx[pick[:, 0]] * 16 + local + rng.uniform(0.1, 0.9, (1000, 3))) * 0.05, rng.uniform(lo - 0.2, hi + 0.2, (1000, 3))]).astype(F)
    got = g.nav_paths(starts, 256)
    print("field", stats, "paths", got["stats"])
    M.assert_paths(got, M.paths(model, starts, 256), "2000 starts")
    assert (g.nav_query(starts) == model.query(starts)).all()
    assert stats["goals_used"] == 2 and full["voxels_reached"] > 10000
    assert min(got["stats"][k] for k in ("paths_reached", "paths_unreachable", "paths_blocked")) > 0, got["stats"]
    g.close()


def test_device_pointer_calls_on_torch_tensors_equal_the_host_calls():
    """The two _device entries on ks_stream(ctx): with stats the call has waited for the kernel and the bytes are the host entry's;
    without, the tensors are read after torch.cuda.synchronize().  Outputs that are not asked for are not written, nor are the rows
    of `waypoints` from n_waypoints on."""
    import torch
    vox = nav_case.random_voxels()
    g = nav_case._stored("random", 16)
    g.nav_update(nav_case.random_goals(vox), radius_m=nav_case.RADIUS)
    starts, mw = nav_case.path_starts(), 48
    want, want_q = g.nav_paths(starts, mw), g.nav_query(starts)
    n = len(starts)
    d_starts = torch.from_numpy(starts).to("cuda")
    ptr = lambda t: t.data_ptr()

    def tensors():
        return dict(status=torch.full((n,), 9, dtype=torch.uint8, device="cuda"), cost=torch.full((n,), 9, dtype=torch.int32, device="cuda"),
                    n_waypoints=torch.full((n,), 9, dtype=torch.int32, device="cuda"),
                    waypoints=torch.full((n, mw, 3), float(g.NAV_WAYPOINT_FILL), dtype=torch.float32, device="cuda"))

    def same(t, keys):
        for k in keys:
            assert t[k].cpu().numpy().tobytes() == np.ascontiguousarray(want[k]).tobytes(), k

    names = ("status", "cost", "n_waypoints", "waypoints")
    t = tensors()
    torch.cuda.synchronize()
    assert g.nav_paths_device(ptr(d_starts), n, mw, *[ptr(t[k]) for k in names]) == want["stats"]
    same(t, names)
    t = tensors()
    torch.cuda.synchronize()
    assert g.nav_paths_device(ptr(d_starts), n, mw, d_cost=ptr(t["cost"]), d_waypoints=ptr(t["waypoints"]), stats=False) is None
    torch.cuda.synchronize()
    same(t, ("cost", "waypoints"))
    assert (t["status"].cpu().numpy() == 9).all() and (t["n_waypoints"].cpu().numpy() == 9).all()
    q = torch.full((n,), 9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.nav_query_device(ptr(d_starts), n, ptr(q))
    torch.cuda.synchronize()
    assert q.cpu().numpy().view(np.uint32).tobytes() == want_q.tobytes()
    g.close()


def test_two_updates_in_one_process_give_identical_bytes():
    vox = nav_case.random_voxels()
    goals = nav_case.random_goals(vox)
    g = nav_case._stored("random", 8)
    idx = g.block_indices()
    first = g.nav_update(goals, radius_m=nav_case.RADIUS)
    a = g.nav_blocks(idx)
    second = g.nav_update(goals, radius_m=nav_case.RADIUS)
    assert g.nav_blocks(idx).tobytes() == a.tobytes()
    assert {k: first[k] for k in M.STAT_KEYS} == {k: second[k] for k in M.STAT_KEYS}
    g.close()


def test_adapter_field_and_paths_equal_model_on_the_layers_it_synced(tmp_path):
    """HipSemanticTsdfIntegrator::updateNavField and ::planPaths after updateEsdf (adapter_demo, KS_DEMO_NAV) against the model on the
    ESDF model of the layers the demo wrote."""
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import test_host_adapter_gpu as A
    from tests.util import NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    csv, fin, fout, fnav = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin", "nav.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    A._write_in(fin, A._frames())
    res = subprocess.run([A.DEMO, "fast", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True, env=dict(os.environ, KS_DEMO_NAV=fnav))
    assert res.returncode == 0 and "adapter_demo: updateNavField + planPaths" in res.stdout, res.stdout + res.stderr
    idx, t, s = A._read_out(fout)
    # the demo's options (adapter_demo.cpp): min_distance_m 0.1, max_distance_m 0.4; radius 0.2, at most 96 waypoints
    esdf = esdf_model.esdf_from_blocks(idx, t, s["label"], 16, 0.05, min_distance_m=0.1, max_distance_m=0.4)
    store = E.Store(idx, esdf.blocks(idx), 16)
    buf = open(fnav, "rb").read()
    ng, ns, mw = struct.unpack_from("<III", buf, 0)
    assert (ng, ns, mw) == (2, 13 ** 3, 96)
    off = 12
    take = lambda dtype, count, shape: np.frombuffer(buf, dtype, count, off).reshape(shape)
    goals = take("<f4", 3 * ng, (ng, 3)); off += 12 * ng
    starts = take("<f4", 3 * ns, (ns, 3)); off += 12 * ns
    status = take(np.uint8, ns, (ns,)); off += ns
    cost = take("<u4", ns, (ns,)); off += 4 * ns
    count = take("<u4", ns, (ns,)); off += 4 * ns
    assert len(buf) == off + 12 * int(count.sum())
    want = M.paths(M.field(store, goals, 0.05, radius_m=0.2), starts, mw)
    assert status.tobytes() == want["status"].tobytes() and cost.tobytes() == want["cost"].tobytes() and count.tobytes() == want["n_waypoints"].tobytes()
    flat = take("<f4", 3 * int(count.sum()), (-1, 3))
    rows = np.arange(mw)[None, :] < count[:, None]
    assert flat.tobytes() == want["waypoints"][rows].tobytes()
    assert want["stats"]["paths_reached"] > 50 and want["stats"]["paths_blocked"] > 50, want["stats"]
