"""GPU tier of path shortening: the cases of tests/path_shorten_case.py on the real device (the same sizes as on the functional
model), one larger map whose paths go from ks_nav_paths_device into ks_path_shorten_device on torch tensors with a frame in flight,
the adapter, and two calls in one process.  The checker is tests/path_shorten_model.py on the stored ESDF as the library hands it
out; every comparison is exact, the eight statistics included."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import esdf_model, path_shorten_case
from tests import esdf_read_model as E
from tests import nav_model as NM
from tests import path_shorten_model as M

pytestmark = pytest.mark.gpu
F = np.float32
NAMES = ("status", "n_waypoints", "waypoints", "length", "min_clearance")


@pytest.mark.parametrize("name", sorted(path_shorten_case.SPECS))
def test_path_shorten_equals_model(name, monkeypatch):
    spec, env = path_shorten_case.SPECS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    path_shorten_case.run_case(spec)


def larger_map():
    """Four 160x120 frames at 5 cm through the frame pipeline (pipeline_frames = 12).  The ESDF is made after two frames and refreshed
    after the third; the fourth is in flight when the field is planned and the paths are read from the store as the refresh left it."""
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
    g.nav_update(goals, radius_m=0.15)
    idx = g.block_indices()
    blocks = g.nav_blocks(idx)
    rng = np.random.default_rng(13)
    free = np.argwhere(blocks != NM.BLOCKED)                                     # half of the starts in traversable voxels, half anywhere
    pick = free[rng.choice(len(free), 1000, replace=False)]
    local = np.stack([pick[:, 1] % 16, (pick[:, 1] // 16) % 16, pick[:, 1] // 256], axis=1)
    side = 16 * 0.05
    lo, hi = idx.min(axis=0) * side, (idx.max(axis=0) + 1) * side
    starts = np.concatenate([(idx[pick[:, 0]] * 16 + local + rng.uniform(0.1, 0.9, (1000, 3))) * 0.05, rng.uniform(lo - 0.2, hi + 0.2, (1000, 3))]).astype(F)
    return g, starts


def test_paths_of_a_larger_map_shortened_on_torch_tensors_equal_model():
    """2000 starts: ks_nav_paths_device writes the paths into torch tensors and ks_path_shorten_device reads them there, with stats
    (the call has waited) and without (the tensors are read after torch.cuda.synchronize()), out of place and in place.  Blocked and
    unreachable starts have no waypoint: INVALID paths.  lookahead 32 keeps the model's sweeps to about a second."""
    import torch
    g, starts = larger_map()
    n, mw, cfg = len(starts), 256, dict(radius_m=0.15, lookahead=32)
    ptr = lambda t: t.data_ptr()
    d_starts = torch.from_numpy(starts).to("cuda")
    d_wp = torch.full((n, mw, 3), float(M.WAYPOINT_FILL), dtype=torch.float32, device="cuda")
    d_nw = torch.zeros((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nav_stats = g.nav_paths_device(ptr(d_starts), n, mw, d_n_waypoints=ptr(d_nw), d_waypoints=ptr(d_wp))
    wp, nw = d_wp.cpu().numpy(), d_nw.cpu().numpy().view(np.uint32)
    want = M.model_of(g, wp, nw, **cfg)
    print("paths", nav_stats, "shortened", want["stats"])
    assert want["stats"]["paths_ok"] > 100 and int((want["n_waypoints"][want["status"] == M.OK] < nw[want["status"] == M.OK]).sum()) > 100
    assert want["stats"]["paths_invalid"] == nav_stats["paths_blocked"] + nav_stats["paths_unreachable"] > 0
    assert want["stats"]["waypoints_out"] < want["stats"]["waypoints_in"]

    def tensors():
        return dict(status=torch.full((n,), 9, dtype=torch.uint8, device="cuda"), n_waypoints=torch.full((n,), 9, dtype=torch.int32, device="cuda"),
                    waypoints=torch.full((n, mw, 3), float(M.WAYPOINT_FILL), dtype=torch.float32, device="cuda"),
                    length=torch.full((n,), -7.0, dtype=torch.float32, device="cuda"), min_clearance=torch.full((n,), -7.0, dtype=torch.float32, device="cuda"))

    def host(t, keys):
        return {k: (t[k].cpu().numpy().view(np.uint32) if k == "n_waypoints" else t[k].cpu().numpy()) for k in keys}

    t = tensors()
    torch.cuda.synchronize()
    stats = g.shorten_paths_device(ptr(d_wp), ptr(d_nw), n, mw, *[ptr(t[k]) for k in NAMES], **cfg)
    M.assert_same(dict(host(t, NAMES), stats=stats), want, "with stats")
    t = tensors()
    torch.cuda.synchronize()
    assert g.shorten_paths_device(ptr(d_wp), ptr(d_nw), n, mw, d_waypoints_out=ptr(t["waypoints"]), d_length=ptr(t["length"]), stats=False, **cfg) is None
    torch.cuda.synchronize()
    M.assert_same(host(t, ("waypoints", "length")), want, "without stats")
    assert (t["status"].cpu().numpy() == 9).all() and (t["n_waypoints"].cpu().numpy() == 9).all() and (t["min_clearance"].cpu().numpy() == -7.0).all()
    # in place: the tensor ks_nav_paths_device wrote is input and output
    t = tensors()
    torch.cuda.synchronize()
    stats = g.shorten_paths_device(ptr(d_wp), ptr(d_nw), n, mw, ptr(t["status"]), ptr(t["n_waypoints"]), ptr(d_wp), ptr(t["length"]), ptr(t["min_clearance"]), **cfg)
    got = dict(host(t, ("status", "n_waypoints", "length", "min_clearance")), waypoints=d_wp.cpu().numpy(), stats=stats)
    M.assert_same(got, want, "in place", in_place_of=wp)
    # ... and the host entry on the same arrays
    M.assert_same(g.shorten_paths(wp, nw, **cfg), want, "host entry")
    g.close()


def test_two_calls_in_one_process_give_identical_bytes():
    g = path_shorten_case.stored("sphere", 8)
    wp, nw = path_shorten_case.many_paths()
    a = g.shorten_paths(wp, nw, radius_m=path_shorten_case.SPHERE_RADIUS, lookahead=70)
    b = g.shorten_paths(wp, nw, radius_m=path_shorten_case.SPHERE_RADIUS, lookahead=70)
    for k in NAMES:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["stats"] == b["stats"] and a["stats"]["paths_ok"] > 0 and a["stats"]["paths_unverified"] > 0
    g.close()


def test_adapter_shortened_paths_equal_model_on_the_layers_it_synced(tmp_path):
    """HipSemanticTsdfIntegrator::shortenPaths after planPaths (adapter_demo, KS_DEMO_NAV with KS_DEMO_SHORTEN) against the model on the
    ESDF model of the layers the demo wrote."""
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import test_host_adapter_gpu as A
    from tests.util import NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    csv, fin, fout, fnav, fshort = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin", "nav.bin", "short.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    A._write_in(fin, A._frames())
    res = subprocess.run([A.DEMO, "fast", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True,
                         env=dict(os.environ, KS_DEMO_NAV=fnav, KS_DEMO_SHORTEN=fshort))
    assert res.returncode == 0 and "adapter_demo: shortenPaths" in res.stdout, res.stdout + res.stderr
    idx, t, s = A._read_out(fout)
    # the demo's options (adapter_demo.cpp): min_distance_m 0.1, max_distance_m 0.4; radius 0.2, at most 96 waypoints, lookahead 48
    esdf = esdf_model.esdf_from_blocks(idx, t, s["label"], 16, 0.05, min_distance_m=0.1, max_distance_m=0.4)
    store = E.Store(idx, esdf.blocks(idx), 16)
    buf = open(fnav, "rb").read()
    ng, ns, mw = struct.unpack_from("<III", buf, 0)
    off = 12 + 12 * ng + 12 * ns + ns + 4 * ns
    count = np.frombuffer(buf, "<u4", ns, off)
    flat = np.frombuffer(buf, "<f4", 3 * int(count.sum()), off + 4 * ns).reshape(-1, 3)
    longest = max(1, int(count.max()))                                           # the adapter's rows are as long as the longest path
    wp = np.full((ns, longest, 3), M.WAYPOINT_FILL, F)
    wp[np.arange(longest)[None, :] < count[:, None]] = flat
    want = M.shorten(store, wp, count, 0.05, radius_m=0.2, lookahead=48)
    buf = open(fshort, "rb").read()
    assert struct.unpack_from("<II", buf, 0) == (ns, 48)
    off = 8
    take = lambda dtype, k: np.frombuffer(buf, dtype, k, off)
    status = take(np.uint8, ns); off += ns
    kept = take("<u4", ns); off += 4 * ns
    length = take("<f4", ns); off += 4 * ns
    min_c = take("<f4", ns); off += 4 * ns
    assert len(buf) == off + 12 * int(kept.sum())
    got = dict(status=status, n_waypoints=kept, length=length, min_clearance=min_c)
    M.assert_same(got, want, "adapter")
    rows = np.arange(longest)[None, :] < kept[:, None]
    assert take("<f4", 3 * int(kept.sum())).tobytes() == want["waypoints"][rows].tobytes()
    assert want["stats"]["paths_ok"] > 50 and want["stats"]["paths_invalid"] > 50 and want["stats"]["waypoints_out"] < want["stats"]["waypoints_in"], want["stats"]
