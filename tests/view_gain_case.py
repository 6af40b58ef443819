"""The view-information-gain cases (ks_view_gain, ks_view_gain_device; DESIGN.md, section "View information gain"), shared by both
tiers like those of tests/frontier_case.py: the GPU tier (tests/test_view_gain_gpu.py) calls run_case in-process, the CPU tier
(tests/test_view_gain_cpu.py) runs it as a child process on the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.view_gain_case '<json spec>'
The checker is tests/view_gain_model.py on the stored ESDF as the library hands it out; every comparison is byte for byte.  The
fields are those of tests/frontier_case.py (see its header: a wall stores 0, a free voxel beside a wall exactly voxel_size).  The
two test-size switches (KS_DEBUG=1 KS_VG_LDS_BITS / KS_VG_GROUPS) are read when a context is made: `switches` sets them around that."""
import contextlib
import ctypes
import json
import os
import sys

import numpy as np

from tests import esdf_case, frontier_case, mesh_case, nav_case, objects_case
from tests import esdf_read_model as E
from tests import view_gain_model as M

VOXEL = mesh_case.VOXEL
F = np.float32
FREE, WALL = frontier_case.FREE, frontier_case.WALL
ECFG = frontier_case.ECFG
refused = objects_case.refused
centre = nav_case.centre
S = float(np.sqrt(0.5))
# T_G_C rotations (w, x, y, z) that turn the camera's +z into the world direction named
LOOK = {"+z": (1, 0, 0, 0), "-z": (0, 1, 0, 0), "+x": (S, 0, S, 0), "-x": (S, 0, -S, 0), "+y": (S, -S, 0, 0), "-y": (S, S, 0, 0)}
_g = np.array([0.83, 0.21, -0.43, 0.29])
GENERIC = tuple(float(v) for v in (_g / np.linalg.norm(_g)).astype(F))
_d = np.array([0.88, 0.12, 0.33, -0.31])
DIAGONAL = tuple(float(v) for v in (_d / np.linalg.norm(_d)).astype(F))


def B():
    from kimera_semantics_amd import binding
    return binding


def pose(q, t):
    return [float(v) for v in q] + [float(v) for v in t]


def K_of(w, h, fov_deg=60.0):
    f = 0.5 * w / np.tan(np.radians(fov_deg) / 2)
    return (f, f, (w - 1) / 2, (h - 1) / 2)


@contextlib.contextmanager
def switches(**kv):
    """KS_DEBUG=1 and the given switches in the environment while the body makes its contexts."""
    names = ["KS_DEBUG"] + list(kv)
    before = {k: os.environ.get(k) for k in names}
    os.environ["KS_DEBUG"] = "1"
    for k, v in kv.items():
        os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_stored = frontier_case._stored


def check(g, what, poses, K, w, h, lds_bits=M.LDS_BITS, groups=M.MAX_GROUPS, tiles=None, **cfg):
    """One call against the model and the sizing rule: (records, stats, model stats).  tiles: those of the ESDF store, where tiles
    have joined the map since it was made."""
    poses = np.asarray(poses, F).reshape(-1, 7)
    got = g.view_gain(poses, K, w, h, **cfg)
    want = M.model_of(g, poses, K, lds_bits=lds_bits, width=w, height=h, **cfg)
    M.assert_same(got, want, what)
    rec, stats = got
    rays = w * h
    ok = rec["flags"] == M.VALID
    assert (rec["rays_hit"][ok] + rec["rays_open"][ok] == rays).all() and (rec["flags"] <= 1).all(), what
    assert all((rec[k][~ok] == 0).all() for k in M.RECORD_DTYPE.names), what
    max_range = cfg.get("max_range_m", M.DEFAULTS["max_range_m"])
    want_ws = M.workspace_bytes(len(g.tile_keys()) if tiles is None else tiles, len(poses), max_range, VOXEL, groups, cfg.get("max_workspace_bytes", 1 << 30)) if len(poses) else 0
    assert stats["workspace_bytes"] == want_ws, (what, stats["workspace_bytes"], want_ws)
    return rec, stats, want[1]


def free_centre(vox, near=(0, 0, 0)):
    """The centre of the free voxel of `vox` nearest to `near` (by index distance, ties by order)."""
    v = min((p for p in vox if vox[p] == FREE), key=lambda p: (sum((a - b) ** 2 for a, b in zip(p, near)), p))
    return centre(*v)


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def case_images(spec):
    """Ray image sizes: 1 x 1, 5 x 3, 9 x 7 (63 rays), 13 x 5 (65) and 32 x 24, on the random field."""
    vox = frontier_case.random_voxels()
    g = _stored(vox, spec["vps"])
    at = free_centre(vox)
    poses = [pose(GENERIC, at), pose(LOOK["+x"], at), pose(DIAGONAL, free_centre(vox, (8, -7, 3)))]
    out = {}
    for w, h in ((1, 1), (5, 3), (9, 7), (13, 5), (32, 24)):
        rec, stats, _ = check(g, "image %d x %d" % (w, h), poses, K_of(w, h), w, h, max_range_m=1.0)
        assert stats["views_valid"] == 3 and stats["rays_hit"] + stats["rays_open"] == 3 * w * h
        out["%dx%d" % (w, h)] = [int(stats[k]) for k in ("unknown_voxels", "free_voxels", "surface_voxels", "samples")]
    assert stats["rays_hit"] > 0 and stats["free_voxels"] > 0 and stats["surface_voxels"] > 0, stats
    g.close()
    return out


def range_for(n, step):
    """A max_range_m (min_range_m = 0) that gives N = n samples at `step`, half a step clear of the next count."""
    return float(F((n - 0.5) * step))


def case_samples(spec):
    """Sample counts N = 1 (min_range == max_range), 64, 65 and 4096; 4097 is refused."""
    vox = frontier_case.room_voxels(True)
    g = _stored(vox, spec["vps"])
    at = centre(0, 0, 0)
    poses = [pose(LOOK["+x"], at), pose(GENERIC, at)]
    w, h = 5, 3
    K = K_of(w, h)
    rec, stats, _ = check(g, "N = 1", poses, K, w, h, min_range_m=0.3, max_range_m=0.3)
    assert M.n_samples(VOXEL, min_range_m=0.3, max_range_m=0.3) == 1 and stats["samples"] == 2 * w * h and stats["rays_open"] > 0
    for n, step in ((64, 0.01), (65, 0.01), (4096, 0.001)):
        cfg = dict(step_m=step, max_range_m=range_for(n, step))
        assert M.n_samples(VOXEL, **cfg) == n
        rec, stats, _ = check(g, "N = %d" % n, poses, K, w, h, **cfg)
        assert stats["samples"] > 2 * w * h
    cfg = dict(step_m=0.001, max_range_m=range_for(4097, 0.001))
    assert M.n_samples(VOXEL, **cfg) == 4097
    assert "4096 samples" in str(refused(B().KS_ERR_INVALID_ARG, lambda: g.view_gain(poses, K, w, h, **cfg)))
    g.close()
    return dict(stats)


def case_fields(spec):
    """Cube, room and random field: poses at the centre, on a tile seam, at the origin, inside a wall, outside every tile and at
    the end of the packed range."""
    vps = spec["vps"]
    w, h = 9, 7
    K = K_of(w, h)
    out = {}
    # the cube: everything seen from inside is free, then unknown
    g = _stored(frontier_case.cube_voxels(), vps)
    poses = [pose(LOOK[d], centre(0, 0, 0)) for d in sorted(LOOK)] + [pose(GENERIC, [0.0, 0.0, 0.0]), pose(DIAGONAL, [0.4, 0.4, 0.4])]
    rec, stats, _ = check(g, "cube", poses, K, w, h, max_range_m=1.0)
    assert stats["surface_voxels"] == 0 and stats["rays_hit"] == 0 and (rec["unknown_voxels"] > 0).all() and (rec["free_voxels"][:7] > 0).all()
    # ... outside every tile: unknown only; every ray runs its N samples
    rec, stats, _ = check(g, "outside every tile", [pose(GENERIC, [10.0, 10.0, 10.0])], K, w, h, max_range_m=1.0)
    assert rec["free_voxels"][0] == 0 and rec["unknown_voxels"][0] > 0 and rec["samples"][0] == w * h * M.n_samples(VOXEL, max_range_m=1.0)
    # ... at the end of the packed range the rays end OPEN where the next voxel index would be 2^20 - 1, and `samples` stops
    edge = ((1 << 20) - 6 + 0.5) * VOXEL
    rec, stats, _ = check(g, "end of the packed range", [pose(LOOK["+x"], [edge, 0.0, 0.0]), pose(LOOK["-x"], [-edge, 0.0, 0.0])], K_of(1, 1), 1, 1,
                          max_range_m=1.0)
    assert (rec["rays_open"] == 1).all() and (rec["samples"] < 8).all() and (rec["samples"] >= 3).all() and (rec["unknown_voxels"] == rec["samples"]).all(), rec
    out["edge_samples"] = rec["samples"].tolist()
    g.close()
    # the closed room from inside a wall: sample 0 is occupied
    g = _stored(frontier_case.room_voxels(False), vps)
    rec, stats, _ = check(g, "inside a wall", [pose(LOOK["-x"], centre(5, 0, 0)), pose(GENERIC, centre(-6, 2, 1))], K, w, h, max_range_m=1.0)
    assert (rec["surface_voxels"] == 1).all() and (rec["samples"] == w * h).all() and (rec["rays_hit"] == w * h).all()
    assert (rec["unknown_voxels"] == 0).all() and (rec["free_voxels"] == 0).all()
    rec, stats, _ = check(g, "room: centre, seam, origin", [pose(GENERIC, centre(0, 0, 0)), pose(DIAGONAL, [0.0, 0.0, 0.0]), pose(LOOK["+y"], [0.0, -0.2, 0.1])],
                          K, w, h, max_range_m=2.0)
    assert (rec["unknown_voxels"] == 0).all() and (rec["rays_hit"] == w * h).all()
    g.close()
    # the random field
    vox = frontier_case.random_voxels()
    g = _stored(vox, vps)
    poses = [pose(GENERIC, free_centre(vox)), pose(DIAGONAL, [0.0, 0.0, 0.0]), pose(LOOK["-y"], [0.4, 0.4, 0.0]), pose(LOOK["+z"], free_centre(vox, (-9, 5, 7)))]
    rec, stats, _ = check(g, "random", poses, K, w, h, max_range_m=2.0)
    assert stats["rays_hit"] > 0 and stats["unknown_voxels"] > 0
    out.update(stats)
    g.close()
    return out


def case_boundary(spec):
    """Rays along +z and -z (exact rotations) from the origin, step = voxel_size: the samples land on voxel boundaries."""
    g = _stored(frontier_case.cube_voxels(), spec["vps"])
    inv = E.inv_of(VOXEL)
    on_boundary = 0
    for k in range(1, 12):
        q = (F(k) * F(VOXEL)) * inv
        on_boundary += int(q == np.floor(q))
    assert on_boundary >= 6, on_boundary                                         # (p * voxel_size_inv is an integer)
    K = (500.0, 500.0, 0.0, 0.0)                                                 # the pixel (0, 0) looks along the optical axis exactly
    poses = [pose(LOOK["+z"], [0.0, 0.0, 0.0]), pose(LOOK["-z"], [0.0, 0.0, 0.0]), pose(LOOK["+z"], [0.1, -0.1, -0.25]), pose(LOOK["-z"], [-0.05, 0.2, 0.25])]
    dg = M.ray_directions(np.array(poses[1], F), K, 1, 1)
    assert dg.tolist() == [[0.0, 0.0, -1.0]]
    rec, stats, _ = check(g, "on voxel boundaries", poses, K, 1, 1, max_range_m=0.5)
    n = M.n_samples(VOXEL, max_range_m=0.5)
    assert n == 11 and (rec["samples"] == n).all() and (rec["rays_open"] == 1).all()
    # +z from z = 0: voxels 0 .. 4 are free (the cube ends at 4), then unknown; -z: sample 0 is voxel 0, then -1 .. -5 free, then unknown
    assert rec["free_voxels"].tolist()[:2] == [5, 6] and rec["unknown_voxels"].tolist()[:2] == [6, 5], rec
    g.close()
    return dict(stats)


def case_stop(spec):
    """stop_distance_m equal to a stored distance bit for bit, and one float below and above it."""
    g = _stored(frontier_case.room_voxels(False), spec["vps"])
    d, flags, _ = E.store_of(g).records(np.array([(4, 0, 0), (3, 0, 0)], np.int64))
    assert d[0].tobytes() == F(VOXEL).tobytes() and d[1] > d[0] and flags.all()
    K = (500.0, 500.0, 0.0, 0.0)
    poses = [pose(LOOK["+x"], centre(0, 0, 0))]
    below, equal, above = float(np.nextafter(F(VOXEL), F(0))), float(F(VOXEL)), float(np.nextafter(F(VOXEL), F(1)))
    seen = {}
    for name, stop in (("zero", 0.0), ("below", below), ("equal", equal), ("above", above)):
        rec, stats, _ = check(g, "stop_distance_m " + name, poses, K, 1, 1, max_range_m=1.0, stop_distance_m=stop)
        seen[name] = (int(rec["samples"][0]), int(rec["free_voxels"][0]), int(rec["surface_voxels"][0]))
    # voxels 0 .. 4 are free, 5 is the wall: the voxel beside it stops the ray once !(distance > stop_distance_m)
    assert seen == {"zero": (6, 5, 1), "below": (6, 5, 1), "equal": (5, 4, 1), "above": (5, 4, 1)}, seen
    g.close()
    return {k: list(v) for k, v in seen.items()}


def labelled_voxels():
    """The cube with a wall at x = 5: label 3 where y < 0, label 7 elsewhere."""
    vox = frontier_case.cube_voxels()
    for y in range(-5, 5):
        for z in range(-5, 5):
            vox[(5, y, z)] = (3 if y < 0 else 7, 1.0, 0.0)
    return vox


def case_labels(spec):
    g = _stored(labelled_voxels(), spec["vps"])
    w, h = 13, 5
    K = K_of(w, h, 90.0)
    poses = [pose(LOOK["+x"], centre(0, 0, 0)), pose(LOOK["+x"], centre(1, -3, 2)), pose(LOOK["-x"], centre(0, 0, 0))]
    seen = {}
    for label in (3, 7, 9, 255):
        rec, stats, _ = check(g, "label %d" % label, poses, K, w, h, max_range_m=1.0, label=label)
        seen[label] = rec["label_voxels"].tolist()
        surface = rec["surface_voxels"].tolist()
    assert seen[9] == [0, 0, 0] and seen[255] == [0, 0, 0] and surface[2] == 0 and surface[0] > 4, (seen, surface)
    assert [a + b for a, b in zip(seen[3], seen[7])] == surface and seen[3][0] > 0 and seen[7][0] > 0 and seen[3][1] > seen[7][1], (seen, surface)
    g.close()
    return {str(k): v for k, v in seen.items()}


def path_poses(vox):
    return [pose(GENERIC, free_centre(vox)), pose(DIAGONAL, [0.0, 0.0, 0.0]), pose(LOOK["-y"], [0.4, 0.4, 0.0]), pose(LOOK["+z"], free_centre(vox, (-9, 5, 7))),
            pose(LOOK["+x"], [10.0, 10.0, 10.0]), pose(GENERIC, [float("nan"), 0.0, 0.0])]


def case_paths(spec):
    """The same views through KS_VG_LDS_BITS = 0, the default, and a budget just below and just above one view's box: the same
    bytes, and views_in_lds and workspace_bytes by the documented rule.  Then one view whose box exceeds any LDS budget."""
    vps = spec["vps"]
    vox = frontier_case.random_voxels()
    w, h = 9, 7
    K = K_of(w, h)
    poses = path_poses(vox)
    g = _stored(vox, vps)
    rec0, stats0, model = check(g, "default budget", poses, K, w, h, max_range_m=1.0)
    g.close()
    box = model["box_bits"]
    assert box[5] == -1 and min(box[:5]) > 1000 and len(set(box[:5])) >= 3 and stats0["views_in_lds"] == 5, box
    middle = box[0]
    assert box.count(middle) == 1
    out = {"box_bits": box}
    for budget in (0, middle - 1, middle):
        with switches(KS_VG_LDS_BITS=budget):
            g = _stored(vox, vps)
        rec, stats, _ = check(g, "budget %d" % budget, poses, K, w, h, lds_bits=budget, max_range_m=1.0)
        assert rec.tobytes() == rec0.tobytes() and stats["views_in_lds"] == sum(1 for b in box if 1 <= b <= budget), (budget, stats)
        assert {k: v for k, v in stats.items() if k != "views_in_lds"} == {k: v for k, v in stats0.items() if k != "views_in_lds"}
        out[str(budget)] = stats["views_in_lds"]
        g.close()
    assert out["0"] == 0 and out[str(middle)] == out[str(middle - 1)] + 1 >= 2, out
    # a work space that holds two slabs: two workgroups in flight for six views
    g = _stored(vox, vps)
    two = M.workspace_bytes(len(g.tile_keys()), 2, 1.0, VOXEL)
    rec, stats, _ = check(g, "two slabs", poses, K, w, h, max_range_m=1.0, max_workspace_bytes=two + 5)
    assert rec.tobytes() == rec0.tobytes() and stats["workspace_bytes"] == two
    g.close()
    # 6.4 m at 5 cm, a wide image of 16 x 12 rays in an almost empty store: the box is beyond any LDS budget
    g = _stored({(x, y, 60): FREE for x in range(8) for y in range(8)}, vps)
    w, h = 16, 12
    big = [pose(DIAGONAL, [0.0, 0.0, 0.0]), pose(LOOK["+z"], [0.35, 0.35, 0.0])]
    rec, stats, model = check(g, "a box beyond the LDS", big, K_of(w, h, 100.0), w, h, max_range_m=6.4)
    assert min(model["box_bits"]) > M.LDS_BITS and stats["views_in_lds"] == 0 and stats["views_valid"] == 2, (model["box_bits"], stats)
    assert M.n_samples(VOXEL, max_range_m=6.4) == 129 and rec["free_voxels"][1] > 0 and rec["samples"][0] == w * h * 129
    out["big"] = model["box_bits"]
    g.close()
    return out


def case_reuse(spec):
    """One bitmap for every view (KS_VG_GROUPS = 1): five views that alternate a large box with a small one, the first repeated last;
    on the LDS path and through global memory.  Then one view more than there are workgroups."""
    vps = spec["vps"]
    vox = frontier_case.random_voxels()
    w, h = 9, 7
    K = K_of(w, h)
    first = pose(DIAGONAL, free_centre(vox))
    end = ((1 << 20) - 3.5) * VOXEL                                              # (a view that the end of the packed range cuts short)
    poses = [first, pose(LOOK["-y"], [0.0, -end, 0.0]), pose(GENERIC, [0.0, 0.0, 0.0]), pose(LOOK["+x"], [end, 0.0, 0.0]), first]
    out = {}
    for budget in (M.LDS_BITS, 0):
        with switches(KS_VG_GROUPS=1, KS_VG_LDS_BITS=budget):
            g = _stored(vox, vps)
        rec, stats, model = check(g, "one workgroup, budget %d" % budget, poses, K, w, h, lds_bits=budget, groups=1, max_range_m=1.5)
        box = model["box_bits"]
        assert box[0] > 2 * box[1] and box[2] > 2 * box[3] and box[1] > 0 and box[3] > 0 and rec[0] == rec[4], box
        assert stats["workspace_bytes"] == M.workspace_bytes(len(g.tile_keys()), 1, 1.5, VOXEL)
        out[str(budget)] = box
        g.close()
    with switches(KS_VG_GROUPS=4):
        g = _stored(vox, vps)
    rec, stats, _ = check(g, "five views, four workgroups", poses, K, w, h, groups=4, max_range_m=1.5)
    assert rec[0] == rec[4]
    rec3, _, _ = check(g, "three views, four workgroups", poses[:3], K, w, h, groups=4, max_range_m=1.5)
    assert rec3.tobytes() == rec[:3].tobytes()
    g.close()
    return out


def case_invalid(spec):
    """n = 0; views that are data, not errors: a NaN, an infinity, a quaternion far from unit length."""
    vox = frontier_case.random_voxels()
    g = _stored(vox, spec["vps"])
    w, h = 5, 3
    K = K_of(w, h)
    rec, stats = g.view_gain(np.zeros((0, 7), F), K, w, h)
    assert rec.shape == (0,) and all(v == 0 for v in stats.values()), stats
    KS = B()
    cfg, st = g.view_gain_config(K, w, h), KS.KsViewGainStats(samples=7)
    assert KS.lib().ks_view_gain(g._h, None, 0, ctypes.byref(cfg), None, ctypes.byref(st)) == 0 and st.samples == 0
    assert KS.lib().ks_view_gain_device(g._h, None, 0, ctypes.byref(cfg), None, None) == 0
    at = free_centre(vox)
    good = [pose(GENERIC, at), pose(LOOK["-x"], at), pose(DIAGONAL, [0.0, 0.0, 0.0])]
    alone, _, _ = check(g, "valid views alone", good, K, w, h, max_range_m=1.0)
    long_q = [30.0 * v for v in GENERIC]
    mixed = [good[0], pose(GENERIC, [0.0, float("nan"), 0.0]), good[1], pose((float("inf"), 0, 0, 0), at), pose(long_q, at), good[2],
             pose(GENERIC, [0.0, 0.0, float("-inf")])]
    rec, stats, model = check(g, "invalid views between valid ones", mixed, K, w, h, max_range_m=1.0)
    assert stats["views_invalid"] == 4 and stats["views_valid"] == 3 and rec[[0, 2, 5]].tobytes() == alone.tobytes()
    assert rec[[1, 3, 4, 6]].tobytes() == bytes(4 * 32) and model["box_bits"][4] == -1
    g.close()
    return dict(stats)


def case_determinism(spec):
    """The same voxels uploaded in another block order (other slots) give the same bytes; so do two calls."""
    vox = frontier_case.random_voxels()
    a, b = _stored(vox, spec["vps"]), _stored(vox, spec["vps"], reverse=True)
    ka, kb = a.tile_keys(), b.tile_keys()
    assert sorted(ka) == sorted(kb) and (ka != kb).any()
    w, h = 13, 5
    K = K_of(w, h)
    poses = path_poses(vox)
    ra, sa, _ = check(a, "forward order", poses, K, w, h, max_range_m=1.5, label=0)
    rb, sb, _ = check(b, "reversed order", poses, K, w, h, max_range_m=1.5, label=0)
    again = a.view_gain(np.array(poses, F), K, w, h, max_range_m=1.5, label=0)
    assert ra.tobytes() == rb.tobytes() == again[0].tobytes() and sa == sb == again[1]
    a.close()
    b.close()
    return dict(sa)


def _frame_totals(st):
    return (st.n_rays_cast, st.n_voxel_updates)


def case_in_flight(spec):
    """Four integrated frames with pipeline_frames = 12: the call completes them, their statistics stay owed until the next flush."""
    vox = frontier_case.cube_voxels()
    frames = mesh_case._frames(4, 64, 48)
    w, h = 9, 7
    K = K_of(w, h)
    poses = [pose(GENERIC, centre(0, 0, 0)), pose(LOOK["+x"], [0.0, 0.0, 0.0])]
    a, b = (_stored(vox, 16, pipeline=12) for _ in range(2))
    tiles = len(a.tile_keys())
    for g in (a, b):
        for f in frames:
            assert _frame_totals(g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)) == (0, 0)     # (in flight)
    rec, stats, _ = check(a, "frames in flight", poses, K, w, h, tiles=tiles, max_range_m=1.0)   # (the store is the snapshot it was)
    assert stats["free_voxels"] > 0
    owed_a, owed_b = _frame_totals(a.flush()), _frame_totals(b.flush())
    assert owed_a == owed_b and owed_a[1] > 0, (owed_a, owed_b)
    a.close()
    b.close()
    return dict(stats)


def case_reads_only(spec):
    """Every flag and stored product is byte-equal before and after, and what follows (a refresh, a mesh of the stale blocks) does
    what it does without the calls."""
    vps = spec["vps"]
    goals = np.array([[-0.7, -0.7, -0.7], [0.7, 0.7, 0.7]], F)
    w, h = 9, 7
    K = K_of(w, h)
    poses = np.array([pose(GENERIC, [0.0, 0.0, 0.0]), pose(LOOK["+x"], [-0.3, 0.1, 0.2]), pose(DIAGONAL, [0.7, 0.7, 0.7])], F)

    def prepared():
        g = nav_case._stored("sphere", vps)
        g.mesh()
        g.objects()
        g.mesh_index()
        g.nav_update(goals, radius_m=0.1)
        g.frontiers(radius_m=0.1)
        g.updated_block_indices(reset=True)
        g.upload(*esdf_case.random_field([(0, 0, 0)], vps, 91))       # written voxels: `updated`, `dirty`, both stale bits
        f = mesh_case._frames(1, 64, 48)[0]
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        return g

    def snapshot(g):
        idx, t, s = g.download()
        n, nr = ctypes.c_size_t(), ctypes.c_size_t()
        assert B().lib().ks_count_updated_voxels(g._h, ctypes.byref(n), ctypes.byref(nr)) == 0
        im = g.mesh_index(build=False)                                 # the stored index and the directory of the stored mesh
        return dict(updated=g.updated_block_indices(reset=False).tobytes(), counted=(n.value, nr.value), idx=idx.tobytes(), tsdf=t.tobytes(),
                    sem=s.tobytes(), esdf=g.esdf_blocks(idx).tobytes(), objects=g.object_records().tobytes(), ids=g.object_ids(idx).tobytes(),
                    nav=g.nav_blocks(idx).tobytes(), frontiers=g.frontier_records().tobytes(), frontier_ids=g.frontier_ids(idx).tobytes(),
                    mesh=im.blocks.tobytes(), index=(im.xyz.tobytes(), im.indices.tobytes(), im.object_ids.tobytes()))

    def calls(g):
        rec, stats = g.view_gain(poses, K, w, h, max_range_m=1.5, label=3)
        assert stats["views_valid"] == 3 and stats["unknown_voxels"] > 0 and stats["surface_voxels"] > 0, stats
        g.view_gain(poses[:1], K, 1, 1)

    def followers(g):
        return dict(stale=g.esdf_refresh()["tiles_stale"], meshed=g.mesh(only_stale=True).stats["blocks_meshed"])

    g = prepared()
    before = snapshot(g)
    assert len(before["updated"]) > 0 and before["counted"][0] > 0
    calls(g)
    after = snapshot(g)
    assert after == before, [k for k in before if before[k] != after[k]]
    with_calls = followers(g)
    g.close()
    g = prepared()                                                    # the same history without the calls
    without = followers(g)
    g.close()
    assert with_calls == without and with_calls["stale"] > 0 and with_calls["meshed"] > 0, (with_calls, without)
    return with_calls


def case_errors(spec):
    KS = B()
    L = KS.lib()
    g = mesh_case._integrator(0, 64, 48, vps=8)
    g.upload(*objects_case.voxel_field(frontier_case.cube_voxels(), 8))
    w, h = 5, 3
    K = K_of(w, h)
    poses = np.array([pose(GENERIC, [0.0, 0.0, 0.0])], F)
    out = np.zeros(1, KS.VIEW_GAIN_DTYPE)
    P = lambda a: a.ctypes.data
    assert ctypes.sizeof(KS.KsViewGainConfig) == 56 and ctypes.sizeof(KS.KsViewGainStats) == 88 and KS.VIEW_GAIN_DTYPE.itemsize == 32
    calls = [lambda **kw: g.view_gain(poses, kw.pop("K", K), kw.pop("width", w), kw.pop("height", h), **kw),
             lambda **kw: g.view_gain_device(8, 1, kw.pop("K", K), kw.pop("width", w), kw.pop("height", h), d_out=8, **kw)]   # (the addresses are never used)
    # no stored ESDF
    for call in calls:
        assert "no ESDF is stored" in str(refused(KS.KS_ERR_INVALID_ARG, call))
    g.esdf_update(**ECFG)
    # NULL ctx or cfg; NULL poses or output with n > 0
    cfg, st = g.view_gain_config(K, w, h), KS.KsViewGainStats()
    assert L.ks_view_gain_default_config(None) == KS.KS_ERR_INVALID_ARG
    for fn in (L.ks_view_gain, L.ks_view_gain_device):
        assert fn(None, P(poses), 1, ctypes.byref(cfg), P(out), ctypes.byref(st)) == KS.KS_ERR_INVALID_ARG
        assert fn(g._h, P(poses), 1, None, P(out), ctypes.byref(st)) == KS.KS_ERR_INVALID_ARG
        assert fn(g._h, None, 1, ctypes.byref(cfg), P(out), ctypes.byref(st)) == KS.KS_ERR_INVALID_ARG
        assert fn(g._h, P(poses), 1, ctypes.byref(cfg), None, ctypes.byref(st)) == KS.KS_ERR_INVALID_ARG
        assert fn(g._h, P(poses), 1 << 24, ctypes.byref(cfg), P(out), ctypes.byref(st)) == KS.KS_ERR_INVALID_ARG
    # the configuration
    for call in calls:
        for bad in (dict(width=0), dict(height=0), dict(width=1025), dict(height=1025), dict(width=1024, height=65), dict(K=(float("nan"), 1.0, 0.0, 0.0)),
                    dict(K=(1.0, 1.0, float("inf"), 0.0)), dict(K=(0.0, 1.0, 0.0, 0.0)), dict(K=(1.0, -1.0, 0.0, 0.0)), dict(min_range_m=2.0, max_range_m=1.0),
                    dict(label=256)):
            refused(KS.KS_ERR_INVALID_ARG, lambda: call(**bad))
        for name in ("min_range_m", "max_range_m", "step_m", "stop_distance_m"):
            for bad in (-0.1, float("nan"), float("inf"), float("-inf")):
                refused(KS.KS_ERR_INVALID_ARG, lambda: call(**{name: bad}))
        refused(KS.KS_ERR_INVALID_ARG, lambda: call(max_range_m=4097 * VOXEL))          # N = 4097 or more
    # the limits themselves are allowed: 1024 x 64 rays is 65536; the work space of one view as the bound
    rec, stats = g.view_gain(poses, K_of(1024, 64), 1024, 64, max_range_m=0.1)
    assert stats["rays_hit"] + stats["rays_open"] == 65536
    one = M.workspace_bytes(len(g.tile_keys()), 1, 5.0, VOXEL)
    assert one == 8 * 256 + 96 + ((203 ** 3 + 31) // 32 + 63) // 64 * 256
    rec, stats, _ = check(g, "just enough work space", poses, K, w, h, max_workspace_bytes=one)
    # ... and one byte less is refused, with the stats saying what one view needs and nothing else
    for fn, po, pr in ((L.ks_view_gain, P(poses), P(out)), (L.ks_view_gain_device, 8, 8)):
        cfg, st = g.view_gain_config(K, w, h, max_workspace_bytes=one - 1), KS.KsViewGainStats(samples=7, views_valid=7)
        out[:] = 0
        assert fn(g._h, po, 1, ctypes.byref(cfg), pr, ctypes.byref(st)) == KS.KS_ERR_UNSUPPORTED
        assert st.workspace_bytes == one and all(getattr(st, k) == 0 for k, _ in KS.KsViewGainStats._fields_ if k != "workspace_bytes")
        assert out.tobytes() == bytes(32)
        assert fn(g._h, po, 1, ctypes.byref(cfg), pr, None) == KS.KS_ERR_UNSUPPORTED    # stats may be NULL
    # stats may be NULL on a call that runs; the default configuration
    cfg = g.view_gain_config(K, w, h)
    assert L.ks_view_gain(g._h, P(poses), 1, ctypes.byref(cfg), P(out), None) == 0 and out.tobytes() == rec.tobytes()
    d = KS.KsViewGainConfig(min_range_m=7, label=7, pad=7)
    assert L.ks_view_gain_default_config(ctypes.byref(d)) == 0
    assert (d.min_range_m, d.max_range_m, d.step_m, d.stop_distance_m, d.width, d.height, d.label, d.pad, d.max_workspace_bytes) == (0, 5, 0, 0, 32, 24, 255, 0, 1 << 30)
    assert list(d.K) == [0, 0, 0, 0]
    refused(KS.KS_ERR_INVALID_ARG, lambda: g.view_gain(poses, (0, 0, 0, 0)))       # K has no default: the caller must set it
    g.close()
    # an empty map with a stored ESDF is no error: everything is unknown
    e = mesh_case._integrator(0, 64, 48, vps=8)
    e.esdf_update(**ECFG)
    rec, stats, _ = check(e, "empty map", poses, K, w, h, max_range_m=1.0)
    assert rec["unknown_voxels"][0] > 0 and rec["free_voxels"][0] == 0 and stats["workspace_bytes"] == M.workspace_bytes(0, 1, 1.0, VOXEL)
    e.close()
    # a marcher context of the exact multi-GPU mode holds no voxel data
    marcher, owner = (mesh_case._integrator(1, 64, 48) for _ in range(2))
    f = mesh_case._frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    for call in (lambda: marcher.view_gain(poses, K, w, h), lambda: marcher.view_gain_device(8, 1, K, w, h, d_out=8)):
        refused(KS.KS_ERR_UNSUPPORTED, call)
    owner.esdf_update(**ECFG)
    assert owner.view_gain(poses, K, w, h)[1]["views_valid"] == 1                  # (the owner holds the map)
    marcher.close()
    owner.close()
    # a context in a failed state (the pool is full: sticky until a clear)
    small = mesh_case._integrator(0, 64, 48, max_tiles=8)
    try:
        small.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        raise AssertionError("a frame fitted 8 tiles")
    except KS.KsError as err:
        assert err.code == KS.KS_ERR_POOL_FULL, err
    for call in (lambda: small.view_gain(poses, K, w, h), lambda: small.view_gain_device(8, 1, K, w, h, d_out=8)):
        assert "failed state" in str(refused(KS.KS_ERR_INVALID_ARG, call))
    small.close()
    return {}


CASES = {"images": case_images, "samples": case_samples, "fields": case_fields, "boundary": case_boundary, "stop": case_stop, "labels": case_labels,
         "paths": case_paths, "reuse": case_reuse, "invalid": case_invalid, "determinism": case_determinism, "in_flight": case_in_flight,
         "reads_only": case_reads_only, "errors": case_errors}

# name -> spec: the same cases in both tiers
SPECS = {}
for _vps in (8, 16):
    for _case in ("images", "samples", "fields", "boundary", "stop", "labels", "paths", "reuse", "invalid", "determinism", "reads_only"):
        SPECS["%s_vps%d" % (_case, _vps)] = dict(case=_case, vps=_vps)
SPECS.update({"in_flight": dict(case="in_flight"), "errors": dict(case="errors")})


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("VIEW_GAIN_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
