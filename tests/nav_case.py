"""The navigation-field cases (ks_nav_update, ks_nav_query, ks_nav_download_blocks, ks_nav_paths; DESIGN.md, section "Navigation
field"), shared by both tiers like those of tests/esdf_read_case.py: the GPU tier (tests/test_nav_gpu.py) calls run_case in-process,
the CPU tier (tests/test_nav_cpu.py) runs it as a child process on the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.nav_case '<json spec>'
The checker is tests/nav_model.py on the stored ESDF as the library hands it out; every comparison is byte for byte, the five
contractual statistics included.  Traversability is shaped by uploads: a FREE voxel is observed with a TSDF distance of 0.3 m (no site
anywhere, so its ESDF distance is max_distance_m = 0.4 m), a wall voxel has weight 0 (unobserved); then ks_esdf_update."""
import ctypes
import json
import os
import sys

import numpy as np

from tests import esdf_case, mesh_case, objects_case
from tests import esdf_read_model as E
from tests import nav_model as M

VOXEL = mesh_case.VOXEL
F = np.float32
FREE = (0, 1.0, 0.3)             # (label, weight, TSDF distance) of objects_case.voxel_field
ECFG = esdf_case.cfg_of({})      # min_distance_m 0.1, max_distance_m 0.4
RADIUS = 0.3
RANDOM_SEED, RANDOM_P = 3, 0.12  # chosen on the CPU with the model: tests/test_nav_cpu.py asserts what they are chosen for
refused = objects_case.refused


def centre(*ijk):
    return [(v + 0.5) * VOXEL for v in ijk]


# ---- fields: voxel sets -------------------------------------------------------------------------------------------------------
def open_box_voxels():
    """3 x 3 x 3 tiles straddling the origin, every voxel free."""
    r = range(-8, 16)
    return [(x, y, z) for x in r for y in r for z in r]


OPEN_BOX_GOAL = (2, 5, 3)        # off-centre in the middle tile

# (goal voxel, its only neighbour, the cost of that neighbour): pairs that touch only across a tile corner, two kinds of tile edge
# and a tile face; 32 voxels apart, so no pair sees another
SEAM_PAIRS = (((7, 7, 7), (8, 8, 8), 17), ((39, 7, 2), (40, 8, 2), 14), ((72, 7, 4), (71, 8, 4), 14), ((103, 3, 3), (104, 3, 3), 10))


def seams_voxels():
    return [p for a, b, _ in SEAM_PAIRS for p in (a, b)]


def _rows(x0, x1, ys, z, leftwards):
    """Rows along x at the given ys of layer z, linked at alternating ends; returns (voxels in walking order, the next direction)."""
    out = []
    for k, y in enumerate(ys):
        xs = list(range(x0, x1 + 1))
        if leftwards:
            xs.reverse()
        out += [(x, y, z) for x in xs]
        if k + 1 < len(ys):
            out.append((xs[-1], (y + ys[k + 1]) // 2, z))
        leftwards = not leftwards
    return out, leftwards


def serpentine_path():
    """A one-voxel corridor in walking order: it winds through the tile (0, 0, 0) in four layers of four rows, zigzags eight times
    between the tiles (1, 0, 0) and (2, 0, 0), and leaves along -y through thirteen more tiles."""
    path, left = [], True
    for k, z in enumerate((0, 2, 4, 6)):                       # the winding: starts at (7, 0, 0), ends at (7, 0, 6)
        ys = (0, 2, 4, 6) if k % 2 == 0 else (6, 4, 2, 0)
        rows, left = _rows(0, 7, ys, z, left)
        path += rows
        if z < 6:
            path.append((path[-1][0], path[-1][1], z + 1))
    path += [(8, 0, 6), (9, 0, 6)]
    left = False
    for k, z in enumerate((6, 4)):                             # the zigzag: x = 10..23, ends at (10, 0, 4)
        ys = (0, 2, 4, 6) if k == 0 else (6, 4, 2, 0)
        rows, left = _rows(10, 23, ys, z, left)
        path += rows
        if z == 6:
            path.append((path[-1][0], path[-1][1], 5))
    path += [(10, 0, z) for z in (3, 2, 1, 0)]
    path += [(10, y, 0) for y in range(-1, -101, -1)]          # the way out, through negative indices
    assert len(set(path)) == len(path)
    return path


def random_voxels(seed=RANDOM_SEED, p=RANDOM_P):
    """4 x 4 x 4 tiles from (-16, -16, -16): a share p of the voxels free."""
    rng = np.random.default_rng(seed)
    free = rng.random((32, 32, 32)) < p
    return [tuple(int(c) - 16 for c in v) for v in np.argwhere(free)]


def random_goals(vox):
    """Goals of the random case: eight free voxels, one of them twice, and one each in a wall, in a tile that is not resident, with a
    non-finite coordinate and outside the packed range."""
    rng = np.random.default_rng(RANDOM_SEED + 1)
    pick = [vox[i] for i in rng.choice(len(vox), 8, replace=False)]
    free = set(vox)
    wall = next(v for v in ((x, 0, 0) for x in range(-16, 16)) if v not in free)
    goals = [centre(*v) for v in pick] + [centre(*pick[2]), centre(*wall), centre(40, 40, 40), [np.nan, 0.0, 0.0], [0.0, -np.inf, 0.0], [6e4, 0.0, 0.0]]
    return np.array(goals, F)


RANDOM_GOALS_BLOCKED = 5


def field_blocks(vox, vps, resident=()):
    return objects_case.voxel_field({v: FREE for v in vox}, vps, resident=resident)


def make_voxels(kind):
    return {"open_box": open_box_voxels, "seams": seams_voxels, "serpentine": serpentine_path, "random": random_voxels}[kind]()


def _stored(kind, vps, reverse=False, **extra):
    g = mesh_case._integrator(0, 64, 48, vps=vps, **extra)
    if kind == "sphere":
        idx, t, s = mesh_case.make_field("sphere", vps)
    else:
        idx, t, s = field_blocks(make_voxels(kind), vps)
    if reverse:
        idx, t, s = idx[::-1].copy(), t[::-1].copy(), s[::-1].copy()
    g.upload(idx, t, s)
    g.esdf_update(**ECFG)
    return g


def check(g, goals, what, **cfg):
    """One update against the model: (stats, block indices, field blocks, model)."""
    stats = g.nav_update(goals, **cfg)
    model = M.model_of(g, goals, **{k: v for k, v in cfg.items() if k in ("radius_m", "max_cost") and v is not None})
    idx, blocks = M.assert_field(g, stats, model, what)
    nt = len(g.tile_keys())
    assert stats["workspace_bytes"] == nt * 512 * 4 + nt * 12 + len(np.asarray(goals).reshape(-1, 3)) * 12, (what, stats)
    return stats, idx, blocks, model


def cost_at(g, *ijk):
    return int(g.nav_query(np.array([centre(*ijk)], F))[0])


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def case_open_box(spec):
    g = _stored("open_box", spec["vps"])
    goal = np.array([centre(*OPEN_BOX_GOAL)], F)
    stats, idx, blocks, model = check(g, goal, "open box", radius_m=RADIUS)
    vox = np.array(open_box_voxels(), np.int64)
    d = np.sort(np.abs(vox - np.array(OPEN_BOX_GOAL)), axis=1)
    closed = (10 * d[:, 2] + 4 * d[:, 1] + 3 * d[:, 0]).astype(np.uint32)
    xyz = ((vox + 0.5) * VOXEL).astype(F)
    got = g.nav_query(xyz)
    assert (got == closed).all(), np.argwhere(got != closed)[:5]
    assert (got == model.query(xyz)).all()
    assert stats["voxels_traversable"] == stats["voxels_reached"] == 24 ** 3 and stats["largest_cost"] == int(closed.max())
    assert stats["goals_used"] == 1 and stats["goals_blocked"] == 0 and stats["rounds"] >= 2 and stats["tile_relaxations"] >= 27
    g.close()
    return dict(stats)


def case_seams(spec):
    g = _stored("seams", spec["vps"])
    goals = np.array([centre(*a) for a, _, _ in SEAM_PAIRS], F)
    stats, idx, blocks, model = check(g, goals, "seams", radius_m=RADIUS)
    for a, b, cost in SEAM_PAIRS:
        assert cost_at(g, *a) == 0 and cost_at(g, *b) == cost, (a, b, cost_at(g, *b))
    assert stats["voxels_traversable"] == stats["voxels_reached"] == 8 and stats["largest_cost"] == 17 and stats["goals_used"] == 4
    if spec["vps"] == 8:   # the tiles between the two of a pair are not resident
        keys = len(g.tile_keys())
        assert keys == 8, keys
    g.close()
    return dict(stats)


def case_serpentine(spec):
    g = _stored("serpentine", spec["vps"])
    path = serpentine_path()
    near, far = np.array([centre(*path[0])], F), np.array([centre(*path[-1])], F)
    stats, idx, blocks, model = check(g, near, "serpentine, one goal", radius_m=RADIUS)
    assert stats["voxels_reached"] == stats["voxels_traversable"] == len(path) and stats["largest_cost"] == model.stats["largest_cost"] > 3000
    assert cost_at(g, *path[-1]) == stats["largest_cost"]
    # (from 32 voxels per side on most resident tiles hold no voxel of the path: the floor counts the tiles the path visits)
    n_tiles = len(g.tile_keys()) if spec["vps"] <= 16 else len({tuple(c >> 3 for c in v) for v in path})
    assert stats["rounds"] >= 16 and stats["tile_relaxations"] > n_tiles / 2, stats
    walk = g.nav_paths(far, 1024)
    M.assert_paths(walk, M.paths(model, far, 1024), "the walk back")
    assert walk["status"][0] == M.REACHED and walk["cost"][0] == stats["largest_cost"]
    both = np.concatenate([near, far])
    stats2, _, _, model2 = check(g, both, "serpentine, a goal at either end", radius_m=RADIUS)
    assert stats2["goals_used"] == 2 and stats["largest_cost"] // 2 - 20 <= stats2["largest_cost"] <= stats["largest_cost"] // 2 + 20, stats2
    # a relaxation that has not converged stores nothing: a returned error code
    e = refused_code(g, lambda: g.nav_update(near, radius_m=RADIUS, max_rounds=1))
    assert e == B().KS_ERR_UNSUPPORTED
    refused(B().KS_ERR_INVALID_ARG, lambda: g.nav_query(near))
    g.close()
    return dict(stats)


def B():
    from kimera_semantics_amd import binding
    return binding


def refused_code(g, call):
    try:
        call()
    except B().KsError as e:
        return e.code
    raise AssertionError("accepted")


def case_random(spec):
    vps = spec["vps"]
    vox = random_voxels()
    goals = random_goals(vox)
    a = _stored("random", vps)
    stats, idx, blocks, model = check(a, goals, "random", radius_m=RADIUS)
    assert stats["goals_blocked"] == RANDOM_GOALS_BLOCKED and stats["goals_used"] == len(goals) - RANDOM_GOALS_BLOCKED
    assert 0 < stats["voxels_reached"] < stats["voxels_traversable"] == len(vox)
    assert (blocks == M.UNREACHED).any() and (blocks == M.BLOCKED).any() and (blocks == 0).sum() == 8
    # the same goals in another order, the same voxels uploaded in another block order: the same bytes
    stats_p, _, blocks_p, _ = check(a, goals[::-1].copy(), "goals reversed", radius_m=RADIUS)
    assert blocks_p.tobytes() == blocks.tobytes() and {k: stats_p[k] for k in M.STAT_KEYS} == {k: stats[k] for k in M.STAT_KEYS}
    b = _stored("random", vps, reverse=True)
    ka, kb = a.tile_keys(), b.tile_keys()
    assert sorted(ka) == sorted(kb) and (ka != kb).any()
    b.nav_update(goals, radius_m=RADIUS)
    assert b.nav_blocks(idx).tobytes() == blocks.tobytes()
    # points: inside, outside the map, outside the packed range, not finite
    rng = np.random.default_rng(5)
    ijk = rng.integers(-22, 22, (2000, 3))
    xyz = np.concatenate([((ijk + 0.5 + rng.uniform(-0.4, 0.4, ijk.shape)) * VOXEL), [[6e4, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]]]).astype(F)
    got = a.nav_query(xyz)
    assert got.dtype == np.uint32 and (got == model.query(xyz)).all() and (got[-3:] == M.BLOCKED).all()
    absent = np.array([[9, 9, 9], [-9, 0, 0]], np.int32)
    assert (a.nav_blocks(absent) == M.BLOCKED).all()
    a.close()
    b.close()
    return dict(stats)


def case_radius(spec):
    g = _stored("sphere", spec["vps"])
    idx = g.block_indices()
    rec = g.esdf_blocks(idx)
    c = np.array(mesh_case.SPHERE_CENTRE)
    goal = np.array([[-0.7, -0.7, -0.7]], F)
    # a stored distance between the band and the clamp, outside the sphere
    ok = (rec["flags"] & 1 != 0) & (rec["distance"] > 0.12) & (rec["distance"] < 0.38)
    j, l = np.argwhere(ok)[len(np.argwhere(ok)) // 2]
    d0 = rec["distance"][j, l]
    vps = spec["vps"]
    v = idx[j].astype(np.int64) * vps + np.array([l % vps, (l // vps) % vps, l // (vps * vps)])
    out = {}
    for name, radius in (("equal", float(d0)), ("next_above", float(np.nextafter(d0, F(1)))), ("zero", 0.0)):
        assert F(radius) == (d0 if name == "equal" else F(radius))
        stats, _, blocks, model = check(g, goal, "radius " + name, radius_m=radius)
        out[name] = stats
        got = cost_at(g, *v)
        assert (got == M.BLOCKED) == (name == "next_above"), (name, got)
        inside = np.array([c + [0.0, 0.0, 0.0], c + [0.2, -0.1, 0.1]], F)
        assert (g.nav_query(inside) == M.BLOCKED).all()                        # negative distances: the sphere's inside
        assert stats["voxels_reached"] > 1000 and stats["goals_used"] == 1, stats
    assert out["zero"]["voxels_traversable"] > out["equal"]["voxels_traversable"] > out["next_above"]["voxels_traversable"]
    g.close()
    return out["equal"]


def case_max_cost(spec):
    g = _stored("open_box", spec["vps"])
    goal = np.array([centre(*OPEN_BOX_GOAL)], F)
    full, idx, blocks, _ = check(g, goal, "uncapped", radius_m=RADIUS)
    present = np.unique(blocks[blocks <= M.MAX_COST])
    cap = int(present[len(present) // 2])                                       # exactly a present cost: it stays
    gaps = np.setdiff1d(np.arange(int(present.max())), present)
    between = int(gaps[len(gaps) // 2])                                         # a cap no voxel has as its cost
    assert 17 < between < present.max()
    for c in (cap, between, 9, 10, 1):
        stats, _, capped, _ = check(g, goal, "cap %d" % c, radius_m=RADIUS, max_cost=c)
        want = np.where(blocks <= c, blocks, np.where(blocks == M.BLOCKED, M.BLOCKED, M.UNREACHED)).astype(np.uint32)
        assert capped.tobytes() == want.tobytes() and stats["largest_cost"] == int(present[present <= c].max()), (c, stats)
    stats, _, capped, _ = check(g, goal, "the largest cap", radius_m=RADIUS, max_cost=M.MAX_COST)
    assert capped.tobytes() == blocks.tobytes()
    g.close()
    return dict(full)


def path_starts():
    """Starts over the random field and around it: reached, unreachable and blocked ones, outside the map, not finite."""
    rng = np.random.default_rng(11)
    vox = random_voxels()
    free = np.array(vox, np.int64)[rng.choice(len(vox), 500, replace=False)]
    anywhere = rng.integers(-20, 20, (200, 3))
    xyz = np.concatenate([(free + 0.5 + rng.uniform(-0.4, 0.4, free.shape)) * VOXEL, (anywhere + 0.5) * VOXEL,
                          [[np.nan, 0, 0], [0, 0, np.inf], [6e4, 6e4, 0]]])
    return xyz.astype(F)


def case_paths(spec):
    """With `chunk` in the spec the case runs under KS_DEBUG=1 KS_NAV_CHUNK=<chunk>: the same bytes as the model, which knows no chunks."""
    chunk = spec.get("chunk")
    if chunk:
        assert os.environ.get("KS_DEBUG") == "1" and int(os.environ.get("KS_NAV_CHUNK", "0")) == chunk
    vox = random_voxels()
    goals = random_goals(vox)
    g = _stored("random", spec["vps"])
    stats, idx, blocks, model = check(g, goals, "random", radius_m=RADIUS)
    starts = path_starts()
    assert len(starts) % 64 != 0 and (not chunk or (len(starts) - 1) // chunk >= 2)
    out = {}
    for mw in (1, 7, 64, 600):
        got = g.nav_paths(starts, mw)
        want = M.paths(model, starts, mw)
        M.assert_paths(got, want, "max_waypoints %d" % mw)
        out[mw] = want["stats"]
        # rows from n_waypoints on keep the pattern they were given
        rows = np.arange(mw)[None, :] >= got["n_waypoints"][:, None]
        assert (got["waypoints"][rows] == g.NAV_WAYPOINT_FILL).all() and (got["waypoints"][~rows] != g.NAV_WAYPOINT_FILL).all()
        assert (got["n_waypoints"][np.isin(got["status"], (M.UNREACHABLE, M.PATH_BLOCKED))] == 0).all()
        assert (got["n_waypoints"][got["status"] == M.TRUNCATED] == mw).all()
    small = out[7]
    assert all(small[k] > 0 for k in ("paths_reached", "paths_unreachable", "paths_blocked", "paths_truncated")), small
    assert out[1]["paths_truncated"] > 0 and out[1]["paths_reached"] >= 0 and out[600]["paths_truncated"] == 0 and out[600]["paths_reached"] > small["paths_reached"]
    full = g.nav_paths(starts, 64)
    assert (full["status"] != M.INVALID).all() and (full["cost"] == g.nav_query(starts)).all()
    # a reached path ends in the centre of a goal voxel, and its steps sum to the cost
    r = np.nonzero(full["status"] == M.REACHED)[0]
    ends = full["waypoints"][r, full["n_waypoints"][r] - 1]
    assert (g.nav_query(ends) == 0).all()
    # every output but one NULL, with and without statistics
    for name in ("status", "cost", "n_waypoints", "waypoints"):
        only = g.nav_paths(starts, 64, outputs=(name,), stats=False)
        assert set(only) == {name, "stats"} and only[name].tobytes() == full[name].tobytes(), name
    M.assert_paths(g.nav_paths(starts, 64), full, "second call")
    one = g.nav_paths(starts[:1], 64)
    assert one["status"][0] == full["status"][0] and one["waypoints"].tobytes() == full["waypoints"][:1].tobytes()
    none = g.nav_paths(np.zeros((0, 3), F), 5)
    assert none["stats"] == dict(paths_reached=0, paths_unreachable=0, paths_blocked=0, paths_truncated=0, waypoints=0) and none["waypoints"].shape == (0, 5, 3)
    assert g.nav_query(np.zeros((0, 3), F)).shape == (0,) and g.nav_blocks(np.zeros((0, 3), np.int32)).shape == (0, spec["vps"] ** 3)
    if chunk:
        assert (g.nav_query(starts) == model.query(starts)).all()
    g.close()
    return {str(k): v for k, v in out.items()}


def case_lifetime(spec):
    vps = 8
    goals = np.array([centre(*OPEN_BOX_GOAL)], F)
    probe = np.array([centre(0, 0, 0), centre(-8, 15, 3)], F)
    idx0 = None
    beside = np.array([[2, 0, 0]], np.int32)                                     # a block on the box's +x face
    inside_new = np.array([centre(16 + 3, 3, 3)], F)

    def fresh():
        g = _stored("open_box", vps)
        return g, check(g, goals, "open box", radius_m=RADIUS)

    g, (stats, idx0, blocks, model) = fresh()
    # the field survives integrate / upload / fuse, and tiles that join later read BLOCKED
    f = mesh_case._frames(1, 64, 48)[0]
    g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.upload(*field_blocks([(16 + x, y, z) for x in range(8) for y in range(8) for z in range(8)], vps))
    src = mesh_case._integrator(0, 64, 48, vps=vps)
    src.upload(*field_blocks([(x, y, 40) for x in range(8) for y in range(8)], vps))
    g.fuse(src, np.array([1, 0, 0, 0, 0, 0, 0], F))
    src.close()
    assert len(g.block_indices()) > len(idx0)
    assert g.nav_blocks(idx0).tobytes() == blocks.tobytes()
    assert (g.nav_blocks(beside) == M.BLOCKED).all() and (g.nav_query(inside_new) == M.BLOCKED).all()
    assert g.nav_paths(inside_new, 8)["status"][0] == M.PATH_BLOCKED
    assert (g.nav_query(probe) == model.query(probe)).all()
    g.close()
    # each of these drops it
    drops = {"esdf_update": lambda g: g.esdf_update(**ECFG), "esdf_refresh": lambda g: g.esdf_refresh(),
             "remove_blocks": lambda g: g.remove_blocks(idx0[:1]), "clear_voxels": lambda g: g.clear_voxels(), "clear": lambda g: g.clear()}
    for name, drop in drops.items():
        g, _ = fresh()
        drop(g)
        for call in (lambda: g.nav_query(probe), lambda: g.nav_blocks(idx0), lambda: g.nav_paths(probe, 8)):
            assert "no stored field" in str(refused(B().KS_ERR_INVALID_ARG, call)), name
        if name not in ("clear_voxels", "clear"):                               # ... and a new update brings one back
            if name == "remove_blocks":
                g.esdf_refresh()
            check(g, goals, "after " + name, radius_m=RADIUS)
        g.close()
    # a removal that takes nothing out leaves it
    g, (stats, idx0, blocks, model) = fresh()
    g.remove_blocks(np.array([[40, 40, 40]], np.int32))
    assert g.nav_blocks(idx0).tobytes() == blocks.tobytes()
    # an update that fails leaves none stored
    refused(B().KS_ERR_INVALID_ARG, lambda: g.nav_update(goals, radius_m=-1.0))
    assert g.nav_blocks(idx0).tobytes() == blocks.tobytes()                      # (refused before anything was touched)
    s = _stored("serpentine", vps)
    near = np.array([centre(*serpentine_path()[0])], F)
    check(s, near, "serpentine", radius_m=RADIUS)
    assert refused_code(s, lambda: s.nav_update(near, radius_m=RADIUS, max_rounds=1)) == B().KS_ERR_UNSUPPORTED
    refused(B().KS_ERR_INVALID_ARG, lambda: s.nav_blocks(idx0))
    s.close()
    g.close()
    return dict(stats)


def case_reads_only(spec):
    vps = spec["vps"]
    goals = np.array([[-0.7, -0.7, -0.7], [0.7, 0.7, 0.7]], F)
    starts = esdf_read_points()

    def prepared():
        g = _stored("sphere", vps)
        g.mesh()
        g.objects()
        g.mesh_index()
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
                    mesh=im.blocks.tobytes(), index=(im.xyz.tobytes(), im.indices.tobytes(), im.object_ids.tobytes()))

    def calls(g):
        g.nav_update(goals, radius_m=0.1)
        g.nav_query(starts)
        g.nav_blocks(g.block_indices())
        g.nav_paths(starts, 32)

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


def esdf_read_points():
    rng = np.random.default_rng(6)
    return rng.uniform(-0.9, 0.9, (500, 3)).astype(F)


def case_errors(spec):
    L = B().lib()
    KS = B()
    g = mesh_case._integrator(0, 64, 48, vps=8)
    g.upload(*field_blocks(open_box_voxels(), 8))
    goals = np.array([centre(*OPEN_BOX_GOAL)], F)
    xyz = esdf_read_points()[:10]
    P = lambda a: a.ctypes.data
    out32, out8, wp = np.zeros(10, np.uint32), np.zeros(10, np.uint8), np.zeros((10, 4, 3), F)
    cfg, st, ps = g.nav_config(), KS.KsNavStats(), KS.KsNavPathStats()
    reads = [lambda: g.nav_query(xyz), lambda: g.nav_blocks(np.zeros((1, 3), np.int32)), lambda: g.nav_paths(xyz, 4),
             lambda: g.nav_query_device(8, 1, 8), lambda: g.nav_paths_device(8, 1, 4, d_status=8)]
    # no stored ESDF; then no stored field (the device addresses are never used)
    assert "no ESDF is stored" in str(refused(KS.KS_ERR_INVALID_ARG, lambda: g.nav_update(goals)))
    g.esdf_update(**ECFG)
    for call in reads:
        assert "no stored field" in str(refused(KS.KS_ERR_INVALID_ARG, call))
    # NULL ctx or cfg, NULL goals, n_goals outside 1..65536
    assert L.ks_nav_default_config(None) == KS.KS_ERR_INVALID_ARG
    assert L.ks_nav_update(None, P(goals), 1, ctypes.byref(cfg), ctypes.byref(st)) == KS.KS_ERR_INVALID_ARG
    assert L.ks_nav_update(g._h, P(goals), 1, None, ctypes.byref(st)) == KS.KS_ERR_INVALID_ARG
    assert L.ks_nav_update(g._h, None, 1, ctypes.byref(cfg), ctypes.byref(st)) == KS.KS_ERR_INVALID_ARG
    for n in (0, 65537, 1 << 40):
        assert L.ks_nav_update(g._h, P(goals), n, ctypes.byref(cfg), ctypes.byref(st)) == KS.KS_ERR_INVALID_ARG   # (refused before goals is read)
    for bad in (-0.1, float("nan"), float("inf"), float("-inf")):
        refused(KS.KS_ERR_INVALID_ARG, lambda: g.nav_update(goals, radius_m=bad))
    refused(KS.KS_ERR_INVALID_ARG, lambda: g.nav_update(goals, max_cost=M.MAX_COST + 1))
    refused(KS.KS_ERR_INVALID_ARG, lambda: g.nav_update(goals, max_cost=0xffffffff))
    for call in reads:
        refused(KS.KS_ERR_INVALID_ARG, call)                                    # ... and none of these stored anything
    # 65536 goals, all blocked but one; stats may be NULL
    many = np.full((65536, 3), np.nan, F)
    many[777] = goals[0]
    stats = g.nav_update(many, radius_m=RADIUS)
    assert stats["goals_used"] == 1 and stats["goals_blocked"] == 65535
    assert L.ks_nav_update(g._h, P(goals), 1, ctypes.byref(cfg), None) == 0
    stats, idx, blocks, model = check(g, goals, "open box", radius_m=RADIUS)
    # all goals blocked is no error: nothing is reached
    none = g.nav_update(np.array([[np.nan, 0, 0], centre(40, 0, 0)], F), radius_m=RADIUS)
    assert none["goals_used"] == 0 and none["goals_blocked"] == 2 and none["voxels_reached"] == 0 and none["largest_cost"] == 0 and none["rounds"] == 0
    assert (g.nav_blocks(idx) == M.UNREACHED).all()
    check(g, goals, "open box again", radius_m=RADIUS)
    # the reads: NULL ctx, NULL input or output with n > 0, n = 0 looks at no pointer, max_waypoints
    for fn in (L.ks_nav_query, L.ks_nav_query_device, L.ks_nav_download_blocks):
        assert fn(None, P(xyz), 1, P(out32)) == KS.KS_ERR_INVALID_ARG
        assert fn(g._h, None, 1, P(out32)) == KS.KS_ERR_INVALID_ARG
        assert fn(g._h, P(xyz), 1, None) == KS.KS_ERR_INVALID_ARG
        assert fn(g._h, None, 0, None) == 0
    for fn in (L.ks_nav_paths, L.ks_nav_paths_device):
        assert fn(None, P(xyz), 10, 4, P(out8), None, None, None, ctypes.byref(ps)) == KS.KS_ERR_INVALID_ARG
        assert fn(g._h, None, 10, 4, P(out8), None, None, None, ctypes.byref(ps)) == KS.KS_ERR_INVALID_ARG
        assert fn(g._h, P(xyz), 10, 4, None, None, None, None, ctypes.byref(ps)) == KS.KS_ERR_INVALID_ARG
        assert fn(g._h, None, 0, 4, None, None, None, None, ctypes.byref(ps)) == 0
        for bad in (0, 65537, 0xffffffff):
            assert fn(g._h, P(xyz), 10, bad, P(out8), None, None, None, ctypes.byref(ps)) == KS.KS_ERR_INVALID_ARG
    for ok in (1, 65536):
        got = g.nav_paths(xyz[:3], ok, outputs=("status", "cost", "n_waypoints"))
        M.assert_paths(got, M.paths(model, xyz[:3], ok), "max_waypoints %d" % ok)
    # ... and none of these changed the field
    assert g.nav_blocks(idx).tobytes() == blocks.tobytes()
    g.close()
    # an empty map with a stored ESDF is no error
    e = mesh_case._integrator(0, 64, 48, vps=8)
    e.esdf_update(**ECFG)
    stats = e.nav_update(goals)
    assert stats["goals_blocked"] == 1 and all(stats[k] == 0 for k in ("voxels_traversable", "voxels_reached", "goals_used", "largest_cost", "rounds"))
    assert (e.nav_query(xyz) == M.BLOCKED).all() and (e.nav_paths(xyz, 4)["status"] == M.PATH_BLOCKED).all()
    e.close()
    # a marcher context of the exact multi-GPU mode holds no voxel data
    marcher, owner = (mesh_case._integrator(1, 64, 48) for _ in range(2))
    f = mesh_case._frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    for call in (lambda: marcher.nav_update(goals), lambda: marcher.nav_query(xyz), lambda: marcher.nav_blocks(np.zeros((1, 3), np.int32)),
                 lambda: marcher.nav_paths(xyz, 4), lambda: marcher.nav_query_device(8, 1, 8), lambda: marcher.nav_paths_device(8, 1, 4, d_status=8)):
        refused(KS.KS_ERR_UNSUPPORTED, call)
    owner.esdf_update(**ECFG)
    assert owner.nav_update(goals, radius_m=0.0)["voxels_traversable"] > 0      # (the owner holds the map)
    marcher.close()
    owner.close()
    # a context in a failed state (the pool is full: sticky until a clear)
    small = mesh_case._integrator(0, 64, 48, max_tiles=8)
    try:
        small.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        raise AssertionError("a frame fitted 8 tiles")
    except KS.KsError as err:
        assert err.code == KS.KS_ERR_POOL_FULL, err
    for call in (lambda: small.nav_update(goals), lambda: small.nav_query(xyz), lambda: small.nav_paths(xyz, 4), lambda: small.nav_query_device(8, 1, 8)):
        assert "failed state" in str(refused(KS.KS_ERR_INVALID_ARG, call))
    small.close()
    return {}


def case_planted(spec):
    """A handful of free voxels at the ends of the linear index range of two blocks: nav_blocks against the model (goal voxels
    0, the other planted voxels unreached, everything else blocked)."""
    vps = spec["vps"]
    vox = mesh_case.planted_voxels(vps)
    g = mesh_case._integrator(0, 64, 48, vps=vps)
    g.upload(*field_blocks(vox, vps))
    g.esdf_update(**ECFG)
    goals = np.array([centre(*v) for v in vox[::2]], F)
    stats, idx, blocks, model = check(g, goals, "planted", radius_m=RADIUS)
    # ((-1, 0, 0) and (0, 0, 0) touch across the seam: one planted voxel that is no goal is reached, at the cost of a face step)
    assert len(idx) == 2 and stats["voxels_traversable"] == len(vox) and stats["goals_used"] == len(goals), stats
    assert (blocks == 0).sum() == len(goals) and stats["voxels_reached"] == len(goals) + 1 and (blocks == M.UNREACHED).sum() == len(vox) - len(goals) - 1
    assert (blocks != M.BLOCKED).sum() == len(vox)
    g.close()
    return dict(stats)


CASES = {"planted": case_planted, "open_box": case_open_box, "seams": case_seams, "serpentine": case_serpentine, "random": case_random, "radius": case_radius,
         "max_cost": case_max_cost, "paths": case_paths, "lifetime": case_lifetime, "reads_only": case_reads_only, "errors": case_errors}

# name -> (spec, extra environment): the same cases in both tiers
SPECS = {}
for _vps in (8, 16, 32):
    for _case in ("open_box", "seams", "random"):
        SPECS["%s_vps%d" % (_case, _vps)] = (dict(case=_case, vps=_vps), {})
SPECS.update({
    "serpentine_vps8": (dict(case="serpentine", vps=8), {}),
    "serpentine_vps16": (dict(case="serpentine", vps=16), {}),
    "serpentine_vps32": (dict(case="serpentine", vps=32), {}),
    "paths_vps32": (dict(case="paths", vps=32), {}),
    "planted_vps64": (dict(case="planted", vps=64), {}),
    "radius_vps8": (dict(case="radius", vps=8), {}),
    "max_cost_vps8": (dict(case="max_cost", vps=8), {}),
    "paths_vps8": (dict(case="paths", vps=8), {}),
    "paths_chunked_vps16": (dict(case="paths", vps=16, chunk=200), {"KS_DEBUG": "1", "KS_NAV_CHUNK": "200"}),
    "lifetime": (dict(case="lifetime"), {}),
    "reads_only_vps8": (dict(case="reads_only", vps=8), {}),
    "errors": (dict(case="errors"), {}),
})


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("NAV_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
