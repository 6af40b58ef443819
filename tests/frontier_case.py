"""The frontier cases (ks_frontiers_update, _size, _download, _download_blocks, _query; DESIGN.md, section "Exploration frontiers"),
shared by both tiers like those of tests/nav_case.py: the GPU tier (tests/test_frontier_gpu.py) calls run_case in-process, the CPU
tier (tests/test_frontier_cpu.py) runs it as a child process on the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.frontier_case '<json spec>'
The checker is tests/frontier_model.py on the stored ESDF (and the stored navigation field) as the library hands them out; every
comparison is byte for byte.  The fields are shaped by uploads and ks_esdf_update with nav_case.ECFG (min 0.1 m, max 0.4 m): a FREE
voxel is observed with a TSDF distance of 0.3 m, a WALL voxel is observed with distance 0: a site, so its stored distance is 0 and a
free voxel beside it stores exactly voxel_size.  With radius_m = 0.04 every observed voxel that is no wall is traversable."""
import ctypes
import json
import os
import sys

import numpy as np

from tests import esdf_case, mesh_case, nav_case, objects_case
from tests import esdf_read_model as E
from tests import frontier_model as M
from tests import nav_model as N

VOXEL = mesh_case.VOXEL
F = np.float32
FREE, WALL = nav_case.FREE, (0, 1.0, 0.0)
ECFG = nav_case.ECFG
SMALL = 0.04                      # below the distance of a voxel beside a wall (0.05)
NONE = int(M.NONE)
UNREACHED = N.UNREACHED
RANDOM_SEED = 2                   # chosen on the CPU with the model: tests/test_frontier_cpu.py asserts what it is chosen for
refused = objects_case.refused
centre = nav_case.centre


def B():
    from kimera_semantics_amd import binding
    return binding


# ---- fields: {voxel: FREE | WALL} and the positions whose blocks are resident without an observed voxel ---------------------------
def cube_voxels():
    r = range(-5, 5)
    return {(x, y, z): FREE for x in r for y in r for z in r}


def room_voxels(door):
    r = range(-6, 6)
    vox = {(x, y, z): (WALL if -6 in (x, y, z) or 5 in (x, y, z) else FREE) for x in r for y in r for z in r}
    if door:
        for y in (-1, 0):
            for z in (-1, 0):
                vox[(5, y, z)] = FREE
    return vox


FACE_DIRS = ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1))     # (axis, sign) in the order -x +x -y +y -z +z
# (the items of the faces field lie 48 apart along x: a block of 16 before each home block and one behind it)


def _boxed(home, open_axis, open_sign, beyond):
    """A free voxel with walls on five faces; the sixth neighbour is `beyond`: 0 its block absent, 1 resident and never observed,
    2 observed (a wall)."""
    vox, resident = {home: FREE}, []
    for axis, sign in FACE_DIRS:
        n = list(home)
        n[axis] += sign
        if (axis, sign) != (open_axis, open_sign):
            vox[tuple(n)] = WALL
        elif beyond == 2:
            vox[tuple(n)] = WALL
        elif beyond == 1:
            resident.append(tuple(n))
    return vox, resident


def faces_field(nan=False):
    """({voxel: record}, resident positions).  Item s sits at x = 48 * s; its home voxel lies on the skin of a block of 16 (and so of a
    tile).  With `nan` one more observed voxel holds a NaN distance: only a hand-made store can (tests/test_frontier_cpu.py); the ESDF
    never stores one."""
    vox, resident = {}, []

    def add(item):
        vox.update(item[0])
        resident.extend(item[1])

    for k, (axis, sign) in enumerate(FACE_DIRS):
        for beyond in range(3):
            home = [48 * (3 * k + beyond) + 19, 19, 19]
            home[axis] += -3 if sign < 0 else 12                # 16 or 31: the first or last voxel of the home block
            add(_boxed(tuple(home), axis, sign, beyond))
    for beyond in range(3):                                      # -y across the origin into negative indices
        add(_boxed((48 * (18 + beyond) + 19, 0, 19), 1, -1, beyond))
    add(_boxed((48 * 21 + 19, 19, 19), 0, 1, 2))                 # every face observed: only edges and corners see unknown space
    o = 48 * 22
    vox[(o + 7, 7, 7)] = vox[(o + 8, 8, 8)] = FREE               # they touch across a tile corner only
    o = 48 * 23
    vox[(o + 8, 7, 4)] = vox[(o + 7, 8, 4)] = FREE               # a backward diagonal across a tile edge
    vox[(48 * 24 + 19, 19, 19)] = WALL                           # a wall alone: observed, not traversable
    if nan:
        vox[(48 * 25 + 19, 19, 19)] = (0, 1.0, float("nan"))
    return vox, resident


# first_voxel -> (n_voxels, unknown_faces) of the faces field with radius_m = 0.04 (and with float32(VOXEL)), min_voxels = 1
FACES_EXPECTED = {
    (16, 19, 19): (1, 1), (64, 19, 19): (1, 1),        # -x: the block beyond is absent | resident and unobserved (observed: none)
    (175, 19, 19): (1, 1), (223, 19, 19): (1, 1),      # +x
    (307, 16, 19): (1, 1), (355, 16, 19): (1, 1),      # -y
    (451, 31, 19): (1, 1), (499, 31, 19): (1, 1),      # +y
    (595, 19, 16): (1, 1), (643, 19, 16): (1, 1),      # -z
    (739, 19, 31): (1, 1), (787, 19, 31): (1, 1),      # +z
    (883, 0, 19): (1, 1), (931, 0, 19): (1, 1),        # -y from y = 0 into y = -1
    (1063, 7, 7): (2, 12),                             # (7,7,7)-(8,8,8): one component, the faces of both
    (1111, 8, 4): (2, 12),                             # (8,7,4)-(7,8,4)
}
# ... and with the float32 after float32(VOXEL): every voxel beside a wall has gone
FACES_EXPECTED_ABOVE = {(1063, 7, 7): (2, 12), (1111, 8, 4): (2, 12)}
RADIUS_EQUAL = float(F(VOXEL))
RADIUS_ABOVE = float(np.nextafter(F(VOXEL), F(1)))


def random_voxels(seed=RANDOM_SEED):
    """4 x 4 x 4 tiles from (-16)^3: the outermost layer walls; inside 2 % never observed, 30 % walls, the rest free."""
    rng = np.random.default_rng(seed)
    u = rng.random((32, 32, 32))
    vox = {}
    for x in range(32):
        for y in range(32):
            for z in range(32):
                edge = 0 in (x, y, z) or 31 in (x, y, z)
                if edge or u[x, y, z] >= 0.02:
                    vox[(x - 16, y - 16, z - 16)] = WALL if edge or u[x, y, z] < 0.32 else FREE
    return vox


def island_voxels():
    r = range(40, 44)
    return {(x, y, z): FREE for x in r for y in r for z in r}


def hand_store(vox, vps, resident=()):
    """The ESDF store such a field leads to, made by hand for the checks that need no library: a wall stores 0, a free voxel beside
    a wall voxel_size, any other free voxel the clamp 0.4; a record whose distance is a NaN keeps it."""
    at = sorted({tuple(int(c) // vps for c in p) for p in list(vox) + list(resident)})
    row = {b: j for j, b in enumerate(at)}
    rec = np.zeros((len(at), vps ** 3), [("distance", "<f4"), ("flags", "u1"), ("label", "u1"), ("pad", "u1", (2,))])
    rec["label"] = 255
    for (x, y, z), (_, _, d) in vox.items():
        j, l = row[(x // vps, y // vps, z // vps)], (x % vps) + vps * ((y % vps) + vps * (z % vps))
        if d == 0.0:
            value = 0.0
        elif d != d:
            value = d
        else:
            beside = any(vox.get((x + dx, y + dy, z + dz), FREE)[2] == 0.0 for dx, dy, dz in M.FACES)
            value = VOXEL if beside else 0.4
        rec["distance"][j, l], rec["flags"][j, l] = value, 1
    return E.Store(np.array(at, np.int32).reshape(-1, 3), rec, vps)


def crossing_a_seam(rec):
    return int(((rec["bb_min"] >> 3) != (rec["bb_max"] >> 3)).any(axis=1).sum())


# ---- a stored ESDF, and one update against the model ----------------------------------------------------------------------------
def _stored(vox, vps, resident=(), reverse=False, **extra):
    g = mesh_case._integrator(0, 64, 48, vps=vps, **extra)
    idx, t, s = objects_case.voxel_field(vox, vps, resident=resident)
    if reverse:
        idx, t, s = idx[::-1].copy(), t[::-1].copy(), s[::-1].copy()
    g.upload(idx, t, s)
    g.esdf_update(**ECFG)
    return g


def ring_of(idx):
    """The blocks and a ring of absent ones around their box."""
    have = {tuple(int(v) for v in r) for r in idx}
    lo, hi = idx.min(axis=0) - 1, idx.max(axis=0) + 1
    extra = [(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]
    return np.concatenate([idx, np.array([e for e in extra if e not in have], np.int32).reshape(-1, 3)])


def check(g, what, field=None, model=None, **cfg):
    """One update against the model: (records, stats, block indices, ids, model).  field: the nav_model.Field of what is stored."""
    rec, stats = g.frontiers(**cfg)
    idx = ring_of(g.block_indices()) if len(g.block_indices()) else g.block_indices()
    ids = g.frontier_ids(idx)
    model = model or M.model_of(g, field, **cfg)
    M.assert_same((rec, stats), model, idx, ids, what)
    assert stats["workspace_bytes"] == M.workspace_bytes(len(g.tile_keys()), stats["components"]), (what, stats)
    assert (rec["pad"] == 0).all()
    # the point query: the centres of the frontier voxels and of as many other voxels
    z, y, x = np.nonzero(model.part)
    ijk = np.stack([x, y, z], axis=1) + model.origin
    rng = np.random.default_rng(9)
    if len(ijk) > 600:
        ijk = ijk[rng.choice(len(ijk), 600, replace=False)]
    ijk = np.concatenate([ijk, ijk + rng.integers(-3, 4, ijk.shape)]) if len(ijk) else np.zeros((1, 3), np.int64)
    xyz = ((ijk + 0.5 + rng.uniform(-0.4, 0.4, ijk.shape)) * VOXEL).astype(F)
    got = g.frontier_query(xyz)
    assert got.dtype == np.uint32 and (got == model.at(ijk)).all(), (what, np.argwhere(got != model.at(ijk))[:5])
    return rec, stats, idx, ids, model


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def case_cube(spec):
    g = _stored(cube_voxels(), spec["vps"])
    rec, stats, idx, ids, model = check(g, "cube", radius_m=SMALL)
    assert len(rec) == 1 and stats["components"] == 1 and stats["voxels_traversable"] == 1000, stats
    r = rec[0]
    assert r["n_voxels"] == 488 and r["unknown_faces"] == 600 and stats["voxels_frontier"] == 488 and stats["unknown_faces"] == 600
    assert tuple(r["first_voxel"]) == (-5, -5, -5) and tuple(r["bb_min"]) == (-5, -5, -5) and tuple(r["bb_max"]) == (4, 4, 4)
    assert tuple(r["sum"]) == (-244, -244, -244) and (B().frontier_centroids(rec, VOXEL) == 0.0).all()
    assert r["nav_cost"] == UNREACHED and tuple(r["nav_voxel"]) == (-5, -5, -5) and stats["nav_field_used"] == 0
    assert (ids != NONE).sum() == 488 and (g.frontier_query(np.array([centre(0, 0, 0), centre(4, 0, 0), centre(5, 0, 0)], F)) == [NONE, 0, NONE]).all()
    if spec["vps"] == 8:
        assert len(g.tile_keys()) == 8
    # a second call gives the same bytes
    rec2, stats2 = g.frontiers(radius_m=SMALL)
    assert rec2.tobytes() == rec.tobytes() and stats2 == stats and g.frontier_ids(idx).tobytes() == ids.tobytes()
    g.close()
    return dict(stats)


def case_room(spec):
    g = _stored(room_voxels(False), spec["vps"])
    rec, stats, idx, ids, _ = check(g, "closed room", radius_m=SMALL, min_voxels=1)
    assert len(rec) == 0 and stats["components"] == 0 and stats["voxels_frontier"] == 0 and stats["voxels_traversable"] == 1000 and (ids == NONE).all()
    g.close()
    g = _stored(room_voxels(True), spec["vps"])
    rec, stats, idx, ids, _ = check(g, "room with a door", radius_m=SMALL, min_voxels=1)
    assert M.by_first(rec) == {(5, -1, -1): (4, 4)} and stats["voxels_traversable"] == 1004 and (ids != NONE).sum() == 4, (rec, stats)
    rec8, stats8, _, ids8, _ = check(g, "room with a door, min_voxels 8", radius_m=SMALL)
    assert len(rec8) == 0 and stats8["components"] == 1 and stats8["voxels_frontier"] == 4 and (ids8 == NONE).all()
    g.close()
    return dict(stats)


def case_faces(spec):
    vox, resident = faces_field()
    g = _stored(vox, spec["vps"], resident=resident)
    rec, stats, idx, ids, model = check(g, "faces", radius_m=SMALL, min_voxels=1)
    assert M.by_first(rec) == FACES_EXPECTED, M.by_first(rec)
    assert stats["components"] == stats["frontiers"] == len(FACES_EXPECTED) and stats["unknown_faces"] == 14 + 24
    # the six homes whose sixth neighbour is observed, the voxel that sees unknown space across edges and corners only, the wall
    quiet = [(48 * (3 * k + 2) + 19 + (a == 0) * (-3 if s < 0 else 12), 19 + (a == 1) * (-3 if s < 0 else 12), 19 + (a == 2) * (-3 if s < 0 else 12))
             for k, (a, s) in enumerate(FACE_DIRS)] + [(48 * 20 + 19, 0, 19), (48 * 21 + 19, 19, 19), (48 * 24 + 19, 19, 19)]
    store = E.store_of(g)
    _, flags, _ = store.records(np.array(quiet, np.int64))
    assert (flags & 1).all() and (g.frontier_query(np.array([centre(*q) for q in quiet], F)) == NONE).all()
    # a stored distance equal to radius_m bit for bit takes part; one float32 above it, it does not
    d, _, _ = store.records(np.array([(16, 19, 19)], np.int64))
    assert d[0].tobytes() == F(VOXEL).tobytes()
    rec_e, _, _, _, _ = check(g, "radius equal to a stored distance", radius_m=RADIUS_EQUAL, min_voxels=1)
    assert M.by_first(rec_e) == FACES_EXPECTED
    rec_a, stats_a, _, _, _ = check(g, "radius one float above it", radius_m=RADIUS_ABOVE, min_voxels=1)
    assert M.by_first(rec_a) == FACES_EXPECTED_ABOVE and stats_a["voxels_traversable"] == 4, stats_a
    g.close()
    return dict(stats)


def case_random(spec):
    g = _stored(random_voxels(), spec["vps"])
    rec, stats, idx, ids, model = check(g, "random, min_voxels 1", radius_m=SMALL, min_voxels=1)
    n = rec["n_voxels"]
    assert stats["components"] >= 100 and (n == 1).sum() >= 5 and n.max() >= 300 and crossing_a_seam(rec) >= 20, (stats, n.max(), crossing_a_seam(rec))
    rec8, stats8, _, ids8, _ = check(g, "random, min_voxels 8", radius_m=SMALL)
    assert stats8["components"] == stats["components"] > stats8["frontiers"] > 0 and (ids8 == NONE).sum() > (ids == NONE).sum()
    g.close()
    return dict(stats, singletons=int((n == 1).sum()), crossing=crossing_a_seam(rec), largest=int(n.max()))


def case_order(spec):
    """The same voxels uploaded in another block order (other slots) give the same bytes, the join included."""
    vox = random_voxels()
    a, b = _stored(vox, spec["vps"]), _stored(vox, spec["vps"], reverse=True)
    ka, kb = a.tile_keys(), b.tile_keys()
    assert sorted(ka) == sorted(kb) and (ka != kb).any()
    goal = np.array([centre(*next(v for v in sorted(vox) if vox[v] == FREE and v >= (0, 0, 0)))], F)
    for g in (a, b):
        g.nav_update(goal, radius_m=SMALL, max_cost=150)                        # (a cap: some frontiers stay unreached)
    field = N.model_of(a, goal, radius_m=SMALL, max_cost=150)
    ra, sa, idx, ia, model = check(a, "forward order", field=field, radius_m=SMALL, min_voxels=2)
    rb, sb, idx_b, ib, _ = check(b, "reversed order", model=model, radius_m=SMALL, min_voxels=2)
    assert (idx == idx_b).all() and ra.tobytes() == rb.tobytes() and ia.tobytes() == ib.tobytes() and sa == sb
    assert (ra["nav_cost"] <= N.MAX_COST).any() and (ra["nav_cost"] == UNREACHED).any()
    a.close()
    b.close()
    return dict(sa)


def case_bounds(spec):
    g = _stored(cube_voxels(), spec["vps"])
    # the four faces across y and z are outside: what is left of the shell is the inside of the two faces across x
    rec, stats, _, ids, _ = check(g, "two patches", radius_m=SMALL, use_bounds=1, bounds_min=(-5, -4, -4), bounds_max=(4, 3, 3))
    assert M.by_first(rec) == {(-5, -4, -4): (64, 64), (4, -4, -4): (64, 64)} and stats["voxels_traversable"] == 1000, (rec, stats)
    # bounds that hold the cube and nothing else: every unobserved voxel lies outside them and still counts as a neighbour
    rec, stats, _, _, _ = check(g, "bounds = the cube", radius_m=SMALL, use_bounds=1, bounds_min=(-5, -5, -5), bounds_max=(4, 4, 4))
    assert M.by_first(rec) == {(-5, -5, -5): (488, 600)}
    rec, stats, _, ids, _ = check(g, "one voxel", radius_m=SMALL, min_voxels=1, use_bounds=1, bounds_min=(4, 4, 4), bounds_max=(4, 4, 4))
    assert M.by_first(rec) == {(4, 4, 4): (1, 3)}
    rec, stats, _, ids, _ = check(g, "elsewhere", radius_m=SMALL, use_bounds=1, bounds_min=(20, 20, 20), bounds_max=(30, 30, 30))
    assert len(rec) == 0 and stats["voxels_frontier"] == 0 and stats["voxels_traversable"] == 1000 and (ids == NONE).all()
    rec, stats, _, _, _ = check(g, "bounds not used", radius_m=SMALL, use_bounds=0, bounds_min=(9, 9, 9), bounds_max=(0, 0, 0))
    assert M.by_first(rec) == {(-5, -5, -5): (488, 600)}
    # the helper that makes such bounds from a metric box
    lo, hi = B().frontier_bounds([-0.25, -0.2, -0.2], [0.249, 0.199, 0.199], VOXEL)
    assert tuple(lo) == (-5, -4, -4) and tuple(hi) == (4, 3, 3)
    g.close()
    return dict(stats)


def case_nav(spec):
    vps = spec["vps"]
    box = {v: FREE for v in nav_case.open_box_voxels()}
    goal = np.array([centre(*nav_case.OPEN_BOX_GOAL)], F)
    # 1) the open box and an island the field does not reach
    g = _stored({**box, **island_voxels()}, vps)
    rec0, stats0, idx, _, _ = check(g, "no stored field", radius_m=0.3)
    assert stats0["nav_field_used"] == 0 and (rec0["nav_cost"] == UNREACHED).all() and (rec0["nav_voxel"] == rec0["first_voxel"]).all() and len(rec0) == 2
    g.nav_update(goal, radius_m=0.3)
    assert g.frontier_records().tobytes() == rec0.tobytes()                     # the field is read at the call: the records stay
    field = N.model_of(g, goal, radius_m=0.3)
    rec, stats, _, ids, model = check(g, "open box and island", field=field, radius_m=0.3)
    assert stats["nav_field_used"] == 1 and M.by_first(rec) == {(-8, -8, -8): (24 ** 3 - 22 ** 3, 6 * 24 * 24), (40, 40, 40): (56, 96)}
    assert field.at([(-8, 5, 3)])[0] == field.at([(2, 15, 3)])[0] == 100          # the tie exists
    assert rec["nav_cost"][0] == 100 and tuple(rec["nav_voxel"][0]) == (-8, 5, 3)
    assert rec["nav_cost"][1] == UNREACHED and tuple(rec["nav_voxel"][1]) == tuple(rec["first_voxel"][1]) == (40, 40, 40)
    target = B().frontier_targets(rec, VOXEL)
    assert target.dtype == F and target.tobytes() == ((rec["nav_voxel"].astype(F) + F(0.5)) * F(VOXEL)).tobytes()
    walk = g.nav_paths(target, 64)
    assert walk["status"][0] == N.REACHED and walk["cost"][0] == 100 and walk["status"][1] == N.UNREACHABLE
    g.close()
    # 2) a frontier radius below the field's: a wall inside the box blocks the field around it, not the frontier
    walled = dict(box)
    walled[(-7, 5, 3)] = WALL
    g = _stored(walled, vps)
    g.nav_update(goal, radius_m=0.3)
    field = N.model_of(g, goal, radius_m=0.3)
    rec, stats, _, _, model = check(g, "radius below the field's", field=field, radius_m=SMALL)
    z, y, x = np.nonzero(model.part)
    cost = field.at(np.stack([x, y, z], axis=1) + model.origin)
    assert (cost == N.BLOCKED).sum() > 10 and field.at([(-8, 5, 3)])[0] == N.BLOCKED and len(rec) == 1
    assert rec["nav_cost"][0] == 100 and tuple(rec["nav_voxel"][0]) == (2, 15, 3)
    g.close()
    return dict(stats)


def _frame_totals(st):
    return (st.n_rays_cast, st.n_voxel_updates)


def case_lifetime(spec):
    vps = 8
    vox = cube_voxels()
    probe = np.array([centre(4, 0, 0)], F)

    def fresh(**extra):
        g = _stored(vox, vps, **extra)
        return g, check(g, "cube", radius_m=SMALL)

    g, (rec, stats, idx0, ids, model) = fresh()
    blocks0 = g.block_indices()
    # the result survives integrate / upload / fuse; tiles that join later read NONE
    f = mesh_case._frames(1, 64, 48)[0]
    g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.upload(*objects_case.voxel_field({(16 + x, y, z): FREE for x in range(8) for y in range(8) for z in range(8)}, vps))
    src = mesh_case._integrator(0, 64, 48, vps=vps)
    src.upload(*objects_case.voxel_field({(x, y, 40): FREE for x in range(8) for y in range(8)}, vps))
    g.fuse(src, np.array([1, 0, 0, 0, 0, 0, 0], F))
    src.close()
    assert len(g.block_indices()) > len(blocks0)
    assert g.frontier_records().tobytes() == rec.tobytes() and g.frontier_ids(idx0).tobytes() == ids.tobytes()
    assert (g.frontier_ids(np.array([[2, 0, 0]], np.int32)) == NONE).all() and g.frontier_query(probe)[0] == 0
    g.close()
    # each of these drops it
    drops = {"esdf_update": lambda g: g.esdf_update(**ECFG), "esdf_refresh": lambda g: g.esdf_refresh(), "remove_blocks": lambda g: g.remove_blocks(blocks0[:1]),
             "clear_voxels": lambda g: g.clear_voxels(), "clear": lambda g: g.clear()}
    n = ctypes.c_size_t()
    for name, drop in drops.items():
        g, _ = fresh()
        out = drop(g)
        if name == "esdf_refresh":
            assert out["tiles_stale"] == 0, out                                 # (a refresh that finds nothing stale)
        for call in (lambda: g.frontier_records(), lambda: g.frontier_ids(idx0), lambda: g.frontier_query(probe)):
            assert "no frontiers are stored" in str(refused(B().KS_ERR_INVALID_ARG, call)), name
        assert B().lib().ks_frontiers_size(g._h, ctypes.byref(n)) == B().KS_ERR_INVALID_ARG
        if name in ("esdf_update", "esdf_refresh"):                             # ... and a new update brings one back
            assert check(g, "after " + name, radius_m=SMALL)[0].tobytes() == rec.tobytes()
        g.close()
    # a refresh that recomputes something drops it as well
    g, _ = fresh()
    g.upload(*objects_case.voxel_field({(0, 0, 0): WALL}, vps))
    assert g.esdf_refresh()["tiles_stale"] > 0
    refused(B().KS_ERR_INVALID_ARG, lambda: g.frontier_records())
    check(g, "after a refresh with work", radius_m=SMALL)
    # a removal that takes nothing out leaves it; an update that is refused before it starts leaves it; one that fails drops it
    rec1, ids1 = g.frontier_records(), g.frontier_ids(idx0)
    g.remove_blocks(np.array([[40, 40, 40]], np.int32))
    assert g.frontier_records().tobytes() == rec1.tobytes() and g.frontier_ids(idx0).tobytes() == ids1.tobytes()
    refused(B().KS_ERR_INVALID_ARG, lambda: g.frontiers(radius_m=-1.0))
    assert g.frontier_records().tobytes() == rec1.tobytes()
    g.close()
    # frames in flight are completed by the update and their statistics stay owed
    a, b = (_stored(vox, 16, pipeline=12) for _ in range(2))
    for g in (a, b):
        st = g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        assert _frame_totals(st) == (0, 0)                                      # (in flight)
    a.frontiers(radius_m=SMALL)
    a.frontier_ids(idx0[:1])
    owed_a, owed_b = _frame_totals(a.flush()), _frame_totals(b.flush())
    assert owed_a == owed_b and owed_a[1] > 0, (owed_a, owed_b)
    a.close()
    b.close()
    return dict(stats)


def case_reads_only(spec):
    vps = spec["vps"]
    goals = np.array([[-0.7, -0.7, -0.7], [0.7, 0.7, 0.7]], F)
    points = nav_case.esdf_read_points()

    def prepared():
        g = nav_case._stored("sphere", vps)
        g.mesh()
        g.objects()
        g.mesh_index()
        g.nav_update(goals, radius_m=0.1)
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
                    nav=g.nav_blocks(idx).tobytes(), mesh=im.blocks.tobytes(), index=(im.xyz.tobytes(), im.indices.tobytes(), im.object_ids.tobytes()))

    def calls(g):
        rec, stats = g.frontiers(radius_m=0.1)
        assert stats["nav_field_used"] == 1 and stats["frontiers"] > 0, stats
        g.frontier_query(points)
        g.frontier_ids(g.block_indices())

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


def case_integrated(spec):
    from kimera_semantics_amd import synth
    w, h = 160, 120
    g = mesh_case._integrator(0, w, h, vps=16, pipeline=12, max_tiles=1 << 13)
    frames = mesh_case._frames(4, w, h)
    for f in frames:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.esdf_update()
    goal = np.array([frames[-1].T_G_C[4:7]], F)
    nav = g.nav_update(goal)
    field = N.model_of(g, goal)
    rec, stats, idx, ids, model = check(g, "integrated", field=field)
    assert stats["frontiers"] >= 2 and stats["components"] >= stats["frontiers"] and stats["nav_field_used"] == 1, stats
    g.close()
    return dict(stats, reached=int((rec["nav_cost"] <= N.MAX_COST).sum()), nav_reached=nav["voxels_reached"])


def case_errors(spec):
    KS = B()
    L = KS.lib()
    g = mesh_case._integrator(0, 64, 48, vps=8)
    g.upload(*objects_case.voxel_field(cube_voxels(), 8))
    idx = g.block_indices()
    xyz = nav_case.esdf_read_points()[:10]
    P = lambda a: a.ctypes.data
    n, one, out32 = ctypes.c_size_t(), np.zeros(1, KS.FRONTIER_DTYPE), np.zeros(512, np.uint32)
    cfg, st = g.frontier_config(radius_m=SMALL), KS.KsFrontierStats()
    assert ctypes.sizeof(KS.KsFrontierConfig) == 40 and ctypes.sizeof(KS.KsFrontierStats) == 72 and KS.FRONTIER_DTYPE.itemsize == 88
    d = g.frontier_config()
    assert (round(d.radius_m, 6), d.min_voxels, d.use_bounds, d.pad) == (0.3, 8, 0, 0)
    reads = [lambda: g.frontier_records(), lambda: g.frontier_ids(idx), lambda: g.frontier_query(xyz)]
    # no stored ESDF; then no stored result
    assert "no ESDF is stored" in str(refused(KS.KS_ERR_INVALID_ARG, lambda: g.frontiers()))
    g.esdf_update(**ECFG)
    for call in reads:
        assert "no frontiers are stored" in str(refused(KS.KS_ERR_INVALID_ARG, call))
    assert L.ks_frontiers_size(g._h, ctypes.byref(n)) == KS.KS_ERR_INVALID_ARG
    assert L.ks_frontiers_download(g._h, P(one), 1, ctypes.byref(n)) == KS.KS_ERR_INVALID_ARG
    # NULL ctx or cfg, the configuration
    assert L.ks_frontiers_default_config(None) == KS.KS_ERR_INVALID_ARG
    assert L.ks_frontiers_update(None, ctypes.byref(cfg), ctypes.byref(st)) == KS.KS_ERR_INVALID_ARG
    assert L.ks_frontiers_update(g._h, None, ctypes.byref(st)) == KS.KS_ERR_INVALID_ARG
    for bad in (-0.1, float("nan"), float("inf"), float("-inf")):
        refused(KS.KS_ERR_INVALID_ARG, lambda: g.frontiers(radius_m=bad))
    refused(KS.KS_ERR_INVALID_ARG, lambda: g.frontiers(min_voxels=0))
    for axis in range(3):
        lo = [0, 0, 0]
        lo[axis] = 1
        refused(KS.KS_ERR_INVALID_ARG, lambda: g.frontiers(use_bounds=1, bounds_min=lo, bounds_max=(0, 0, 0)))
    for call in reads:
        refused(KS.KS_ERR_INVALID_ARG, call)                                    # ... and none of these stored anything
    # stats may be NULL; the closed form of the work space (check); radius 0 is allowed
    assert L.ks_frontiers_update(g._h, ctypes.byref(cfg), None) == 0
    rec, stats, _, ids, _ = check(g, "cube", radius_m=SMALL)
    assert stats["workspace_bytes"] == 8 * (5120 + 128) + 96 + 196 and len(rec) == 1
    assert g.frontiers(radius_m=0.0)[1]["voxels_traversable"] == 1000
    check(g, "cube again", radius_m=SMALL)
    # capacity too small; NULL input or output with n > 0; n = 0 looks at no pointer
    assert L.ks_frontiers_size(None, ctypes.byref(n)) == KS.KS_ERR_INVALID_ARG and L.ks_frontiers_size(g._h, None) == KS.KS_ERR_INVALID_ARG
    assert L.ks_frontiers_size(g._h, ctypes.byref(n)) == 0 and n.value == 1
    n.value = 99
    assert L.ks_frontiers_download(g._h, P(one), 0, ctypes.byref(n)) == KS.KS_ERR_INVALID_ARG and n.value == 1
    assert L.ks_frontiers_download(g._h, None, 1, ctypes.byref(n)) == KS.KS_ERR_INVALID_ARG
    assert L.ks_frontiers_download(None, P(one), 1, ctypes.byref(n)) == KS.KS_ERR_INVALID_ARG
    assert L.ks_frontiers_download(g._h, P(one), 1, None) == 0 and one.tobytes() == rec.tobytes()
    for fn, arg in ((L.ks_frontiers_download_blocks, idx), (L.ks_frontiers_query, xyz)):
        assert fn(None, P(arg), 1, P(out32)) == KS.KS_ERR_INVALID_ARG
        assert fn(g._h, None, 1, P(out32)) == KS.KS_ERR_INVALID_ARG
        assert fn(g._h, P(arg), 1, None) == KS.KS_ERR_INVALID_ARG
        assert fn(g._h, None, 0, None) == 0
    far = np.array([[1e9, 0, 0], [float("nan"), 0, 0], [0, 0, float("inf")]], F)
    assert (g.frontier_query(far) == NONE).all() and g.frontier_query(np.zeros((0, 3), F)).shape == (0,)
    assert g.frontier_ids(idx).tobytes() == ids[:len(idx)].tobytes()             # ... and none of these changed what is stored
    g.close()
    # an empty map with a stored ESDF is no error: zero records
    e = mesh_case._integrator(0, 64, 48, vps=8)
    e.esdf_update(**ECFG)
    rec, stats = e.frontiers()
    assert len(rec) == 0 and all(stats[k] == 0 for k in M.STAT_KEYS) and stats["workspace_bytes"] == 96, stats
    assert (e.frontier_ids(idx[:2]) == NONE).all() and (e.frontier_query(xyz) == NONE).all()
    e.close()
    # a marcher context of the exact multi-GPU mode holds no voxel data
    marcher, owner = (mesh_case._integrator(1, 64, 48) for _ in range(2))
    f = mesh_case._frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    for call in (lambda: marcher.frontiers(), lambda: marcher.frontier_records(), lambda: marcher.frontier_ids(idx[:1]), lambda: marcher.frontier_query(xyz)):
        refused(KS.KS_ERR_UNSUPPORTED, call)
    owner.esdf_update(**ECFG)
    assert owner.frontiers(radius_m=0.0)[1]["voxels_traversable"] > 0            # (the owner holds the map)
    marcher.close()
    owner.close()
    # a context in a failed state (the pool is full: sticky until a clear)
    small = mesh_case._integrator(0, 64, 48, max_tiles=8)
    try:
        small.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        raise AssertionError("a frame fitted 8 tiles")
    except KS.KsError as err:
        assert err.code == KS.KS_ERR_POOL_FULL, err
    for call in (lambda: small.frontiers(), lambda: small.frontier_records(), lambda: small.frontier_query(xyz)):
        assert "failed state" in str(refused(KS.KS_ERR_INVALID_ARG, call))
    small.close()
    return {}


def case_planted(spec):
    """A handful of free voxels at the ends of the linear index range of two blocks: the per-voxel ids of the block export against
    the model ((-1, 0, 0) and (0, 0, 0) touch across the seam and make one frontier of two)."""
    vox = mesh_case.planted_voxels(spec["vps"])
    g = _stored({v: FREE for v in vox}, spec["vps"])
    rec, stats, idx, ids, model = check(g, "planted", radius_m=SMALL, min_voxels=1)
    assert len(g.block_indices()) == 2 and stats["voxels_frontier"] == stats["voxels_in_frontiers"] == (ids != NONE).sum() == len(vox), stats
    assert stats["frontiers"] == len(vox) - 1 and stats["largest_frontier_voxels"] == 2, stats
    g.close()
    return dict(stats)


CASES = {"planted": case_planted, "cube": case_cube, "room": case_room, "faces": case_faces, "random": case_random, "order": case_order, "bounds": case_bounds,
         "nav": case_nav, "lifetime": case_lifetime, "reads_only": case_reads_only, "integrated": case_integrated, "errors": case_errors}

# name -> spec: the same cases in both tiers
SPECS = {}
for _vps in (8, 16, 32):
    for _case in ("cube", "room", "faces", "random", "order", "bounds", "nav"):
        SPECS["%s_vps%d" % (_case, _vps)] = dict(case=_case, vps=_vps)
SPECS.update({
    "planted_vps64": dict(case="planted", vps=64),
    "lifetime": dict(case="lifetime"),
    "reads_only_vps8": dict(case="reads_only", vps=8),
    "reads_only_vps16": dict(case="reads_only", vps=16),
    "integrated": dict(case="integrated"),
    "errors": dict(case="errors"),
})


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("FRONTIER_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
