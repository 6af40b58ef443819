"""The cases of block removal (ks_remove_blocks, ks_remove_distant_blocks), shared by both tiers: the GPU
tier (tests/test_remove_gpu.py) calls run_case in-process, the CPU tier (tests/test_remove_cpu.py) runs it as a child process on
the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.remove_case '<json spec>'
The yardstick is tests/remove_model.py for the removed set and the map, and EQUIVALENCE for everything else: a second, fresh
context that was only ever given the kept blocks through ks_upload_blocks must produce the same bytes."""
import ctypes
import json
import os
import sys

import numpy as np

from tests import esdf_case, mesh_case
from tests import remove_model as M

VOXEL = mesh_case.VOXEL          # 5 cm
ESDF_CFG = dict(min_distance_m=0.1, max_distance_m=0.4)   # R = 8 voxels, g = 1 tile
GROW = 1
RENDER_POSE = (-1.6, 0.2, 0.1)   # outside the sphere field, looking along +x at it


# ---- contexts and fields -------------------------------------------------------------------------------------------------------
def _ctx(method=0, vps=8, pipeline=0, max_tiles=512, size=(64, 48), **extra):
    return mesh_case._integrator(method, size[0], size[1], vps=vps, pipeline=pipeline, max_tiles=max_tiles, **extra)


def box_field(vps, seed=5, origin=(-2, -1, 0)):
    """Not geometric (esdf_case.random_field): 5 x 4 x 3 = 60 blocks of 8^3 voxels, or 3 x 2 x 2 = 12 blocks of 16^3 (96 tiles)."""
    n = (5, 4, 3) if vps == 8 else (3, 2, 2)
    idx = np.array([(origin[0] + x, origin[1] + y, origin[2] + z) for x in range(n[0]) for y in range(n[1]) for z in range(n[2])], np.int32)
    return esdf_case.random_field(idx, vps, seed)


def sphere_field(vps):
    """The sphere of radius 0.6 m over [-0.8 m, 0.8 m)^3: 64 tiles either way."""
    return esdf_case.sphere_blocks(vps, 4 if vps == 8 else 2)


def two_clusters(vps):
    """The sphere around the origin (tiles -2 .. 1) and one far cluster of random voxels at tiles 8 .. 9 along x: 7 tiles apart,
    further than 2 g + 2 = 4."""
    idx, t, s = sphere_field(vps)
    far = np.array([(8, y, z) for y in (0, 1) for z in (0, 1)], np.int32) if vps == 8 else np.array([(4, 0, 0)], np.int32)
    fi, ft, fs = esdf_case.random_field(far, vps, 9)
    return np.concatenate([idx, fi]), np.concatenate([t, ft]), np.concatenate([s, fs])


def tiles_of(g):
    k = g.tile_keys().astype(np.uint64)
    f = lambda sh: ((k >> np.uint64(sh)) & np.uint64(0x3ffff)).astype(np.int64) - (1 << 17)
    return np.stack([f(36), f(18), f(0)], axis=1)


def blocks_by_slot(g):
    """(nt, 3): the block of the tile at every slot."""
    return tiles_of(g) // (g.vps // 8)


def _rows(a):
    return [tuple(int(v) for v in r) for r in np.asarray(a).reshape(-1, 3)]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def refused(code, call):
    from kimera_semantics_amd import binding as B
    try:
        call()
    except B.KsError as e:
        assert e.code == code, e
        return e
    raise AssertionError("accepted")


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
def fresh_with(make, idx, t, s, removed):
    """A fresh context that is only ever given the kept blocks."""
    f = make()
    kidx, kt, ks = M.kept_of(idx, removed, t, s)
    if len(kidx):
        f.upload(kidx, kt, ks)
    return f


def g_capacity(g):
    """The pool's capacity as a removal that removes nothing reports it."""
    return g.remove_blocks(np.zeros((0, 3), np.int32))["pool_capacity_tiles"]


def remove_and_check(make, field, pick, what, by_distance=None, on_the_radius=False):
    """One context, one removal: pick(blocks_by_slot) -> the block list to pass (or by_distance = (centre, radius)).  on_the_radius: the
    case is ABOUT blocks whose d2 equals max_distance^2 bit for bit, so the float32 rule alone decides."""
    g = make()
    g.upload(*field)
    before = g.download()
    slots = blocks_by_slot(g)
    cap = g_capacity(g)
    if by_distance is None:
        listed = np.asarray(pick(slots), np.int32).reshape(-1, 3)
        removed = M.removed_of_list(before[0], listed)
        stats = g.remove_blocks(listed)
    else:
        centre, radius = by_distance
        if not on_the_radius:
            M.assert_away_from_threshold(before[0], centre, radius, VOXEL, g.vps)
        removed = M.removed_of_distance(before[0], centre, radius, VOXEL, g.vps)
        stats = g.remove_distant(centre, radius)
    f = fresh_with(make, *before, removed)
    assert _same(g.removed_blocks(), removed), (what, g.removed_blocks(), removed)
    assert stats["pool_capacity_tiles"] == cap, (what, stats, cap)
    idx, t, s = before
    kidx = M.kept_of(idx, removed)[0]
    assert _same(g.block_indices(), kidx), what
    check_map(g, f, before, removed, what)
    keep_slot = np.array([b not in set(_rows(removed)) for b in _rows(slots)], bool)
    nt2, moves = M.moves_needed(keep_slot)
    assert stats["blocks_removed"] == len(removed) and stats["tiles_removed"] == len(keep_slot) - nt2, (what, stats)
    assert stats["tiles_resident"] == nt2 == len(g.tile_keys()) and stats["tiles_moved"] == moves, (what, stats, moves)
    return g, f, before, removed, stats


def check_map(g, f, before, removed, what, uploaded=True):
    idx, t, s = before
    _, gt, gs = g.download(idx)
    _, ft, fs = f.download(idx)
    assert gt.tobytes() == ft.tobytes() and gs.tobytes() == fs.tobytes(), what
    gone = set(_rows(removed))
    keep = np.array([r not in gone for r in _rows(idx)], bool)
    assert gt[keep].tobytes() == t[keep].tobytes() and gs[keep].tobytes() == s[keep].tobytes(), what
    if (~keep).any():
        empty = _ctx(vps=g.vps, max_tiles=64)
        _, et, es = empty.download(idx[~keep])
        empty.close()
        assert gt[~keep].tobytes() == et.tobytes() and gs[~keep].tobytes() == es.tobytes(), what
        assert (et["weight"] == 0).all() and (gt[~keep]["weight"] == 0).all()
    assert _same(g.block_indices(), M.kept_of(idx, removed)[0]), what
    if uploaded:
        assert sorted(g.tile_keys().tolist()) == sorted(f.tile_keys().tolist()), what


# ---- slot patterns -------------------------------------------------------------------------------------------------------------
def _unique_blocks(rows):
    seen, out = set(), []
    for r in _rows(rows):
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


PATTERNS = {
    "nothing": lambda slots: [],
    "everything": lambda slots: _unique_blocks(slots),
    "lowest_slots": lambda slots: _unique_blocks(slots[:16]),
    "highest_slots": lambda slots: _unique_blocks(slots[-16:]),
    "alternating": lambda slots: _unique_blocks(slots)[::2],
    "more_removed_than_kept": lambda slots: [b for i, b in enumerate(_unique_blocks(slots)) if i not in (1, len(_unique_blocks(slots)) // 2, len(_unique_blocks(slots)) - 1)][::-1],
    "single_tile": lambda slots: _unique_blocks(slots[7:8]),
    "absent_block": lambda slots: [(99, 99, 99)] + _unique_blocks(slots[3:9]) + [(-50, 0, 7)],
    "listed_twice": lambda slots: _unique_blocks(slots[10:20]) + _unique_blocks(slots[12:14]) + _unique_blocks(slots[10:11]),
}


def case_pattern(spec):
    vps = spec["vps"]
    make = lambda: _ctx(vps=vps)
    out = {}
    for name in spec["patterns"]:
        g, f, before, removed, stats = remove_and_check(make, box_field(vps), PATTERNS[name], name)
        n_blocks = len(before[0])
        if name == "nothing":
            assert stats["blocks_removed"] == stats["tiles_moved"] == 0 and len(g.block_indices()) == n_blocks
        if name == "everything":
            assert stats["tiles_resident"] == 0 and len(g.block_indices()) == 0 and len(g.tile_keys()) == 0
        if name == "highest_slots":
            assert stats["tiles_moved"] == 0 and stats["tiles_removed"] > 0, stats   # nothing above the new count survives
        if name == "lowest_slots":
            assert stats["tiles_moved"] > 0, stats
        if name == "more_removed_than_kept":
            assert stats["tiles_removed"] > stats["tiles_resident"] and 0 < stats["tiles_moved"] < stats["tiles_removed"], stats
        if name == "single_tile" and vps == 8:
            assert stats["tiles_removed"] == 1 and stats["tiles_moved"] == 1, stats
        if name == "absent_block":
            assert stats["blocks_removed"] == len(removed) > 0 and (99, 99, 99) not in _rows(g.removed_blocks())
        if name == "listed_twice":
            assert stats["blocks_removed"] == len(removed) == len(set(_rows(removed)))
        out[name] = stats
        g.close()
        f.close()
    return out


def case_scattered(spec):
    """vps 16 on an INTEGRATED map: the rays allocate a block's tiles one by one, so blocks hold fewer than 8 tiles and their tiles sit
    in scattered slots.  Blocks whose tiles are no contiguous run of slots are removed; every tile of each goes."""
    w, h = 64, 48
    make = lambda: _ctx(method=1, vps=16, max_tiles=2048, size=(w, h))
    g = make()
    f1 = mesh_case._frames(1, w, h)[0]
    g.integrate(f1.T_G_C, f1.xyz, f1.rgba, f1.labels)
    before = g.download()
    slots, keys_before = blocks_by_slot(g), g.tile_keys()
    by_block = {}
    for s_, b in enumerate(_rows(slots)):
        by_block.setdefault(b, []).append(s_)
    scattered = sorted(b for b, v in by_block.items() if len(v) > 1 and max(v) - min(v) >= len(v))
    assert len(scattered) >= 3, len(scattered)
    victims = np.array(scattered[::2][:6], np.int32)
    n_tiles = sum(len(by_block[b]) for b in _rows(victims))
    assert any(len(by_block[b]) < 8 for b in _rows(victims))
    st = g.remove_blocks(victims)
    assert st["blocks_removed"] == len(victims) and st["tiles_removed"] == n_tiles and st["tiles_resident"] == len(slots) - n_tiles, st
    assert _same(g.removed_blocks(), victims)
    keep_slot = np.array([b not in set(_rows(victims)) for b in _rows(slots)], bool)
    assert st["tiles_moved"] == M.moves_needed(keep_slot)[1]
    f = fresh_with(make, *before, victims)
    check_map(g, f, before, victims, "scattered blocks", uploaded=False)
    # the tiles that stayed are the tiles that were there (the fresh context holds whole blocks: compare with the directory before)
    assert sorted(g.tile_keys().tolist()) == sorted(keys_before[keep_slot].tolist())
    g.close()
    f.close()
    return dict(st, scattered=len(scattered))


def case_distance(spec):
    """The distance entry on an uploaded field: the float32 rule against the device, away from the threshold."""
    vps = spec["vps"]
    make = lambda: _ctx(vps=vps)
    out = {}
    for centre, radius in spec["queries"]:
        g, f, before, removed, stats = remove_and_check(make, box_field(vps), None, "distance %r %r" % (centre, radius), by_distance=(centre, radius))
        out["%r/%r" % (centre, radius)] = stats
        g.close()
        f.close()
    kinds = [v["blocks_removed"] for v in out.values()]
    assert min(kinds) == 0 and max(kinds) > 0, kinds        # (one query removes nothing, the others something)
    return out


def case_distance_on_the_radius(spec):
    """Blocks whose origin lies on the radius exactly stay (the rule is d2 > r^2): the centre at the origin and r = 2 block sizes in
    float32, so that d2 and r^2 of the blocks (+-2, 0, 0), (0, +-2, 0), (0, 0, 2) are the same float32 product.  The block size is
    voxel_size * vps: with any other factor these blocks fall on one side of the radius."""
    vps = spec["vps"]
    blocks = [(-2, 0, 0), (0, 0, 0), (2, 0, 0), (3, 0, 0)]
    if vps < 64:
        blocks += [(-3, 0, 0), (-1, 0, 0), (1, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (2, 1, 0), (0, -3, 0), (1, 1, 1)]
    idx = np.array(sorted(blocks), np.int32)
    tiles = len(idx) * (vps // 8) ** 3
    make = lambda: _ctx(vps=vps, max_tiles=max(512, 2 * tiles))
    radius = float(np.float32(2) * (np.float32(VOXEL) * np.float32(vps)))
    far = M.distant_f32(idx, [0, 0, 0], radius, VOXEL, vps)
    on = np.abs(M.distance_f64(idx, [0, 0, 0], VOXEL, vps) - radius) == 0
    assert on.sum() == (2 if vps == 64 else 5) and not far[on].any() and far.sum() == (1 if vps == 64 else 4), (on, far)
    g, f, before, removed, stats = remove_and_check(make, esdf_case.random_field(idx, vps, 5), None, "on the radius", by_distance=([0, 0, 0], radius),
                                                    on_the_radius=True)
    assert _same(removed, idx[far]) and stats["blocks_removed"] == far.sum() and stats["tiles_removed"] == far.sum() * (vps // 8) ** 3, stats
    g.close()
    f.close()
    return dict(stats)


# ---- flags and syncs -------------------------------------------------------------------------------------------------------------
def _sorted_voxels(v):
    order = np.lexsort((v["linear"], v["block"][:, 2], v["block"][:, 1], v["block"][:, 0]))
    return v[order]


def case_flags(spec):
    """`updated` (block sync and voxel sync) and `dirty` travel with their tiles: two contexts integrate the same frame; one of them
    removes blocks, and reports afterwards exactly what the other reports for the blocks that stayed."""
    w, h = 64, 48
    f1 = mesh_case._frames(1, w, h)[0]
    a, b = (_ctx(method=1, vps=16, max_tiles=2048, size=(w, h)) for _ in range(2))
    for g in (a, b):
        g.integrate(f1.T_G_C, f1.xyz, f1.rgba, f1.labels)
    idx = a.block_indices()
    removed = idx[::3]
    ua = a.updated_block_indices(reset=False)
    assert len(ua) == len(idx) > 6
    st = b.remove_blocks(removed)
    assert st["blocks_removed"] == len(removed) and st["tiles_moved"] > 0, st
    ub = b.updated_block_indices(reset=False)
    assert _same(ub, M.kept_of(ua, removed)[0])
    va, vb = a.download_updated_voxels(), b.download_updated_voxels()
    gone = set(_rows(removed))
    keep = np.array([r not in gone for r in _rows(va["block"])], bool)
    assert 0 < keep.sum() < len(va) and len(vb) == keep.sum(), (len(va), len(vb), keep.sum())
    assert _sorted_voxels(va[keep]).tobytes() == _sorted_voxels(vb).tobytes()
    assert len(b.download_updated_voxels()) == 0 and len(b.updated_block_indices()) == 0    # consumed, as without a removal
    a.close()
    b.close()
    return dict(st, voxels=int(len(vb)))


# ---- removal followed by growth and re-insertion -------------------------------------------------------------------------------------
def case_grow(spec):
    """Enough uploads after a removal to force grow_pool (a rehash after the compaction), and the re-upload of a removed block."""
    vps = 8
    g = _ctx(vps=vps, max_tiles=96)
    idx, t, s = box_field(vps)                       # 60 tiles: the pool has already doubled once or twice
    g.upload(idx, t, s)
    cap0 = g_capacity(g)
    removed = idx[1::2]
    assert len(g.updated_block_indices(reset=True)) == len(idx)        # (tiles that join a map count as updated: consumed here)
    st = g.remove_blocks(removed)
    assert st["pool_capacity_tiles"] == cap0 and st["tiles_resident"] == 30, st
    assert len(g.updated_block_indices(reset=False)) == 0
    # a removed block comes back with other contents: it reads as uploaded, not as it was
    back = removed[:3]
    _, nt_, ns_ = esdf_case.random_field(back, vps, 77)
    g.upload(back, nt_, ns_)
    _, gt, gs = g.download(back)
    assert gt.tobytes() == nt_.tobytes() and gs.tobytes() == ns_.tobytes()
    assert _same(g.updated_block_indices(reset=False), np.array(sorted(_rows(back)), np.int32))   # the fresh tiles, and nothing a freed slot left behind
    # more blocks than the pool's free half: it grows, the directory is rebuilt once more
    more = np.array([(20 + x, y, z) for x in range(6) for y in range(6) for z in range(6)], np.int32)
    mi, mt, ms = esdf_case.random_field(more, vps, 78)
    g.upload(mi, mt, ms)
    assert g_capacity(g) > cap0
    kidx, kt, ks = M.kept_of(idx, removed, t, s)
    for bi, bt, bs, what in ((kidx, kt, ks, "kept"), (back, nt_, ns_, "re-uploaded"), (mi, mt, ms, "new")):
        _, gt, gs = g.download(bi)
        assert gt.tobytes() == bt.tobytes() and gs.tobytes() == bs.tobytes(), what
    assert len(g.block_indices()) == len(kidx) + len(back) + len(more) == len(g.tile_keys())
    g.close()
    return dict(st)


def _sum_stats(stats):
    keys = ("n_points", "n_valid_points", "n_rays_cast", "n_voxel_updates", "n_blocks_allocated")
    return {k: sum(int(getattr(s, k)) for s in stats) for k in keys}


def case_integrate(spec):
    """A frame integrated after a removal, bit for bit against a fresh context that holds the kept blocks uploaded and integrates
    the same frame.  `merged` keeps no cross-frame state, so the two must agree.  pipeline > 0: the frames before the removal are
    still in flight when it is called, and their statistics still arrive."""
    w, h = 64, 48
    pipeline = spec.get("pipeline", 0)
    f1, f2, f3 = mesh_case._frames(3, w, h, step=12)
    make = lambda p=0: _ctx(method=1, vps=16, pipeline=p, max_tiles=2048, size=(w, h))
    # the plain context: what the frames before the removal leave, and their statistics
    plain = make()
    want_stats = [plain.integrate(f.T_G_C, f.xyz, f.rgba, f.labels) for f in (f1, f2)]
    before = plain.download()
    centre, radius = [float(v) for v in f2.T_G_C[4:7]], spec.get("radius", 2.0)
    radius = _clear_radius(before[0], centre, radius, 16)
    removed = M.removed_of_distance(before[0], centre, radius, VOXEL, 16)
    assert 0 < len(removed) < len(before[0]), (len(removed), len(before[0]))
    # the context under test
    g = make(pipeline)
    got_stats = [g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels) for f in (f1, f2)]
    if pipeline:
        assert g.pipeline_shape()["lag"] > 0 and _sum_stats(got_stats)["n_voxel_updates"] < _sum_stats(want_stats)["n_voxel_updates"]   # frames in flight
    st = g.remove_distant(centre, radius)
    assert _same(g.removed_blocks(), removed) and st["blocks_removed"] == len(removed), st
    got_stats.append(g.integrate(f3.T_G_C, f3.xyz, f3.rgba, f3.labels))
    got_stats.append(g.flush())
    # the yardstick: kept blocks uploaded, then the same frame
    f = fresh_with(make, *before, removed)
    s3 = f.integrate(f3.T_G_C, f3.xyz, f3.rgba, f3.labels)
    union = np.array(sorted(set(_rows(g.block_indices())) | set(_rows(before[0]))), np.int32)
    assert _same(g.block_indices(), f.block_indices())
    _, gt, gs = g.download(union)
    _, ft, fs = f.download(union)
    assert gt.tobytes() == ft.tobytes() and gs.tobytes() == fs.tobytes()
    # the owed statistics of the frames completed by the removal still arrive; frame 3 allocates the removed tiles it touches afresh
    total = _sum_stats(got_stats)
    want = _sum_stats(want_stats + [s3])
    for k in ("n_points", "n_valid_points", "n_rays_cast", "n_voxel_updates"):
        assert total[k] == want[k], (k, total, want)
    again = set(_rows(removed)) & set(_rows(g.block_indices()))
    assert again, "frame 3 touches none of the removed blocks"
    assert int(s3.n_blocks_allocated) > 0
    if not pipeline:
        assert int(got_stats[2].n_voxel_updates) == int(s3.n_voxel_updates) and int(got_stats[2].n_blocks_allocated) > 0
    for c in (plain, g, f):
        c.close()
    return dict(st, readded=len(again))


def _clear_radius(blocks, centre, radius, vps):
    """The radius nudged until no block origin lies within 2 mm of it (the cases must not depend on a borderline block)."""
    d = M.distance_f64(blocks, centre, VOXEL, vps)
    for k in range(200):
        r = radius + 0.004 * k
        if np.abs(d - float(np.float32(r))).min() > 2e-3:
            M.assert_away_from_threshold(blocks, centre, r, VOXEL, vps)
            return r
    raise AssertionError("no clear radius")


# ---- products ------------------------------------------------------------------------------------------------------------------
def _mesh_same(a, b, what):
    for k in ("blocks", "xyz", "normals", "rgba", "labels"):
        assert _same(getattr(a, k), getattr(b, k)), (what, k)
    assert a.stats["triangles_total"] == b.stats["triangles_total"] and a.stats["blocks_total"] == b.stats["blocks_total"], what


def _corner(idx):
    """The blocks of the field's upper x / y corner."""
    idx = np.asarray(idx)
    return idx[(idx[:, 0] == idx[:, 0].max()) & (idx[:, 1] >= idx[:, 1].max() - 1)]


def case_mesh(spec):
    vps = spec["vps"]
    make = lambda: _ctx(vps=vps)
    g = make()
    field = sphere_field(vps)
    g.upload(*field)
    m0 = g.mesh()
    assert m0.n_triangles > 500
    removed = _corner(field[0]) if vps == 8 else np.array([(0, -1, -1)], np.int32)     # (of 2 x 2 x 2 blocks: one with a single lower neighbour)
    st = g.remove_blocks(removed)
    stored = _mesh_size(g)
    assert stored == (len(m0.blocks), len(m0.xyz))        # until the next update the stored mesh is the one of the last update
    m1 = g.mesh(only_stale=True)
    f = fresh_with(make, *field, removed)
    full = f.mesh()
    _mesh_same(m1, full, "only_stale after a removal")
    changed = set(_rows(g.mesh_changed_blocks()))
    want = set(M.mesh_blocks_to_remesh(M.kept_of(field[0], removed)[0], removed))
    assert set(_rows(removed)) <= changed and changed == want | set(_rows(removed)), (sorted(changed ^ (want | set(_rows(removed))))[:5])
    assert m1.stats["blocks_meshed"] == len(want) < m1.stats["blocks_total"] == len(field[0]) - len(removed), m1.stats
    assert not (set(_rows(m1.blocks["block"])) & set(_rows(removed)))
    # nothing happened since: nothing to do
    m2 = g.mesh(only_stale=True)
    assert m2.stats["blocks_meshed"] == 0 and len(g.mesh_changed_blocks()) == 0
    _mesh_same(m2, full, "idle refresh")
    # a removed block comes back: the refresh picks it up again
    back = removed[:1]
    bi, bt, bs = M.kept_of(field[0], M.kept_of(field[0], back)[0], field[1], field[2])
    for c in (g, f):
        c.upload(bi, bt, bs)
    _mesh_same(g.mesh(only_stale=True), f.mesh(), "after the re-upload")
    # everything leaves: an empty mesh
    g.remove_blocks(g.block_indices())
    m3 = g.mesh(only_stale=True)
    assert m3.n_triangles == 0 and len(m3.blocks) == 0 and m3.stats["blocks_total"] == 0
    g.close()
    f.close()
    return dict(st, meshed=m1.stats["blocks_meshed"], total=m1.stats["blocks_total"])


def _mesh_size(g):
    from kimera_semantics_amd import binding as B
    nb, nv = ctypes.c_size_t(), ctypes.c_size_t()
    g._chk(B.lib().ks_mesh_size(g._h, ctypes.byref(nb), ctypes.byref(nv)))
    return nb.value, nv.value


def case_esdf(spec):
    vps = spec["vps"]
    make = lambda: _ctx(vps=vps)
    g = make()
    field = sphere_field(vps)
    g.upload(*field)
    g.esdf_update(**ESDF_CFG)
    removed = _corner(field[0]) if vps == 8 else field[0][-1:]
    st = g.remove_blocks(removed)
    r = g.esdf_refresh()
    f = fresh_with(make, *field, removed)
    fs = f.esdf_update(**ESDF_CFG)
    idx = field[0]
    assert g.esdf_blocks(idx).tobytes() == f.esdf_blocks(idx).tobytes()
    for k in ("voxels_observed", "voxels_fixed", "voxels_clamped"):
        assert r[k] == fs[k], (k, r, fs)
    tpb = vps // 8
    o = np.array([(x, y, z) for x in range(tpb) for y in range(tpb) for z in range(tpb)], np.int64)
    tiles = lambda blocks: (np.asarray(blocks, np.int64).reshape(-1, 1, 3) * tpb + o[None]).reshape(-1, 3)
    want = M.esdf_tiles_to_recompute(tiles(M.kept_of(idx, removed)[0]), tiles(removed), GROW)
    assert r["tiles_stale"] == 0 and r["tiles_recomputed"] == len(want) < r["tiles_total"] == len(g.tile_keys()), (r, len(want))
    assert (g.esdf_blocks(removed)["flags"] == 0).all()
    # nothing happened since
    r2 = g.esdf_refresh()
    assert r2["tiles_recomputed"] == 0 and all(r2[k] == r[k] for k in ("voxels_observed", "voxels_fixed", "voxels_clamped")), r2
    # a tile that joined after the update moves into a slot inside the store: it has no records until the refresh
    extra = np.array([(idx[:, 0].min() - 1, 0, 0)], np.int32)
    ei, et, es = esdf_case.random_field(extra, vps, 31)
    for c in (g, f):
        c.upload(ei, et, es)
    low = blocks_by_slot(g)[:2]
    g.remove_blocks(low)
    f2 = fresh_with(make, *f.download(), low)
    assert (g.esdf_blocks(ei)["flags"] == 0).all()
    r3 = g.esdf_refresh()
    fs2 = f2.esdf_update(**ESDF_CFG)
    allidx = np.concatenate([idx, ei])
    assert g.esdf_blocks(allidx).tobytes() == f2.esdf_blocks(allidx).tobytes()
    assert all(r3[k] == fs2[k] for k in ("voxels_observed", "voxels_fixed", "voxels_clamped")), (r3, fs2)
    # everything leaves
    g.remove_blocks(g.block_indices())
    r4 = g.esdf_refresh()
    assert r4["tiles_total"] == 0 and r4["voxels_observed"] == 0, r4
    for c in (g, f, f2):
        c.close()
    return dict(st, recomputed=r["tiles_recomputed"], total=r["tiles_total"])


def case_objects(spec):
    vps = spec["vps"]
    make = lambda: _ctx(vps=vps)
    g = make()
    field = box_field(vps)
    g.upload(*field)
    cfg = dict(min_voxels=1)
    rec, stats = g.objects(**cfg)
    idx = field[0]
    ids = g.object_ids(idx)
    assert stats["objects"] > 10 and (ids != 0xffffffff).sum() > 100
    removed = M.removed_of_list(idx, PATTERNS["alternating"](blocks_by_slot(g)))
    st = g.remove_blocks(removed)
    assert st["tiles_moved"] > 0
    # the records are the snapshot of the last update; ids travel with their tiles; removed blocks read none
    assert g.object_records().tobytes() == rec.tobytes()
    ids2 = g.object_ids(idx)
    gone = set(_rows(removed))
    keep = np.array([r not in gone for r in _rows(idx)], bool)
    assert ids2[keep].tobytes() == ids[keep].tobytes() and (ids2[~keep] == 0xffffffff).all() and (ids[~keep] != 0xffffffff).any()
    centres = ((idx.astype(np.float64) * vps + 3.5) * VOXEL).astype(np.float32)
    q = g.object_query(centres)
    lin = 3 + vps * (3 + vps * 3)
    assert (q[~keep] == 0xffffffff).all() and (q[keep] == ids[keep][:, lin]).all()
    # a tile that joins afterwards reads none, wherever its slot is
    extra = np.array([(40, 0, 0)], np.int32)
    g.upload(*esdf_case.random_field(extra, vps, 3))
    assert (g.object_ids(extra) == 0xffffffff).all()
    g.remove_blocks(extra)
    # a new update equals the one of a fresh context
    f = fresh_with(make, *field, removed)
    ra, sa = g.objects(**cfg)
    rb, sb = f.objects(**cfg)
    assert ra.tobytes() == rb.tobytes() and sa == sb and g.object_ids(idx).tobytes() == f.object_ids(idx).tobytes()
    g.close()
    f.close()
    return dict(st, objects=sa["objects"])


def case_render_align(spec):
    from kimera_semantics_amd import synth
    vps = spec["vps"]
    make = lambda: _ctx(vps=vps)
    g = make()
    field = sphere_field(vps)
    g.upload(*field)
    T = synth.pose_to_T(RENDER_POSE, 0.0)
    K = (40.0, 40.0, 31.5, 23.5)
    v0 = g.render(T, K, 64, 48, max_range_m=4.0)
    assert v0[4]["pixels_hit"] > 500
    idx = field[0]
    removed = idx[idx[:, 1] >= 0][::2] if vps == 8 else idx[idx[:, 1] >= 0][:2]       # part of the half the camera's left side sees
    st = g.remove_blocks(removed)
    f = fresh_with(make, *field, removed)
    va, vb = g.render(T, K, 64, 48, max_range_m=4.0), f.render(T, K, 64, 48, max_range_m=4.0)
    for k in range(4):
        assert va[k].tobytes() == vb[k].tobytes(), k
    assert va[4] == vb[4] and va[4]["pixels_hit"] < v0[4]["pixels_hit"], (va[4], v0[4])    # the renderer sees nothing there
    # the points of the first view, aligned from a pose a little off
    depth = v0[0]
    cloud = synth.backproject(depth, K).reshape(-1, 3)
    cloud = cloud[np.isfinite(cloud).all(axis=1)]
    from tests import align_case
    T0 = align_case.perturbed(T, dt=(0.01, -0.01, 0.01), deg=0.5)
    pa, sa = g.align(T0, cloud, min_inliers=16)
    pb, sb = f.align(T0, cloud, min_inliers=16)
    assert pa.tobytes() == pb.tobytes() and sa == sb and sa["inliers_first"] > 100, (sa, sb)
    g.close()
    f.close()
    return dict(st, hit_before=v0[4]["pixels_hit"], hit_after=va[4]["pixels_hit"])


def case_locality(spec):
    """Two clusters further apart than 2 g + 2 tiles; one of them is removed in part: the refreshes touch that cluster only."""
    vps = spec["vps"]
    tpb = vps // 8
    make = lambda: _ctx(vps=vps)
    field = two_clusters(vps)
    idx = field[0]
    near = idx[idx[:, 0] * tpb < 4]
    removed = near[near[:, 0] == near[:, 0].max()]       # its +x face: the blocks behind it read it across their border
    kept = M.kept_of(idx, removed)[0]
    o = np.array([(x, y, z) for x in range(tpb) for y in range(tpb) for z in range(tpb)], np.int64)
    tiles = lambda blocks: (np.asarray(blocks, np.int64).reshape(-1, 1, 3) * tpb + o[None]).reshape(-1, 3)
    # the model's own lists first: the inequalities are satisfiable for this field, and the far cluster is out of reach
    gap = int(tiles(idx[idx[:, 0] * tpb >= 4])[:, 0].min() - tiles(near)[:, 0].max())
    assert gap > 2 * GROW + 2, gap
    remesh = M.mesh_blocks_to_remesh(kept, removed)
    recompute = M.esdf_tiles_to_recompute(tiles(kept), tiles(removed), GROW)
    assert 0 < len(remesh) < len(kept) and 0 < len(recompute) < len(tiles(kept)), (len(remesh), len(recompute))
    assert all(b[0] * tpb < 4 for b in remesh) and (recompute[:, 0] < 4).all()
    g = make()
    g.upload(*field)
    g.mesh()
    g.esdf_update(**ESDF_CFG)
    st = g.remove_blocks(removed)
    m = g.mesh(only_stale=True)
    r = g.esdf_refresh()
    assert m.stats["blocks_meshed"] == len(remesh) < m.stats["blocks_total"] == len(kept), m.stats
    assert r["tiles_recomputed"] == len(recompute) < r["tiles_total"] == len(tiles(kept)), r
    f = fresh_with(make, *field, removed)
    _mesh_same(m, f.mesh(), "locality")
    f.esdf_update(**ESDF_CFG)
    assert g.esdf_blocks(idx).tobytes() == f.esdf_blocks(idx).tobytes()
    g.close()
    f.close()
    return dict(st, meshed=m.stats["blocks_meshed"], blocks=m.stats["blocks_total"], recomputed=r["tiles_recomputed"], tiles=r["tiles_total"])


# ---- sliding window --------------------------------------------------------------------------------------------------------------
SLIDING = dict(max_tiles=256, frames=14, radius=1.6, ray=1.2, size=(32, 24))


def _sliding_frames():
    """A straight walk of 1 m steps along x through the hall, looking ahead; rays are cut at SLIDING['ray'] metres."""
    from kimera_semantics_amd import synth
    sc = synth.make_scene("hall")
    w, h = SLIDING["size"]
    return [synth.render_frame(sc, synth.pose_to_T((-6.5 + 1.0 * k, 0.0, 1.5), 0.0), w, h, hfov_deg=90.0, seed=90 + k) for k in range(SLIDING["frames"])]


def case_sliding(spec):
    """`fast` with a small pool: pruning around the sensor after every frame keeps the pool at its initial capacity, while the same
    frames without it make it grow."""
    w, h = SLIDING["size"]
    make = lambda: _ctx(method=0, vps=16, max_tiles=SLIDING["max_tiles"], size=(w, h), max_ray_length_m=SLIDING["ray"])
    frames = _sliding_frames()
    g, plain = make(), make()
    cap0 = g_capacity(g)
    assert cap0 == SLIDING["max_tiles"]
    resident, touched = [], set()
    for f in frames:
        plain.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        touched |= set(g.tile_keys().tolist())
        centre = [float(v) for v in f.T_G_C[4:7]]
        st = g.remove_distant(centre, SLIDING["radius"])
        assert st["pool_capacity_tiles"] == cap0, st
        resident.append(st["tiles_resident"])
        # what stayed lies within the radius, what left beyond it (block origins, in f64: the fields are far from the threshold or not judged)
        d = M.distance_f64(g.block_indices(), centre, VOXEL, 16)
        assert (d <= SLIDING["radius"] + 1e-3).all()
    assert len(touched) > 2 * cap0, (len(touched), cap0)                   # the walk needs more than twice the pool
    assert max(resident) * 2 <= cap0, resident                              # ... and never more than half of it at a time
    cap_plain = g_capacity(plain)
    assert cap_plain > cap0 and len(plain.tile_keys()) > cap0, (cap_plain, len(plain.tile_keys()))
    # the window's map equals what the unpruned map holds for those blocks wherever no removed block was touched again
    out = dict(capacity=cap0, capacity_without=cap_plain, touched=len(touched), resident=resident)
    g.close()
    plain.close()
    return out


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def case_errors(spec):
    from kimera_semantics_amd import binding as B
    L = B.lib()
    g = _ctx(vps=16)
    field = box_field(16)
    g.upload(*field)
    idx = field[0]
    one = np.ascontiguousarray(idx[:1])
    ctr = np.zeros(3, np.float32)
    st = B.KsRemoveStats()
    n = ctypes.c_size_t()
    assert L.ks_remove_blocks(None, one.ctypes.data, 1, None) == B.KS_ERR_INVALID_ARG
    assert L.ks_remove_blocks(g._h, None, 1, None) == B.KS_ERR_INVALID_ARG
    assert L.ks_remove_distant_blocks(None, ctr.ctypes.data, 1.0, None) == B.KS_ERR_INVALID_ARG
    assert L.ks_remove_distant_blocks(g._h, None, 1.0, None) == B.KS_ERR_INVALID_ARG
    assert L.ks_removed_blocks(None, None, 0, ctypes.byref(n)) == B.KS_ERR_INVALID_ARG
    assert L.ks_removed_blocks(g._h, None, 0, None) == B.KS_ERR_INVALID_ARG
    for bad in ([float("nan"), 0, 0], [0, float("inf"), 0], [0, 0, -float("inf")]):
        refused(B.KS_ERR_INVALID_ARG, lambda: g.remove_distant(bad, 1.0))
    for bad in (-1.0, -1e-30, float("nan"), float("inf")):
        refused(B.KS_ERR_INVALID_ARG, lambda: g.remove_distant([0, 0, 0], bad))
    lim = (1 << 17) // 2
    for bad in ([[lim, 0, 0]], [[0, -lim - 1, 0]], [list(idx[0]), [0, 0, 1 << 30]]):
        refused(B.KS_ERR_INDEX_RANGE, lambda: g.remove_blocks(np.array(bad, np.int32)))
    # ... and none of these changed the map
    assert _same(g.block_indices(), idx)
    _, t, s = g.download(idx)
    assert t.tobytes() == field[1].tobytes() and s.tobytes() == field[2].tobytes()
    # n = 0 removes nothing (a NULL list is fine then); stats may be NULL
    assert L.ks_remove_blocks(g._h, None, 0, ctypes.byref(st)) == 0 and st.blocks_removed == 0 and st.tiles_resident == len(idx) * 8
    assert len(g.removed_blocks()) == 0
    assert L.ks_remove_blocks(g._h, one.ctypes.data, 1, None) == 0
    assert _rows(g.removed_blocks()) == _rows(one)
    # ks_removed_blocks after each kind of call; a capacity that is too small
    far = g.remove_distant([0.0, 0.0, 0.0], 1.3)
    want = M.removed_of_distance(idx[1:], [0.0, 0.0, 0.0], 1.3, VOXEL, 16)
    M.assert_away_from_threshold(idx[1:], [0.0, 0.0, 0.0], 1.3, VOXEL, 16)
    assert far["blocks_removed"] == len(want) >= 2 and _same(g.removed_blocks(), want)
    out = np.zeros((len(want), 3), np.int32)
    n.value = 0
    assert L.ks_removed_blocks(g._h, out.ctypes.data, len(want) - 1, ctypes.byref(n)) == B.KS_ERR_INVALID_ARG and n.value == len(want)
    assert L.ks_removed_blocks(g._h, out.ctypes.data, len(want), ctypes.byref(n)) == 0 and _same(out, want)
    assert L.ks_remove_distant_blocks(g._h, ctr.ctypes.data, 100.0, None) == 0 and len(g.removed_blocks()) == 0    # the LAST call's
    # max_distance_m = 0 is allowed: every block whose origin is not the centre itself goes
    z = g.remove_distant([0.0, 0.0, 0.0], 0.0)
    assert _rows(g.block_indices()) in ([], [(0, 0, 0)]) and z["tiles_resident"] == len(g.tile_keys())
    g.close()
    # a marcher context of the exact multi-GPU mode holds no voxel data
    marcher, owner = (mesh_case._integrator(1, 64, 48) for _ in range(2))
    f = mesh_case._frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    refused(B.KS_ERR_UNSUPPORTED, lambda: marcher.remove_blocks(one))
    refused(B.KS_ERR_UNSUPPORTED, lambda: marcher.remove_distant([0, 0, 0], 1.0))
    nb = len(owner.block_indices())
    assert owner.remove_distant([float(v) for v in f.T_G_C[4:7]], 1.0)["blocks_removed"] > 0 and len(owner.block_indices()) < nb   # (the owner holds the map)
    marcher.close()
    owner.close()
    return {}


CASES = {"pattern": case_pattern, "scattered": case_scattered, "distance": case_distance, "distance_on_the_radius": case_distance_on_the_radius, "flags": case_flags, "grow": case_grow,
         "integrate": case_integrate, "mesh": case_mesh, "esdf": case_esdf, "objects": case_objects, "render_align": case_render_align,
         "locality": case_locality, "sliding": case_sliding, "errors": case_errors}

# name -> spec: the same cases in both tiers
SPECS = {
    "patterns_a_vps8": dict(case="pattern", vps=8, patterns=["nothing", "everything", "lowest_slots", "highest_slots", "single_tile"]),
    "patterns_b_vps8": dict(case="pattern", vps=8, patterns=["alternating", "more_removed_than_kept", "absent_block", "listed_twice"]),
    "patterns_vps16": dict(case="pattern", vps=16, patterns=["everything", "lowest_slots", "alternating", "more_removed_than_kept", "listed_twice"]),
    "scattered_block_vps16": dict(case="scattered"),
    "distance_vps8": dict(case="distance", vps=8, queries=[[[0.1, 0.1, 0.3], 5.0], [[0.1, 0.1, 0.3], 0.71], [[-0.9, 0.4, 0.0], 0.33]]),
    "distance_vps16": dict(case="distance", vps=16, queries=[[[0.1, 0.1, 0.3], 5.0], [[0.3, 0.2, 0.1], 0.93]]),
    "distance_vps32": dict(case="distance", vps=32, queries=[[[0.1, 0.1, 0.3], 9.0], [[0.3, 0.2, 0.1], 1.93]]),
    "distance_on_the_radius_vps32": dict(case="distance_on_the_radius", vps=32),
    "distance_on_the_radius_vps64": dict(case="distance_on_the_radius", vps=64),
    "flags_travel": dict(case="flags"),
    "grow_and_reupload": dict(case="grow"),
    "integrate_merged": dict(case="integrate"),
    "integrate_pipelined_owed_stats": dict(case="integrate", pipeline=2),
    "mesh_vps8": dict(case="mesh", vps=8),
    "mesh_vps16": dict(case="mesh", vps=16),
    "esdf_vps8": dict(case="esdf", vps=8),
    "esdf_vps16": dict(case="esdf", vps=16),
    "objects_vps8": dict(case="objects", vps=8),
    "objects_vps16": dict(case="objects", vps=16),
    "render_align_vps8": dict(case="render_align", vps=8),
    "render_align_vps16": dict(case="render_align", vps=16),
    "locality_vps8": dict(case="locality", vps=8),
    "locality_vps16": dict(case="locality", vps=16),
    "sliding_window": dict(case="sliding"),
    "errors": dict(case="errors"),
}


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("REMOVE_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
