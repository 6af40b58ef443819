"""The cases of the incremental ESDF refresh (ks_esdf_refresh; DESIGN.md, section "ESDF", incremental refresh), shared by both
tiers like those of tests/esdf_case.py: the GPU tier (tests/test_esdf_refresh_gpu.py) calls run_case in-process, the CPU tier
(tests/test_esdf_refresh_cpu.py) runs it as a child process on the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.esdf_refresh_case '<json spec>'
The checker is tests/esdf_model.py on the map as it is after the refresh: the bytes of every record of every block.  The tile
counts (what is stale, what is recomputed, which blocks changed) are worked out here from the tile coordinates."""
import ctypes
import json
import os
import sys

import numpy as np

from tests import esdf_case, mesh_case
from tests import esdf_model as M

VOXEL = esdf_case.VOXEL
cfg_of = esdf_case.cfg_of


def grow_of(spec):
    """g = ceil(R / 8) tiles."""
    return (M.reach(cfg_of(spec)["max_distance_m"], VOXEL) + 7) // 8


def resident_tiles(g):
    """(n, 3) tile coordinates of the map, from the packed tile keys (three 18-bit fields, bias 2^17)."""
    k = g.tile_keys().astype(np.uint64)
    f = lambda sh: ((k >> np.uint64(sh)) & np.uint64(0x3ffff)).astype(np.int64) - (1 << 17)
    return np.stack([f(36), f(18), f(0)], axis=1)


def tiles_of_blocks(blocks, vps):
    tpb = vps // 8
    o = np.array([(x, y, z) for x in range(tpb) for y in range(tpb) for z in range(tpb)], np.int64)
    return (np.asarray(blocks, np.int64).reshape(-1, 1, 3) * tpb + o[None]).reshape(-1, 3)


def reached(tiles, stale, grow, vps, region=None):
    """Of `tiles`, those within `grow` of one of `stale` on every axis (and inside the region of blocks): the set A."""
    tiles, stale = np.asarray(tiles, np.int64).reshape(-1, 3), np.asarray(stale, np.int64).reshape(-1, 3)
    near = (np.abs(tiles[:, None, :] - stale[None, :, :]).max(axis=2) <= grow).any(axis=1) if len(stale) else np.zeros(len(tiles), bool)
    if region is not None:
        b = tiles // (vps // 8)
        near &= ((b >= np.array(region[0])) & (b <= np.array(region[1]))).all(axis=1)
    return tiles[near]


def blocks_of_tiles(tiles, vps):
    b = np.unique(np.asarray(tiles, np.int64).reshape(-1, 3) // (vps // 8), axis=0)   # (np.unique sorts rows by x, then y, then z)
    return b.astype(np.int32).reshape(-1, 3)


def check_counts(g, st, stale_blocks, spec, region=None):
    vps = g.vps
    res = resident_tiles(g)
    S = tiles_of_blocks(stale_blocks, vps)
    A = reached(res, S, grow_of(spec), vps, region)
    assert st["tiles_total"] == len(res), (st, len(res))
    assert st["tiles_stale"] == len(S), (st, len(S))
    assert st["tiles_recomputed"] == len(A), (st, len(A))
    want = blocks_of_tiles(A, vps)
    got = g.esdf_changed_blocks()
    assert got.shape == want.shape and (got == want).all(), (got, want)
    return A


def check_map(g, st, spec, what, region=None):
    """The whole stored ESDF against the model of the map as it is now."""
    idx = g.block_indices()
    model = M.model_of(g, cfg_of(spec))
    rec = g.esdf_blocks(idx)
    M.assert_same(rec, model.blocks(idx, region=region), what)
    if region is None:
        for k in ("voxels_observed", "voxels_fixed", "voxels_clamped"):
            assert st[k] == model.stats[k], (what, k, st[k], model.stats[k])
    return idx, rec, model


def refused(code, call):
    from kimera_semantics_amd import binding as B
    try:
        call()
    except B.KsError as e:
        assert e.code == code, e
        return e
    raise AssertionError("accepted")


def _field(vps):
    return esdf_case.sphere_blocks(vps, 64 // vps)   # 64^3 voxels, 512 tiles at every block size


def _sphere(vps):
    g = mesh_case._integrator(0, 64, 48, vps=vps)
    g.upload(*_field(vps))
    return g


def _zero_weight(g, block):
    idx, t, s = g.download(np.array([block], np.int32))
    t["weight"] = 0.0
    return idx, t, s


def _flipped(g, block):
    idx, t, s = g.download(np.array([block], np.int32))
    t["distance"] = -t["distance"]
    return idx, t, s


def case_mutate(spec):
    vps = spec["vps"]
    g = _sphere(vps)
    first = g.esdf_update(**cfg_of(spec))
    assert len(g.esdf_changed_blocks()) == 0
    lo = int(g.block_indices().min())
    steps = [("interior, another random field", (0, 0, 0), lambda b: esdf_case.random_field([b], vps, 23)),
             ("corner, weight 0", (lo, lo, lo), lambda b: _zero_weight(g, b)),
             ("signs flipped", (1, -2, 0) if vps <= 16 else (0, -1, 0), lambda b: _flipped(g, b))]
    out = {}
    for what, block, make in steps:
        g.upload(*make(block))
        st = g.esdf_refresh()
        check_map(g, st, spec, what)
        check_counts(g, st, [block], spec)
        assert 0 < st["workspace_bytes"]
        if what.startswith("interior") and grow_of(spec) == 1:
            assert st["tiles_recomputed"] < st["tiles_total"], st
        out[what] = st["tiles_recomputed"]
    assert st["voxels_observed"] < first["voxels_observed"]          # (the corner block's voxels are gone)
    idx = g.block_indices()
    refreshed = g.esdf_blocks(idx)
    scratch = g.esdf_update(**cfg_of(spec))
    M.assert_same(g.esdf_blocks(idx), refreshed, "from scratch on the same context")
    for k in ("voxels_observed", "voxels_fixed", "voxels_clamped"):
        assert scratch[k] == st[k], (k, scratch, st)
    assert len(g.esdf_changed_blocks()) == 0
    g.close()
    return out


def case_integrated(spec):
    w, h = 64, 48
    extra = {"max_tiles": spec["max_tiles"]} if "max_tiles" in spec else {}
    g = mesh_case._integrator(spec["method"], w, h, **extra)
    # every pose looks elsewhere, so new tiles join the map with each frame (151, 671 and 1187 tiles after one, two and three
    # frames).  The update follows the first frame and the refresh the second; where the pool has to double in between, one
    # frame later each: 671 tiles fit a pool of 1024 and are more than half of it, so the pool doubles before the third frame
    before = spec.get("frames_before", 1)
    frames = mesh_case._frames(before + 1, w, h, step=40, hfov=50.0)
    for f in frames[:before]:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    idx1, rec1, _ = g.esdf(**cfg_of(spec))
    n1 = len(g.tile_keys())
    f2 = frames[before]
    g.integrate(f2.T_G_C, f2.xyz, f2.rgba, f2.labels)
    st = g.esdf_refresh()
    idx2, rec2, model = check_map(g, st, spec, "after the second frame")
    assert len(idx2) > len(idx1)
    n2 = len(g.tile_keys())
    assert st["tiles_total"] == n2 > n1 and n2 - n1 <= st["tiles_stale"] <= n2 and st["tiles_stale"] <= st["tiles_recomputed"] <= n2, (st, n1, n2)
    assert rec2.tobytes() != M.default_records(rec2.shape).tobytes()
    if "max_tiles" in spec:   # the pool held max_tiles at the update and holds more tiles than that now: it doubled in between
        assert spec["max_tiles"] // 2 < n1 <= spec["max_tiles"] < n2, (n1, n2)
    joined = np.array([tuple(b) not in {tuple(a) for a in idx1} for b in idx2])
    assert (rec2[joined]["flags"] != 0).any()                 # tiles that joined hold real records
    g.close()
    return dict(tiles=[n1, n2], stale=st["tiles_stale"], recomputed=st["tiles_recomputed"])


def case_clusters(spec):
    from kimera_semantics_amd import binding as B
    vps, room = 8, 64 << 20
    g = mesh_case._integrator(0, 64, 48, vps=vps)
    one = np.array([(x, y, z) for x in range(4) for y in range(4) for z in range(4)], np.int32)
    two = one + np.array([1000, 900, 800], np.int32)
    f1 = esdf_case.random_field(one, vps, 31)
    g.upload(*f1)
    g.esdf_update(**cfg_of(spec))
    f2 = esdf_case.random_field(two, vps, 32)
    g.upload(*f2)
    again = esdf_case.random_field([(1, 2, 1)], vps, 33)
    g.upload(*again)
    j = int(np.flatnonzero((one == np.array([1, 2, 1])).all(axis=1))[0])
    f1[1][j], f1[2][j] = again[1][0], again[2][0]
    st = g.esdf_refresh(max_workspace_bytes=room)
    assert 0 < st["workspace_bytes"] <= room, st
    check_counts(g, st, np.concatenate([two, [(1, 2, 1)]]), spec)
    total = dict(voxels_observed=0, voxels_fixed=0, voxels_clamped=0)
    for blocks, (idx, t, s) in ((one, f1), (two, f2)):      # further than R apart: each is the ESDF of its own blocks alone
        m = M.esdf_from_blocks(idx, t, s["label"], vps, VOXEL, **cfg_of(spec))
        M.assert_same(g.esdf_blocks(blocks), m.blocks(blocks), "cluster at %r" % (tuple(blocks[0]),))
        for k in total:
            total[k] += m.stats[k]
    for k in total:
        assert st[k] == total[k], (k, st, total)
    both = np.concatenate([one, two])
    before = g.esdf_blocks(both)
    e = refused(B.KS_ERR_UNSUPPORTED, lambda: g.esdf_update(max_workspace_bytes=room, **cfg_of(spec)))   # a box of 1004 x 904 x 804 tiles
    assert e.stats["workspace_bytes"] > (1 << 40), e.stats
    M.assert_same(g.esdf_blocks(both), before, "after the refused update")
    g.close()
    return dict(st)


def case_region_blocks(spec):
    """A region given in blocks of vps^3 voxels: the stored ESDF of an update over half of the map's blocks, and its refresh after a
    block inside and a block outside the region changed, against the model (the region's box is region * vps / 8 tiles)."""
    vps = spec["vps"]
    g = _sphere(vps)
    n = 64 // vps // 2
    region = ([-n, 0, -n], [n - 1, n - 1, n - 1])          # the half y >= 0
    g.esdf_update(region=region, **cfg_of(spec))
    idx = g.block_indices()
    model = M.model_of(g, cfg_of(spec))
    M.assert_same(g.esdf_blocks(idx), model.blocks(idx, region=region), "region update")
    inside = np.array([all(region[0][a] <= b[a] <= region[1][a] for a in range(3)) for b in idx])
    assert inside.sum() * 2 == len(idx) and (g.esdf_blocks(idx[inside])["flags"] != 0).any()
    assert g.esdf_blocks(idx[~inside]).tobytes() == M.default_records((int((~inside).sum()), vps ** 3)).tobytes()
    changed = [(0, 0, 0), (-1, -1, 0)]
    fresh = esdf_case.random_field([changed[0]], vps, 41)
    g.upload(*fresh)
    g.upload(*_flipped(g, changed[1]))
    st = g.esdf_refresh()
    check_map(g, st, spec, "region refresh", region=region)
    A = check_counts(g, st, changed, spec, region=region)
    assert 0 < len(A) < st["tiles_total"] // 2 + 1 and st["tiles_stale"] == 2 * (vps // 8) ** 3, st
    assert st["voxels_observed"] == inside.sum() * vps ** 3 - int((fresh[1]["weight"] == 0).sum()), st   # (the random block leaves a tenth unobserved)
    g.close()
    return dict(st)


def case_region(spec):
    vps = 8
    g = _sphere(vps)
    region = ([-1, -1, -1], [0, 0, 0])
    g.esdf_update(region=region, **cfg_of(spec))
    R = M.reach(cfg_of(spec)["max_distance_m"], VOXEL)
    assert R == 11
    # near: voxels 8..15 along x, within R of the region's last voxel 7.  far: the corner block, 17 voxels from the region's
    # first voxel on EVERY axis (the map is too small for 2 R on one axis): 17 sqrt(3) = 29.4 > 2 R = 22 voxels from it, and
    # three tiles from its tiles, more than g = 2 — no record of the region can depend on it
    near, far = (1, 0, 0), (-4, -4, -4)
    assert 8 - 7 <= R and 3 * 17 ** 2 > (2 * R) ** 2 and 3 > grow_of(spec)
    g.upload(*esdf_case.random_field([near], vps, 41))
    g.upload(*_flipped(g, far))
    st = g.esdf_refresh()
    idx, rec, model = check_map(g, st, spec, "region", region=region)
    A = check_counts(g, st, [near, far], spec, region=region)
    assert 0 < len(A) == st["tiles_recomputed"] <= 8 and st["tiles_stale"] == 2
    inside = np.array([all(region[0][a] <= b[a] <= region[1][a] for a in range(3)) for b in idx])
    assert inside.sum() == 8 and rec[~inside].tobytes() == M.default_records(rec[~inside].shape).tobytes()
    assert st["voxels_observed"] == 8 * 512, st
    g.close()
    return dict(st)


def case_independent(spec):
    from kimera_semantics_amd import binding as B
    vps = 8
    g = _sphere(vps)
    g.esdf_update(**cfg_of(spec))
    g.mesh()
    g.updated_block_indices(reset=True)
    block = (1, 1, -2)
    g.upload(*esdf_case.random_field([block], vps, 51))
    # the other consumers of "written since" run first: none of them takes the ESDF's mark
    assert g.mesh(only_stale=True).stats["blocks_meshed"] > 0
    g.updated_block_indices(reset=True)
    n, nr = ctypes.c_size_t(), ctypes.c_size_t()
    assert B.lib().ks_count_updated_voxels(g._h, ctypes.byref(n), ctypes.byref(nr)) == 0
    st = g.esdf_refresh()
    assert st["tiles_stale"] > 0
    idx, rec, _ = check_map(g, st, spec, "after the other consumers")
    check_counts(g, st, [block], spec)
    # ... and the refresh takes none of theirs: a second overwrite is re-meshed after a refresh that saw it first
    g.upload(*esdf_case.random_field([block], vps, 52))
    st = g.esdf_refresh()
    assert st["tiles_stale"] > 0
    idx, rec, _ = check_map(g, st, spec, "second overwrite")
    assert g.mesh(only_stale=True).stats["blocks_meshed"] > 0
    # nothing stale: nothing recomputed, the same bytes and totals
    again = g.esdf_refresh()
    assert again["tiles_stale"] == 0 and again["tiles_recomputed"] == 0 and again["tiles_total"] == st["tiles_total"], again
    assert len(g.esdf_changed_blocks()) == 0
    M.assert_same(g.esdf_blocks(idx), rec, "refresh right after a refresh")
    for k in ("voxels_observed", "voxels_fixed", "voxels_clamped"):
        assert again[k] == st[k], (k, again, st)
    g.close()
    return dict(st)


def case_errors(spec):
    from kimera_semantics_amd import binding as B
    vps = 8
    g = _sphere(vps)
    refused(B.KS_ERR_INVALID_ARG, g.esdf_refresh)                 # before any update
    g.esdf_update(**cfg_of(spec))
    g.clear()
    refused(B.KS_ERR_INVALID_ARG, g.esdf_refresh)                 # after clear()
    g.upload(*_field(vps))
    idx, before, _ = g.esdf(**cfg_of(spec))
    g.upload(*esdf_case.random_field([(0, 1, 0)], vps, 61))
    e = refused(B.KS_ERR_UNSUPPORTED, lambda: g.esdf_refresh(max_workspace_bytes=4096))
    assert e.stats["workspace_bytes"] > 4096 and e.stats["tiles_stale"] == 1 and e.stats["tiles_recomputed"] == 27, e.stats
    M.assert_same(g.esdf_blocks(idx), before, "after the refused refresh")
    st = g.esdf_refresh()                                         # the marks were not consumed
    assert st["tiles_stale"] == 1
    check_map(g, st, spec, "after the refusal")
    g.close()
    # a marcher context of the exact multi-GPU mode holds no voxel data
    marcher, owner = (mesh_case._integrator(1, 64, 48) for _ in range(2))
    f = mesh_case._frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    refused(B.KS_ERR_UNSUPPORTED, marcher.esdf_refresh)
    marcher.close()
    owner.close()
    return {}


CASES = {"region_blocks": case_region_blocks, "mutate": case_mutate, "integrated": case_integrated, "clusters": case_clusters, "region": case_region,
         "independent": case_independent, "errors": case_errors}

# max_distance_m 0.4: R = 8, g = 1, the window ends exactly on a tile edge; 0.55: R = 11, g = 2, it ends mid-tile
SPECS = {}
for _r, _d in ((8, 0.4), (11, 0.55)):
    for _vps in (8, 16):
        SPECS["mutate_vps%d_r%d" % (_vps, _r)] = dict(case="mutate", vps=_vps, max_distance_m=_d)
SPECS.update({
    "mutate_vps32_r8": dict(case="mutate", vps=32, max_distance_m=0.4),
    "mutate_vps32_r11": dict(case="mutate", vps=32, max_distance_m=0.55),
    "region_blocks_vps16": dict(case="region_blocks", vps=16, max_distance_m=0.55),
    "region_blocks_vps32": dict(case="region_blocks", vps=32, max_distance_m=0.55),
    "integrated_fast": dict(case="integrated", method=0, max_distance_m=0.4),
    "integrated_merged": dict(case="integrated", method=1, max_distance_m=0.4),
    "integrated_pool_doubles": dict(case="integrated", method=0, max_distance_m=0.4, max_tiles=1024, frames_before=2),
    "clusters": dict(case="clusters", max_distance_m=0.4),
    "region": dict(case="region", max_distance_m=0.55),
    "independent": dict(case="independent", max_distance_m=0.4),
    "errors": dict(case="errors", max_distance_m=0.4),
})


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("ESDF_REFRESH_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
