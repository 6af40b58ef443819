"""The object-instance cases, shared by both tiers: run_case(spec) drives whatever library the binding has loaded — the GPU tier
(tests/test_objects_gpu.py) calls it in-process, the CPU tier (tests/test_objects_cpu.py) runs it as a child process on the
host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.objects_case '<json spec>'
The checker is tests/objects_model.py (NumPy, written from the contract): the bytes of every record, every stat, the id of
every voxel of every block."""
import ctypes
import json
import os
import sys

import numpy as np

from tests import mesh_case
from tests import objects_model as M

VOXEL = mesh_case.VOXEL          # 5 cm
RANDOM_SEED = 7                  # chosen on the CPU with the model: case_random asserts what it is chosen for
RANDOM_LABELS = (3, 7, 12)
NONE = int(M.NONE)


# ---- fields ----------------------------------------------------------------------------------------------------------------
def voxel_field(vox, vps, resident=()):
    """Host-layout blocks (indices, tsdf, sem) with the voxels of `vox` = {(x, y, z) global index: (label, weight, distance)} set and
    everything else never observed (weight 0); the blocks are those of the voxels and of the `resident` voxel positions."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    at = sorted({tuple(int(c) // vps for c in p) for p in list(vox) + list(resident)})
    idx = np.array(at, np.int32).reshape(-1, 3)
    row = {b: j for j, b in enumerate(at)}
    t, s = np.zeros((len(idx), vps ** 3), B.TSDF_DTYPE), np.zeros((len(idx), vps ** 3), B.SEM_DTYPE)
    s["priors"] = np.float32(-0.60205999132)
    lut = synth.default_label_colors()
    for (x, y, z), (label, weight, distance) in vox.items():
        j, l = row[(x // vps, y // vps, z // vps)], (x % vps) + vps * ((y % vps) + vps * (z % vps))
        t["distance"][j, l], t["weight"][j, l], t["color"][j, l] = distance, weight, lut[label]
        s["label"][j, l], s["color"][j, l] = label, lut[label]
        s["priors"][j, l, label] = np.float32(-0.1)
    return idx, t, s


JUST_ABOVE = float(np.nextafter(np.float32(VOXEL), np.float32(1)))   # the smallest |distance| above the default surface_distance_m

# first_voxel -> (n_voxels, label) of the seams field with min_voxels = 1
SEAMS_EXPECTED = {
    (7, 3, 3): (2, 5),      # a face crossing (7,3,3)-(8,3,3)
    (7, 7, 2): (2, 6),      # an edge crossing (7,7,2)-(8,8,2): the tiles (1,0,0) and (0,1,0) are resident and empty there
    (7, 7, 7): (2, 7),      # a corner crossing (7,7,7)-(8,8,8)
    (7, 8, 4): (2, 8),      # a backward diagonal (8,7,4)-(7,8,4): tile offset (-1,+1,0)
    (-1, 0, 0): (2, 9),     # across the origin into negative indices
    (15, 3, 3): (1, 10),    # the same adjacency with two labels: no join
    (16, 3, 3): (1, 11),
    (14, 10, 3): (1, 12),   # a link broken by weight 0 at (15,10,3)
    (16, 10, 3): (1, 12),
    (14, 12, 3): (1, 13),   # a link broken by |distance| just above surface_distance_m at (15,12,3); (16,12,3) sits exactly on it
    (16, 12, 3): (1, 13),
    (31, 3, 3): (1, 14),    # its neighbour tile (4,0,0) is not resident
}


def seams_field(vps):
    on = lambda label: (label, 1.0, 0.0)
    vox = {(7, 3, 3): on(5), (8, 3, 3): on(5), (7, 7, 2): on(6), (8, 8, 2): on(6), (7, 7, 7): on(7), (8, 8, 8): on(7),
           (8, 7, 4): on(8), (7, 8, 4): on(8), (-1, 0, 0): on(9), (0, 0, 0): on(9), (15, 3, 3): on(10), (16, 3, 3): on(11),
           (14, 10, 3): on(12), (15, 10, 3): (12, 0.0, 0.0), (16, 10, 3): on(12),
           (14, 12, 3): on(13), (15, 12, 3): (13, 1.0, -JUST_ABOVE), (16, 12, 3): (13, 1.0, -VOXEL),
           (31, 3, 3): on(14), (3, 3, 6): (5, 1.0, float("nan"))}
    idx, t, s = voxel_field(vox, vps, resident=[(8, 0, 0), (0, 8, 0)])
    # (the tile beside (31,3,3) stays absent; in a block of 64 it is resident and empty, which joins nothing either)
    assert vps == 64 or not any(tuple(b) == (32 // vps, 0, 0) for b in idx)
    return idx, t, s


def serpentine_field(vps):
    """Two interleaved one-voxel-wide combs through 4 x 4 x 2 tiles from (-16, -16, 0): comb A (label 3) in the layers z = 0, 4, 8, 12,
    rows along x at every even y, linked at alternating ends, the layers linked by a column at the corner (0, 0); comb B (label 7)
    the same in the layers z = 2, 6, 10, 14 with rows at every odd y and its column at the corner (31, 31)."""
    vox = {}
    o = (-16, -16, 0)
    put = lambda x, y, z, label: vox.__setitem__((x + o[0], y + o[1], z + o[2]), (label, 1.0, 0.0))
    for label, z0, y0, corner in ((3, 0, 0, (0, 0)), (7, 2, 1, (31, 31))):
        for z in range(z0, 16, 4):
            rows = list(range(y0, 32, 2))
            for k, y in enumerate(rows):
                for x in range(32):
                    put(x, y, z, label)
                if k + 1 < len(rows):
                    put(31 if k % 2 == 0 else 0, y + 1, z, label)
            if z + 4 < 16:
                for dz in (1, 2, 3):
                    put(corner[0], corner[1], z + dz, label)
    return voxel_field(vox, vps)


SERPENTINE_VOXELS = 4 * (16 * 32 + 15) + 3 * 3


def random_field(vps, seed=RANDOM_SEED):
    """4 x 4 x 4 tiles from (-16, -16, -16): 40 % surface voxels, of the others half never observed and half far from the surface;
    three labels uniformly.  At 32 and 64 voxels per side: the voxels of the vps-16 field, in the blocks {-1, 0}^3 that hold them, and
    every other voxel of those blocks never observed."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    if vps > 16:
        idx16, t16, s16 = random_field(16, seed)
        box = ((-vps, vps),) * 3
        out = []
        for rows in (t16, s16):
            big = np.zeros((2 * vps,) * 3, rows.dtype)
            if rows.dtype == B.SEM_DTYPE:
                big["priors"] = np.float32(-0.60205999132)
            big[vps - 16:vps + 16, vps - 16:vps + 16, vps - 16:vps + 16] = mesh_case.from_blocks(idx16, rows, 16, ((-16, 16),) * 3)
            idx, blocked = mesh_case.to_blocks([b[0] for b in box], big, vps)
            out.append(blocked)
        return idx, out[0], out[1]
    rng = np.random.default_rng(seed)
    n = 32 // vps
    idx = np.array([(x, y, z) for x in range(-n // 2, n // 2) for y in range(-n // 2, n // 2) for z in range(-n // 2, n // 2)], np.int32)
    shape = (len(idx), vps ** 3)
    t, s = np.zeros(shape, B.TSDF_DTYPE), np.zeros(shape, B.SEM_DTYPE)
    surface = rng.random(shape) < 0.40
    seen = surface | (rng.random(shape) < 0.5)
    t["weight"] = seen.astype(np.float32)
    t["distance"] = np.where(surface, rng.uniform(-0.04, 0.04, shape), 0.3).astype(np.float32)
    label = rng.choice(np.array(RANDOM_LABELS, np.uint8), shape)
    lut = synth.default_label_colors()
    t["color"] = lut[label]
    s["label"], s["color"] = label, lut[label]
    s["priors"] = np.float32(-0.60205999132)
    np.put_along_axis(s["priors"], label[..., None].astype(np.int64), np.float32(-0.1), axis=-1)
    return idx, t, s


def make_field(kind, vps):
    if kind == "seams":
        return seams_field(vps)
    if kind == "serpentine":
        return serpentine_field(vps)
    if kind == "random":
        return random_field(vps)
    if kind == "sphere":
        return mesh_case.make_field("sphere", vps)
    raise ValueError(kind)


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _uploaded(kind, vps, reverse=False):
    g = mesh_case._integrator(0, 64, 48, vps=vps)
    idx, t, s = make_field(kind, vps)
    if reverse:
        idx, t, s = idx[::-1].copy(), t[::-1].copy(), s[::-1].copy()
    g.upload(idx, t, s)
    return g


def check(g, cfg, what, model=None):
    """One update against the model: (records, stats, block indices, ids, model)."""
    rec, stats = g.objects(**cfg)
    idx = g.block_indices()
    ids = g.object_ids(idx)
    model = model or M.model_of(g, cfg)
    M.assert_same((rec, stats), model, idx, ids, what)
    assert stats["workspace_bytes"] == M.workspace_bytes(len(g.tile_keys()), stats["components"]), (what, stats)
    return rec, stats, idx, ids, model


def refused(code, call):
    from kimera_semantics_amd import binding as B
    try:
        call()
    except B.KsError as e:
        assert e.code == code, e
        return e
    raise AssertionError("accepted")


def _by_first(rec):
    return {tuple(int(v) for v in r["first_voxel"]): (int(r["n_voxels"]), int(r["label"])) for r in rec}


def crossing_a_seam(rec):
    return int(((rec["bb_min"] >> 3) != (rec["bb_max"] >> 3)).any(axis=1).sum())


# ---- cases -----------------------------------------------------------------------------------------------------------------
def case_seams(spec):
    g = _uploaded("seams", spec["vps"])
    rec, stats, idx, ids, model = check(g, dict(min_voxels=1), "seams")
    assert _by_first(rec) == SEAMS_EXPECTED, _by_first(rec)
    assert stats["objects"] == stats["components"] == len(SEAMS_EXPECTED) and stats["voxels_surface"] == 17
    # the record of the crossing at the origin, field by field
    r = rec[0]
    assert tuple(r["first_voxel"]) == (-1, 0, 0) and tuple(r["bb_min"]) == (-1, 0, 0) and tuple(r["bb_max"]) == (0, 0, 0)
    assert tuple(r["sum"]) == (-1, 0, 0) and r["pad"] == 0
    # with min_voxels = 2 the singletons go, and their voxels read as none
    rec2, stats2, _, ids2, _ = check(g, dict(min_voxels=2), "seams, min_voxels 2")
    assert stats2["objects"] == 5 and stats2["components"] == len(SEAMS_EXPECTED) and (ids2 != NONE).sum() == 10
    g.close()
    return dict(stats)


def case_serpentine(spec):
    g = _uploaded("serpentine", spec["vps"])
    rec, stats, idx, ids, model = check(g, {}, "serpentine")
    assert len(rec) == 2 and sorted(int(l) for l in rec["label"]) == [3, 7], rec
    assert (rec["n_voxels"] == SERPENTINE_VOXELS).all() and stats["components"] == 2, (rec, stats)
    assert stats["voxels_surface"] == stats["voxels_in_objects"] == 2 * SERPENTINE_VOXELS
    assert len(g.tile_keys()) >= 4 * 4 * 2
    g.close()
    return dict(stats)


def case_random(spec):
    g = _uploaded("random", spec["vps"])
    rec, stats, idx, ids, model = check(g, dict(min_voxels=1), "random, min_voxels 1")
    # what the seed is chosen for
    assert (rec["n_voxels"] > 1000).sum() >= 1, rec["n_voxels"].max()
    assert (rec["n_voxels"] == 1).sum() >= 100, (rec["n_voxels"] == 1).sum()
    assert crossing_a_seam(rec) >= 20, crossing_a_seam(rec)
    assert set(int(l) for l in rec["label"]) == set(RANDOM_LABELS)
    assert 0.35 < stats["voxels_surface"] / 32.0 ** 3 < 0.45
    rec8, stats8, _, ids8, _ = check(g, dict(min_voxels=8), "random, min_voxels 8")
    assert stats8["components"] == stats["components"] > stats8["objects"] > 0
    assert (ids8 == NONE).sum() > (ids == NONE).sum()
    mask = sum(1 << l for l in RANDOM_LABELS if l != 7)
    recm, statsm, _, _, _ = check(g, dict(min_voxels=1, label_mask=mask), "random, label 7 masked")
    assert set(int(l) for l in recm["label"]) == set(RANDOM_LABELS) - {7} and statsm["voxels_surface"] < stats["voxels_surface"]
    assert recm.tobytes() == rec[rec["label"] != 7].tobytes()
    g.close()
    return dict(stats, singletons=int((rec["n_voxels"] == 1).sum()), crossing=crossing_a_seam(rec), largest=int(rec["n_voxels"].max()))


def case_order(spec):
    """The same voxels uploaded in another block order (other slots) give the same bytes."""
    a, b = _uploaded("random", spec["vps"]), _uploaded("random", spec["vps"], reverse=True)
    ka, kb = a.tile_keys(), b.tile_keys()
    assert sorted(ka) == sorted(kb) and (ka != kb).any()
    ra, sa, idx, ia, model = check(a, {}, "forward order")
    rb, sb, idx_b, ib, _ = check(b, {}, "reversed order", model=model)
    assert (idx == idx_b).all() and ra.tobytes() == rb.tobytes() and ia.tobytes() == ib.tobytes() and sa == sb
    a.close()
    b.close()
    return dict(sa)


def case_integrated(spec):
    w, h = spec.get("size", [64, 48])
    g = mesh_case._integrator(spec["method"], w, h)
    for f in mesh_case._frames(2, w, h):
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    rec, stats, idx, ids, model = check(g, spec.get("cfg", {}), "integrated")
    labels = np.unique(rec["label"])
    assert len(labels) >= 3, (labels, stats)
    g.close()
    return dict(stats, labels=len(labels))


def _updated_voxels(g):
    from kimera_semantics_amd import binding as B
    n, nr = ctypes.c_size_t(), ctypes.c_size_t()
    g._chk(B.lib().ks_count_updated_voxels(g._h, ctypes.byref(n), ctypes.byref(nr)))
    return n.value, nr.value


def case_lifetime(spec):
    """Side effects (none) and the lifetime of what is stored."""
    from kimera_semantics_amd import binding as B
    w, h = 64, 48
    f1, f2, f3 = mesh_case._frames(3, w, h, step=40, hfov=50.0)   # every pose looks elsewhere: new tiles join the map
    a, b = (mesh_case._integrator(spec.get("method", 0), w, h) for _ in range(2))
    ecfg = dict(min_distance_m=0.1, max_distance_m=0.4)
    for g in (a, b):
        g.integrate(f1.T_G_C, f1.xyz, f1.rgba, f1.labels)
        g.mesh()
        g.esdf_update(**ecfg)
        g.integrate(f2.T_G_C, f2.xyz, f2.rgba, f2.labels)
    rec, stats, idx, ids, model = check(a, {}, "after frame 2")   # ... an objects call in between, on `a` alone
    assert stats["objects"] > 0
    assert _updated_voxels(a) == _updated_voxels(b)
    ua, ub = a.updated_block_indices(reset=False), b.updated_block_indices(reset=False)
    assert ua.shape == ub.shape and (ua == ub).all() and len(ua) > 0
    ma, mb = a.mesh(only_stale=True), b.mesh(only_stale=True)
    assert ma.stats == mb.stats and 0 < ma.stats["blocks_meshed"] < ma.stats["blocks_total"], (ma.stats, mb.stats)
    ea, eb = a.esdf_refresh(), b.esdf_refresh()
    assert ea == eb and ea["tiles_stale"] > 0, (ea, eb)
    ia, ta, sa = a.download()
    ib, tb, sb = b.download()
    assert (ia == ib).all() and ta.tobytes() == tb.tobytes() and sa.tobytes() == sb.tobytes()
    # a second update gives the same bytes
    rec2, stats2 = a.objects()
    assert rec2.tobytes() == rec.tobytes() and stats2 == stats and a.object_ids(idx).tobytes() == ids.tobytes()
    # the store describes the map as it was at the update
    a.integrate(f3.T_G_C, f3.xyz, f3.rgba, f3.labels)
    idx3 = a.block_indices()
    old = {tuple(int(v) for v in r) for r in idx}
    joined = np.array([r for r in idx3 if tuple(int(v) for v in r) not in old], np.int32).reshape(-1, 3)
    assert len(joined) > 0
    assert a.object_ids(idx).tobytes() == ids.tobytes() and a.object_records().tobytes() == rec.tobytes()
    assert (a.object_ids(joined) == NONE).all()
    M.assert_same((a.object_records(), stats), model, idx3, a.object_ids(idx3), "snapshot after another frame")
    rec3, stats3, _, _, _ = check(a, {}, "third update")
    assert stats3["voxels_surface"] > stats["voxels_surface"]
    a.clear_voxels()
    refused(B.KS_ERR_INVALID_ARG, lambda: a.object_ids(idx))
    refused(B.KS_ERR_INVALID_ARG, lambda: a.object_records())
    refused(B.KS_ERR_INVALID_ARG, lambda: a.object_query(np.zeros((1, 3))))
    # ... and so does ks_clear
    assert b.objects()[1]["objects"] > 0 and len(b.object_records()) > 0
    b.clear()
    refused(B.KS_ERR_INVALID_ARG, lambda: b.object_ids(idx))
    refused(B.KS_ERR_INVALID_ARG, lambda: b.object_records())
    refused(B.KS_ERR_INVALID_ARG, lambda: b.object_query(np.zeros((1, 3))))
    assert b.objects()[1]["objects"] == 0 and len(b.object_records()) == 0   # (an update of the emptied map: zero objects, stored)
    a.close()
    b.close()
    return dict(stats)


def case_errors(spec):
    from kimera_semantics_amd import binding as B
    L = B.lib()
    g = _uploaded("sphere", 8)
    idx = g.block_indices()
    n = ctypes.c_size_t()
    one = np.zeros(1, B.OBJECT_DTYPE)
    # before any update
    refused(B.KS_ERR_INVALID_ARG, lambda: g.object_ids(idx))
    refused(B.KS_ERR_INVALID_ARG, lambda: g.object_query(np.zeros((1, 3))))
    refused(B.KS_ERR_INVALID_ARG, lambda: g.object_records())
    assert L.ks_objects_size(g._h, ctypes.byref(n)) == B.KS_ERR_INVALID_ARG
    assert L.ks_objects_download(g._h, one.ctypes.data, 1, ctypes.byref(n)) == B.KS_ERR_INVALID_ARG
    # NULL context or configuration
    cfg = g.objects_config()
    assert L.ks_objects_update(None, ctypes.byref(cfg), None) == B.KS_ERR_INVALID_ARG
    assert L.ks_objects_update(g._h, None, None) == B.KS_ERR_INVALID_ARG
    assert L.ks_objects_default_config(None) == B.KS_ERR_INVALID_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(B.KS_ERR_INVALID_ARG, lambda: g.objects(min_weight=bad))
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        refused(B.KS_ERR_INVALID_ARG, lambda: g.objects(surface_distance_m=bad))
    for bad in (0, 1 << 21, 0xffffffff, 0x3fffff):
        refused(B.KS_ERR_INVALID_ARG, lambda: g.objects(label_mask=bad))
    refused(B.KS_ERR_INVALID_ARG, lambda: g.objects(min_voxels=0))
    refused(B.KS_ERR_INVALID_ARG, lambda: g.object_ids(idx))            # ... and none of these stored anything
    # the sphere: one object of label 5; stats may be NULL
    assert L.ks_objects_update(g._h, ctypes.byref(cfg), None) == 0
    rec, stats, _, _, _ = check(g, {}, "sphere")
    assert len(rec) == 1 and rec["label"][0] == 5
    # capacity too small
    assert L.ks_objects_size(g._h, ctypes.byref(n)) == 0 and n.value == 1
    n.value = 99
    assert L.ks_objects_download(g._h, one.ctypes.data, 0, ctypes.byref(n)) == B.KS_ERR_INVALID_ARG and n.value == 1
    assert L.ks_objects_download(g._h, None, 1, ctypes.byref(n)) == B.KS_ERR_INVALID_ARG
    assert L.ks_objects_download(g._h, one.ctypes.data, 1, None) == 0 and one.tobytes() == rec.tobytes()
    g.close()
    # an empty map is no error
    e = mesh_case._integrator(0, 64, 48, vps=8)
    rec, stats = e.objects()
    assert len(rec) == 0 and all(stats[k] == 0 for k in M.STAT_KEYS), stats
    assert (e.object_ids(idx[:2]) == NONE).all() and (e.object_query(np.zeros((3, 3))) == NONE).all()
    e.close()
    # a marcher context of the exact multi-GPU mode holds no voxel data
    marcher, owner = (mesh_case._integrator(1, 64, 48) for _ in range(2))
    f = mesh_case._frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    refused(B.KS_ERR_UNSUPPORTED, lambda: marcher.objects())
    assert owner.objects()[1]["voxels_surface"] > 0   # (the owner holds the map)
    marcher.close()
    owner.close()
    return {}


def ids_at(idx, ids, vps, ijk):
    """The id of the voxels ijk (n, 3) from the ids of host-layout blocks: none where no block is."""
    row = {tuple(int(v) for v in b): j for j, b in enumerate(idx)}
    out = np.full(len(ijk), M.NONE, np.uint32)
    for i, p in enumerate(np.asarray(ijk, np.int64)):
        j = row.get(tuple(int(c) // vps for c in p))
        if j is not None:
            x, y, z = (int(c) % vps for c in p)
            out[i] = ids[j, x + vps * (y + vps * z)]
    return out


def case_query(spec):
    vps = spec["vps"]
    g = _uploaded("random", vps)
    rec, stats, idx, ids, model = check(g, dict(min_voxels=1), "random")
    rng = np.random.default_rng(3)
    ijk = rng.integers(-22, 22, (4096, 3))          # the map spans [-16, 16): some points lie outside it
    jitter = rng.uniform(-0.4, 0.4, (4096, 3))
    xyz = ((ijk + 0.5 + jitter) * VOXEL).astype(np.float32)
    got = g.object_query(xyz)
    want = ids_at(idx, ids, vps, ijk)
    assert (want == model.at(ijk)).all()
    assert got.dtype == np.uint32 and (got == want).all(), np.argwhere(got != want)[:5]
    outside = (ijk < -16).any(axis=1) | (ijk >= 16).any(axis=1)
    assert outside.sum() > 100 and (got[outside] == NONE).all() and (got != NONE).sum() > 500 and (got[~outside] == NONE).sum() > 500
    far = np.array([[1e9, 0, 0], [0, -1e9, 0], [float("nan"), 0, 0], [0, 0, float("inf")]], np.float32)   # beyond the packed range
    assert (g.object_query(far) == NONE).all()
    g.close()
    return {}


def case_planted(spec):
    """A handful of surface voxels at the ends of the linear index range of two blocks: the per-voxel ids of the block export against
    the model ((-1, 0, 0) and (0, 0, 0) touch across the seam and make one object of two)."""
    vox = mesh_case.planted_voxels(spec["vps"])
    g = mesh_case._integrator(0, 64, 48, vps=spec["vps"])
    g.upload(*voxel_field({v: (5, 1.0, 0.0) for v in vox}, spec["vps"]))
    rec, stats, idx, ids, model = check(g, dict(min_voxels=1), "planted")
    assert len(idx) == 2 and stats["voxels_surface"] == stats["voxels_in_objects"] == (ids != NONE).sum() == len(vox), stats
    assert stats["objects"] == len(vox) - 1 and stats["largest_object_voxels"] == 2, stats
    g.close()
    return dict(stats)


CASES = {"planted": case_planted, "seams": case_seams, "serpentine": case_serpentine, "random": case_random, "order": case_order, "integrated": case_integrated,
         "lifetime": case_lifetime, "errors": case_errors, "query": case_query}

# name -> spec: the same cases in both tiers
SPECS = {}
for _vps in (8, 16, 32):
    for _case in ("seams", "serpentine", "random", "order", "query"):
        SPECS["%s_vps%d" % (_case, _vps)] = dict(case=_case, vps=_vps)
SPECS.update({
    "planted_vps64": dict(case="planted", vps=64),
    "integrated_fast": dict(case="integrated", method=0),
    "integrated_merged": dict(case="integrated", method=1),
    "lifetime": dict(case="lifetime"),
    "errors": dict(case="errors"),
})


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("OBJECTS_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
