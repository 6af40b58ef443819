"""The cases of submap fusion (ks_fuse_map), shared by both tiers: the GPU tier (tests/test_fuse_gpu.py) calls
run_case in-process, the CPU tier (tests/test_fuse_cpu.py) runs it as a child process on the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.fuse_case '<json spec>'
The yardstick is tests/fuse_model.py (NumPy, written from the contract): every comparison is exact, maps arrive through
ks_upload_blocks, and downloads are per block (sorted), never per slot."""
import ctypes
import json
import os
import sys

import numpy as np

from tests import esdf_case, mesh_case
from tests import fuse_model as M

VOXEL = mesh_case.VOXEL          # 5 cm
ESDF_CFG = dict(min_distance_m=0.1, max_distance_m=0.4)
TILE_WORKSPACE = 512 * 128 + 16  # what one candidate tile needs of max_workspace_bytes


# ---- poses, contexts, fields ------------------------------------------------------------------------------------------------------
def pose(axis=(0, 0, 1), deg=0.0, t=(0, 0, 0)):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = np.deg2rad(deg) / 2
    return np.concatenate([[np.cos(h)], np.sin(h) * a, np.asarray(t, np.float64)]).astype(np.float32)


POSES = {
    "identity": pose(),
    "shift_voxels": pose(t=(3 * VOXEL, -11 * VOXEL, 8 * VOXEL)),      # crosses tile seams, negative indices
    "shift_half": pose(t=(0.5 * VOXEL, -0.5 * VOXEL, 0.5 * VOXEL)),
    "yaw90": pose((0, 0, 1), 90.0),
    "generic": pose((1, 2, 3), 33.0, (0.31, -0.17, 0.23)),
    "far": pose(t=(6e4, 0, 0)),
}


def _ctx(vps=8, max_tiles=512, method=0, pipeline=0, size=(64, 48), **extra):
    return mesh_case._integrator(method, size[0], size[1], vps=vps, pipeline=pipeline, max_tiles=max_tiles, **extra)


def sphere_field(vps):
    """The sphere of radius 0.6 m over [-0.8 m, 0.8 m)^3: 64 tiles either way."""
    return esdf_case.sphere_blocks(vps, 4 if vps == 8 else 2)


def random_cube(vps, seed, lo=-1, n=None):
    """Not geometric (esdf_case.random_field): a cube of blocks from block `lo` on, 3^3 blocks of 8^3 voxels or 2^3 of 16^3."""
    n = n or (3 if vps == 8 else 2)
    idx = np.array([(lo + x, lo + y, lo + z) for x in range(n) for y in range(n) for z in range(n)], np.int32)
    return esdf_case.random_field(idx, vps, seed)


def holes_field(vps=8):
    """A random field (a tenth of its voxels unobserved) over the sphere's blocks with a third of the blocks missing."""
    idx = sphere_field(vps)[0]
    keep = np.array([(int(b[0]) + 2 * int(b[1]) + 3 * int(b[2])) % 3 != 0 for b in idx], bool)
    return esdf_case.random_field(idx[keep], vps, 17)


FIELDS = {"sphere": sphere_field, "holes": holes_field, "random": lambda vps: random_cube(vps, 21)}


def _rows(a):
    return [tuple(int(v) for v in r) for r in np.asarray(a).reshape(-1, 3)]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def tile_key(t):
    b = 1 << 17
    return ((int(t[0]) + b) << 36) | ((int(t[1]) + b) << 18) | (int(t[2]) + b)


def refused(code, call):
    from kimera_semantics_amd import binding as B
    try:
        call()
    except B.KsError as e:
        assert e.code == code, e
        return e
    raise AssertionError("accepted")


def capacity(g):
    return g.remove_blocks(np.zeros((0, 3), np.int32))["pool_capacity_tiles"]


# ---- the yardstick --------------------------------------------------------------------------------------------------------------
def model_of(dst, src, T, min_weight=1e-4):
    """The model's result for the maps the two contexts hold now."""
    from kimera_semantics_amd import synth
    di, dt, ds = dst.download()
    si, st, ss = src.download()
    return M.fuse((di, dt, ds, dst.vps), (si, st, ss, src.vps), T, VOXEL, min_weight=min_weight, color_mode=int(dst.cfg.color_mode),
                  max_weight=float(dst.cfg.max_weight), label_rgba=synth.default_label_colors())


def assert_map(g, R, what):
    """The destination holds the model's blocks, byte for byte."""
    assert _same(g.block_indices(), R.idx), (what, len(g.block_indices()), len(R.idx))
    _, t, s = g.download(R.idx)
    for name, a, b in (("distance", t["distance"], R.tsdf["distance"]), ("weight", t["weight"], R.tsdf["weight"]), ("colour", t["color"], R.tsdf["color"]),
                       ("label", s["label"], R.sem["label"]), ("priors", s["priors"], R.sem["priors"]), ("semantic colour", s["color"], R.sem["color"])):
        if a.tobytes() != b.tobytes():
            bad = (a.reshape(a.shape[0], a.shape[1], -1).view(np.uint8) != b.reshape(a.shape[0], a.shape[1], -1).view(np.uint8)).any(axis=2)
            j, l = np.argwhere(bad)[0]
            raise AssertionError("%s: %s differs at %d voxels (%d of them touched), first block %r voxel %d: %r vs %r" % (
                what, name, bad.sum(), (bad & R.touched).sum(), tuple(R.idx[j]), l, a[j, l], b[j, l]))
    assert t.tobytes() == R.tsdf.tobytes() and s.tobytes() == R.sem.tobytes(), what


def fuse_and_check(dst, src, T, what, **kw):
    """One call against the model: map, tile set and stats."""
    tiles_before = set(dst.tile_keys().tolist())
    R = model_of(dst, src, T, kw.get("min_weight") or 1e-4)
    n_src = len(src.tile_keys())
    stats = dst.fuse(src, T, **kw)
    assert_map(dst, R, what)
    touched = {tile_key(t) for t in R.tiles_touched}
    assert set(dst.tile_keys().tolist()) == tiles_before | touched, what       # a tile exists iff it existed or holds a touched voxel
    assert len(dst.tile_keys()) == len(tiles_before | touched), what
    assert stats["tiles_source"] == n_src and stats["voxels_fused"] == R.voxels_fused, (what, stats, R.voxels_fused)
    assert stats["tiles_touched"] == len(touched) <= stats["tiles_candidate"], (what, stats, len(touched))
    assert stats["tiles_allocated"] == len(touched - tiles_before), (what, stats)
    if n_src:
        assert stats["chunks"] >= 1 and stats["workspace_bytes"] >= TILE_WORKSPACE and stats["workspace_bytes"] % TILE_WORKSPACE == 0, (what, stats)
    return R, stats


def _pair(spec):
    """(dst, src) as the spec describes them: `src_field` uploaded into a context of `src_vps`, `dst_field` (or nothing) into `dst_vps`."""
    src = _ctx(vps=spec.get("src_vps", 8))
    src.upload(*FIELDS[spec.get("src_field", "sphere")](src.vps))
    dst = _ctx(vps=spec.get("dst_vps", 8), color_mode=spec.get("color_mode", 1))
    if spec.get("dst_field"):
        dst.upload(*FIELDS[spec["dst_field"]](dst.vps))
    return dst, src


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def case_pose(spec):
    dst, src = _pair(spec)
    R, stats = fuse_and_check(dst, src, POSES[spec["pose"]], spec["pose"])
    assert stats["voxels_fused"] > 5000, stats
    if spec["pose"] == "identity" and not spec.get("dst_field"):
        # at the identity the centres ARE source voxels (f = 0.5 - 0.5 exactly or one rounding off it): what is touched carries a source voxel
        assert stats["tiles_touched"] <= stats["tiles_source"]
    if spec.get("dst_field"):
        before_blocks = len(FIELDS[spec["dst_field"]](dst.vps)[0])
        assert stats["tiles_allocated"] > 0 and stats["tiles_touched"] > stats["tiles_allocated"] and len(R.idx) > before_blocks, stats   # overlaps, and grows
    dst.close()
    src.close()
    return stats


def case_holes(spec):
    dst, src = _pair(dict(spec, src_field="holes"))
    R, stats = fuse_and_check(dst, src, POSES["generic"], "holes")
    assert 0 < stats["tiles_touched"] < stats["tiles_candidate"], stats
    assert _same(dst.block_indices(), R.idx)
    assert 0 < stats["voxels_fused"] < 512 * stats["tiles_touched"], stats
    dst.close()
    src.close()
    return stats


def case_chunked(spec):
    from kimera_semantics_amd import binding as B
    a, src = _pair(dict(spec, dst_field="random"))
    b = _ctx()
    b.upload(*FIELDS["random"](8))
    T = POSES["generic"]
    R, whole = fuse_and_check(a, src, T, "one chunk")
    assert whole["chunks"] == 1, whole
    before = b.download()
    keys = sorted(b.tile_keys().tolist())
    e = refused(B.KS_ERR_UNSUPPORTED, lambda: b.fuse(src, T, max_workspace_bytes=TILE_WORKSPACE - 1))
    assert e.stats["workspace_bytes"] == TILE_WORKSPACE and e.stats["tiles_touched"] == 0, e.stats
    _, t, s = b.download(before[0])
    assert _same(b.block_indices(), before[0]) and t.tobytes() == before[1].tobytes() and s.tobytes() == before[2].tobytes()
    assert sorted(b.tile_keys().tolist()) == keys
    parts = b.fuse(src, T, max_workspace_bytes=2 * TILE_WORKSPACE + 5)
    assert parts["chunks"] == (parts["tiles_candidate"] + 1) // 2 > 1 and parts["workspace_bytes"] == 2 * TILE_WORKSPACE, parts
    assert_map(b, R, "chunks of two tiles")
    for k in ("tiles_source", "tiles_candidate", "tiles_touched", "tiles_allocated", "voxels_fused"):
        assert parts[k] == whole[k], (k, parts, whole)
    assert sorted(a.tile_keys().tolist()) == sorted(b.tile_keys().tolist())
    for c in (a, b, src):
        c.close()
    return parts


def case_upload_order(spec):
    idx, t, s = sphere_field(8)
    rng = np.random.default_rng(3)
    order = rng.permutation(len(idx))
    T = POSES["generic"]
    out = []
    for o in (np.arange(len(idx)), order, order[::-1]):
        src, dst = _ctx(), _ctx()
        src.upload(idx[o], t[o], s[o])
        st = dst.fuse(src, T)
        out.append((dst.download(), st, src.tile_keys().tolist()))
        src.close()
        dst.close()
    assert out[0][2] != out[1][2] != out[2][2]            # the slots of the source really differ
    for (d, st, _) in out[1:]:
        assert _same(d[0], out[0][0][0]) and d[1].tobytes() == out[0][0][1].tobytes() and d[2].tobytes() == out[0][0][2].tobytes()
        assert st == out[0][1], (st, out[0][1])
    return out[0][1]


def _sum_stats(stats):
    keys = ("n_points", "n_valid_points", "n_rays_cast", "n_voxel_updates", "n_blocks_allocated")
    return {k: sum(int(getattr(s, k)) for s in stats) for k in keys}


def case_in_flight(spec):
    """Both contexts pipelined, their 64 x 48 frames not yet flushed: the result is that of flush-then-fuse, and the statistics of the
    frames the call completed arrive at the next flush."""
    w, h = 64, 48
    frames = mesh_case._frames(4, w, h, step=12)
    make = lambda: _ctx(vps=16, method=1, pipeline=2, max_tiles=2048, size=(w, h))
    T = POSES["generic"]
    got, want = {}, {}
    dst, src, rdst, rsrc = make(), make(), make(), make()
    for c, r, fr, name in ((dst, rdst, frames[:2], "dst"), (src, rsrc, frames[2:], "src")):
        got[name] = [c.integrate(f.T_G_C, f.xyz, f.rgba, f.labels) for f in fr]
        want[name] = [r.integrate(f.T_G_C, f.xyz, f.rgba, f.labels) for f in fr] + [r.flush()]
        assert c.pipeline_shape()["lag"] > 0 and _sum_stats(got[name])["n_voxel_updates"] < _sum_stats(want[name])["n_voxel_updates"]   # frames in flight
    src_before = rsrc.download()
    st = dst.fuse(src, T)
    R, rst = fuse_and_check(rdst, rsrc, T, "flushed first")
    assert st == rst, (st, rst)
    assert_map(dst, R, "frames in flight")
    assert st["voxels_fused"] > 1000
    for c, name in ((dst, "dst"), (src, "src")):
        got[name].append(c.flush())
        a, b = _sum_stats(got[name]), _sum_stats(want[name])
        for k in ("n_points", "n_valid_points", "n_rays_cast", "n_voxel_updates"):
            assert a[k] == b[k], (name, k, a, b)
    _, t, s = src.download(src_before[0])
    assert _same(src.block_indices(), src_before[0]) and t.tobytes() == src_before[1].tobytes() and s.tobytes() == src_before[2].tobytes()
    for c in (dst, src, rdst, rsrc):
        c.close()
    return st


def _mesh_same(a, b, what):
    for k in ("blocks", "xyz", "normals", "rgba", "labels"):
        assert _same(getattr(a, k), getattr(b, k)), (what, k)
    assert a.stats["triangles_total"] == b.stats["triangles_total"] and a.stats["blocks_total"] == b.stats["blocks_total"], what


def case_products(spec):
    """The destination holds a stored mesh and a stored ESDF: the refreshes after the call equal a fresh context that was given the
    fused map by upload.  The source is only read: bytes, updated list, both stale bits, its own stored products."""
    dst, src = _ctx(), _ctx()
    # the destination: the sphere's lower half; the source: the whole sphere, moved a little (the two surfaces nearly agree)
    idx, t, s = sphere_field(8)
    low = idx[:, 2] < 0
    dst.upload(idx[low], t[low], s[low])
    src.upload(idx, t, s)
    m0 = dst.mesh()
    dst.esdf_update(**ESDF_CFG)
    sm0 = src.mesh()
    se0 = src.esdf_update(**ESDF_CFG)
    src_before = src.download()
    src_updated = src.updated_block_indices(reset=False)
    src_keys = src.tile_keys().tolist()
    assert m0.n_triangles > 200 and len(src_updated) == len(idx)
    T = pose((0, 1, 0), 4.0, (0.02, -0.03, 0.41))
    R, st = fuse_and_check(dst, src, T, "products")
    assert st["tiles_allocated"] > 0 and st["tiles_touched"] > st["tiles_allocated"], st
    m1 = dst.mesh(only_stale=True)
    r1 = dst.esdf_refresh()
    fresh = _ctx()
    fresh.upload(*dst.download())
    assert sorted(fresh.tile_keys().tolist()) == sorted(dst.tile_keys().tolist())
    _mesh_same(m1, fresh.mesh(), "only_stale after a fuse")
    fs = fresh.esdf_update(**ESDF_CFG)
    all_idx = dst.block_indices()
    assert dst.esdf_blocks(all_idx).tobytes() == fresh.esdf_blocks(all_idx).tobytes()
    for k in ("voxels_observed", "voxels_fixed", "voxels_clamped"):
        assert r1[k] == fs[k], (k, r1, fs)
    assert m1.stats["blocks_meshed"] > 0 and r1["tiles_recomputed"] > 0
    # the source
    _, t2, s2 = src.download(src_before[0])
    assert _same(src.block_indices(), src_before[0]) and t2.tobytes() == src_before[1].tobytes() and s2.tobytes() == src_before[2].tobytes()
    assert _same(src.updated_block_indices(reset=False), src_updated) and src.tile_keys().tolist() == src_keys
    sm1 = src.mesh(only_stale=True)
    assert sm1.stats["blocks_meshed"] == 0 and len(src.mesh_changed_blocks()) == 0
    _mesh_same(sm1, sm0, "the source's stored mesh")
    se1 = src.esdf_refresh()
    assert se1["tiles_stale"] == 0 and se1["tiles_recomputed"] == 0 and all(se1[k] == se0[k] for k in ("voxels_observed", "voxels_fixed", "voxels_clamped")), se1
    for c in (dst, src, fresh):
        c.close()
    return dict(st, meshed=m1.stats["blocks_meshed"], recomputed=r1["tiles_recomputed"])


def case_syncs(spec):
    """After the flags were cleared, the block sync reports the blocks of the touched tiles and the voxel sync exactly the touched voxels."""
    dst, src = _pair(dict(spec, dst_field="random", dst_vps=16))
    assert len(dst.updated_block_indices(reset=True)) > 0
    dst.download_updated_voxels()
    assert len(dst.updated_block_indices(reset=False)) == 0 and len(dst.download_updated_voxels()) == 0
    R, st = fuse_and_check(dst, src, POSES["generic"], "syncs")
    tpb = dst.vps // 8
    want_blocks = np.array(sorted({tuple(c // tpb for c in t) for t in R.tiles_touched}), np.int32).reshape(-1, 3)
    assert _same(dst.updated_block_indices(reset=False), want_blocks)
    v = dst.download_updated_voxels()
    assert len(v) == st["voxels_fused"] == int(R.touched.sum())
    order = np.lexsort((v["linear"], v["block"][:, 2], v["block"][:, 1], v["block"][:, 0]))
    v = v[order]
    j, l = np.nonzero(R.touched)                          # (R.idx is ascending by (x, y, z): the same order)
    assert _same(v["block"], R.idx[j]) and _same(v["linear"], l.astype(np.uint32))
    assert v["tsdf"].tobytes() == R.tsdf[j, l].tobytes() and v["sem"].tobytes() == R.sem[j, l].tobytes()
    assert len(dst.download_updated_voxels()) == 0        # consumed
    assert _same(dst.updated_block_indices(reset=True), np.zeros((0, 3), np.int32))   # (the voxel sync consumed the tiles' flags too)
    dst.close()
    src.close()
    return st


def case_pool_growth(spec):
    src = _ctx()
    src.upload(*sphere_field(8))
    dst = _ctx(max_tiles=64)
    dst.upload(*random_cube(8, 23, lo=0, n=2))
    cap0 = capacity(dst)
    R, st = fuse_and_check(dst, src, POSES["generic"], "pool growth")
    assert st["tiles_allocated"] > cap0 // 2 and capacity(dst) > cap0, (st, cap0, capacity(dst))
    dst.close()
    src.close()
    return dict(st, capacity_before=cap0)


def case_out_of_range(spec):
    from kimera_semantics_amd import binding as B
    dst, src = _pair(dict(spec, dst_field="random"))
    before = dst.download()
    keys = dst.tile_keys().tolist()
    e = refused(B.KS_ERR_INDEX_RANGE, lambda: dst.fuse(src, POSES["far"]))
    assert e.stats["tiles_touched"] == 0 and e.stats["voxels_fused"] == 0, e.stats
    _, t, s = dst.download(before[0])
    assert _same(dst.block_indices(), before[0]) and t.tobytes() == before[1].tobytes() and s.tobytes() == before[2].tobytes()
    assert dst.tile_keys().tolist() == keys
    R, st = fuse_and_check(dst, src, POSES["generic"], "usable afterwards")
    dst.close()
    src.close()
    return st


def case_empty_source(spec):
    dst, src = _ctx(), _ctx()
    dst.upload(*FIELDS["random"](8))
    before = dst.download()
    st = dst.fuse(src, POSES["generic"])
    assert all(v == 0 for v in st.values()), st
    _, t, s = dst.download(before[0])
    assert _same(dst.block_indices(), before[0]) and t.tobytes() == before[1].tobytes() and s.tobytes() == before[2].tobytes()
    # ... and an empty destination with an empty source
    e = _ctx()
    assert all(v == 0 for v in e.fuse(src, POSES["identity"]).values()) and len(e.block_indices()) == 0
    for c in (dst, src, e):
        c.close()
    return st


def case_errors(spec):
    """Point 9 of the contract, on a live context."""
    from kimera_semantics_amd import binding as B
    L = B.lib()
    dst, src = _pair(dict(spec, dst_field="random"))
    before = dst.download()
    cfg, st = B.KsFuseConfig(), B.KsFuseStats()
    assert L.ks_fuse_default_config(ctypes.byref(cfg)) == 0
    T = np.ascontiguousarray(POSES["generic"])
    assert L.ks_fuse_map(None, src._h, T.ctypes.data, ctypes.byref(cfg), None) == B.KS_ERR_INVALID_ARG
    assert L.ks_fuse_map(dst._h, None, T.ctypes.data, ctypes.byref(cfg), None) == B.KS_ERR_INVALID_ARG
    assert L.ks_fuse_map(dst._h, src._h, None, ctypes.byref(cfg), None) == B.KS_ERR_INVALID_ARG
    assert L.ks_fuse_map(dst._h, src._h, T.ctypes.data, None, None) == B.KS_ERR_INVALID_ARG
    refused(B.KS_ERR_INVALID_ARG, lambda: dst.fuse(dst, T))
    other = mesh_case._integrator(0, 64, 48, vps=8, max_tiles=64)
    coarse = B.HipIntegrator(B.default_config(method=0, voxel_size=np.nextafter(np.float32(VOXEL), np.float32(1)), voxels_per_side=8,
                                              truncation_distance=4 * VOXEL, max_tiles=64, max_points=64 * 48))
    refused(B.KS_ERR_INVALID_ARG, lambda: dst.fuse(coarse, T))
    refused(B.KS_ERR_INVALID_ARG, lambda: coarse.fuse(src, T))
    for k in range(7):
        for bad in (float("nan"), float("inf")):
            Tb = T.copy()
            Tb[k] = bad
            refused(B.KS_ERR_INVALID_ARG, lambda: dst.fuse(src, Tb))
    refused(B.KS_ERR_INVALID_ARG, lambda: dst.fuse(src, [0, 0, 0, 0, 0.1, 0.2, 0.3]))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(B.KS_ERR_INVALID_ARG, lambda: dst.fuse(src, T, min_weight=bad))
    # none of these changed the map
    _, t, s = dst.download(before[0])
    assert _same(dst.block_indices(), before[0]) and t.tobytes() == before[1].tobytes() and s.tobytes() == before[2].tobytes()
    # a quaternion that is not of unit length is normalised
    R, st = fuse_and_check(other, src, T, "unit quaternion")
    again = mesh_case._integrator(0, 64, 48, vps=8, max_tiles=64)
    T3 = T.copy()
    T3[:4] *= np.float32(2.0)                              # (exact in f32 and in f64)
    assert again.fuse(src, T3) == st
    assert_map(again, R, "scaled quaternion")
    # stats may be NULL
    assert L.ks_fuse_map(dst._h, src._h, T.ctypes.data, ctypes.byref(cfg), None) == 0
    # a marcher context of the exact multi-GPU mode holds no voxel data
    marcher, owner = (mesh_case._integrator(1, 64, 48) for _ in range(2))
    f = mesh_case._frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    wide = mesh_case._integrator(1, 64, 48)
    refused(B.KS_ERR_UNSUPPORTED, lambda: marcher.fuse(owner, T))
    refused(B.KS_ERR_UNSUPPORTED, lambda: wide.fuse(marcher, T))
    assert wide.fuse(owner, T)["voxels_fused"] > 0           # (the owner holds the map)
    for c in (dst, src, other, coarse, again, marcher, owner, wide):
        c.close()
    return st


CASES = {"pose": case_pose, "holes": case_holes, "chunked": case_chunked, "upload_order": case_upload_order, "in_flight": case_in_flight,
         "products": case_products, "syncs": case_syncs, "pool_growth": case_pool_growth, "out_of_range": case_out_of_range,
         "empty_source": case_empty_source, "errors": case_errors}

# name -> spec: the same cases in both tiers
SPECS = {
    "identity_empty": dict(case="pose", pose="identity"),
    "shift_voxels": dict(case="pose", pose="shift_voxels"),
    "shift_half": dict(case="pose", pose="shift_half"),
    "yaw90": dict(case="pose", pose="yaw90"),
    "generic_empty": dict(case="pose", pose="generic"),
    "generic_vps": dict(case="pose", pose="generic", src_vps=8, dst_vps=16),
    # blocks of 4^3 tiles on both sides, {-1, 0}^3 each: a block expands to 64 tile keys, negative ones among them
    "generic_vps32": dict(case="pose", pose="generic", src_vps=32, dst_vps=32),
    "overlap_color": dict(case="pose", pose="generic", dst_field="random", color_mode=0),
    "overlap_prob": dict(case="pose", pose="generic", dst_field="random", color_mode=2),
    "holes": dict(case="holes"),
    "chunked": dict(case="chunked"),
    "upload_order": dict(case="upload_order"),
    "in_flight": dict(case="in_flight"),
    "products": dict(case="products"),
    "syncs": dict(case="syncs"),
    "pool_growth": dict(case="pool_growth"),
    "out_of_range": dict(case="out_of_range"),
    "empty_source": dict(case="empty_source"),
    "errors": dict(case="errors"),
}


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("FUSE_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
