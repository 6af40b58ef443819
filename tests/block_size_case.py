"""One map, four block sizes, shared by both tiers: run_case(spec) drives whatever library the binding has loaded — the GPU tier
(tests/test_block_size_invariance_gpu.py) calls it in-process, the CPU tier (tests/test_block_size_invariance_cpu.py) runs it
as a child process on the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.block_size_case '<json spec>'

mesh_case.same_map(vps) cuts ONE voxel content into blocks of 8^3, 16^3, 32^3 or 64^3 voxels: the resident tiles are the same
1024 at every size, so whatever a reader of the map returns may depend on voxels_per_side through its block layout alone.
collect(vps) uploads the map and runs every reader; what comes back in blocks is put back into global voxel coordinates.  The
result at 8 voxels per side is checked against the NumPy models (the yardsticks of the per-module tests), and the results at 16,
32 and 64 are compared with it: byte for byte, except where the contract orders by block (the mesh: as multisets, with its own
order rule checked per size) and the object ids (up to a bijection).

Two more cases live here because they are about the block size and nothing else: case_upload_limits (both tiers: ks_upload_blocks at
the rim of the packed tile-key range, whose limit in blocks is 2^17 / (vps / 8)) and case_chunks (GPU tier only, by design: it moves
about 330 MB each way through the 256 MiB staging chunks of ks_upload_blocks / ks_download_blocks, which no other test fills)."""
import json
import os
import sys

import numpy as np

from tests import mesh_case, render_case

VOXEL = mesh_case.VOXEL
ECFG = dict(min_distance_m=0.1, max_distance_m=0.4)
RADIUS = 0.15
SHIFT = np.array([0.0, 1.6, 1.6], np.float32)          # render_case's cameras look at the origin; the map's sphere sits here
CAMERA_NAMES = ("front", "corner")
VIEW_K, VIEW_SIZE, VIEW_CFG = (8.0, 8.0, 7.5, 5.5), (16, 12), dict(max_range_m=2.0)
_REF = {}                                              # the vps-8 result: computed and model-checked once per process


def cameras():
    out = []
    for name in CAMERA_NAMES:
        T = render_case.CAMERAS[name].copy()
        T[4:7] += SHIFT
        out.append(T)
    return out


def pocket_centre():
    return np.array([[(a + b) * 0.5 * VOXEL for a, b in mesh_case.SAME_MAP_POCKET]], np.float32)


def sample_points():
    """Points all over the box and a little beyond, off the grid; some exactly on block seams."""
    rng = np.random.default_rng(17)
    lo = np.array([b[0] for b in mesh_case.SAME_MAP_BOX]) - 2.0
    hi = np.array([b[1] for b in mesh_case.SAME_MAP_BOX]) + 2.0
    p = (rng.uniform(lo, hi, (4096, 3)) * VOXEL).astype(np.float32)
    p[:64, 0] = 0.0                                    # the seam x = 0 of every block size
    p[64:128, 1] = np.float32(32 * VOXEL)              # a seam of 8, 16 and 32, the middle of a block of 64
    return p


def polyline():
    """A staircase through the free pocket, one voxel per step, then a long diagonal back: (waypoints (1, m, 3), n_waypoints)."""
    (x0, x1), (y0, y1), (z0, _) = mesh_case.SAME_MAP_POCKET
    vox, z = [], z0 + 8
    for k in range(20):
        vox += [(x0 + 4 + k, y0 + 4 + k, z), (x0 + 5 + k, y0 + 4 + k, z)]
    vox.append((x0 + 6, y1 - 6, z + 20))
    wp = ((np.array(vox, np.float64) + 0.5) * VOXEL).astype(np.float32)[None]
    return wp, np.array([wp.shape[1]], np.uint32)


def view_poses():
    from kimera_semantics_amd import binding as B
    at = np.concatenate([pocket_centre(), np.array([[0.3, 1.6, 0.3]], np.float32)])
    return B.view_gain_yaw_poses(at, 4)


def _triangles(m):
    """One row of bytes per triangle of a Mesh: xyz, normals, rgba and labels of its three corners; sorted."""
    n = len(m.xyz) // 3
    row = np.concatenate([np.ascontiguousarray(m.xyz).view(np.uint8).reshape(n, 36), np.ascontiguousarray(m.normals).view(np.uint8).reshape(n, 36),
                          np.ascontiguousarray(m.rgba).reshape(n, 12), np.ascontiguousarray(m.labels).reshape(n, 3)], axis=1)
    return np.sort(np.ascontiguousarray(row).view("V87").reshape(-1)).tobytes()


def _vertices(im):
    n = im.n_vertices
    row = np.concatenate([np.ascontiguousarray(im.xyz).view(np.uint8).reshape(n, 12), np.ascontiguousarray(im.normals).view(np.uint8).reshape(n, 12),
                          np.ascontiguousarray(im.rgba).reshape(n, 4), np.ascontiguousarray(im.labels).reshape(n, 1)], axis=1)
    return np.sort(np.ascontiguousarray(row).view("V29").reshape(-1)).tobytes()


def _ascending(blocks):
    b = np.asarray(blocks, np.int64).reshape(-1, 3)
    return all(tuple(b[i]) < tuple(b[i + 1]) for i in range(len(b) - 1))


def collect(vps, check_models=False):
    """Every reader of the map on same_map(vps); with check_models each against its NumPy model as well."""
    from kimera_semantics_amd import binding as B
    g = mesh_case._integrator(0, 64, 48, vps=vps)
    idx, t, s = mesh_case.same_map(vps)
    g.upload(idx, t, s)
    out = {}
    unblock = lambda rows: mesh_case.from_blocks(bi, rows, vps)
    bi = g.block_indices()
    assert len(g.tile_keys()) == mesh_case.SAME_MAP_TILES and len(bi) == len(idx) and _ascending(bi), (vps, len(g.tile_keys()), len(bi))
    # download(): what went up, voxel for voxel
    _, dt, ds = g.download()
    _, t0, s0 = mesh_case.same_map_voxels()
    out["tsdf"], out["sem"] = unblock(dt), unblock(ds)
    assert out["tsdf"].tobytes() == t0.tobytes() and out["sem"].tobytes() == s0.tobytes(), "download() differs from the upload"
    # render: the kernel never sees vps
    views = [g.render(T, render_case.K_EVEN, 64, 48) for T in cameras()]
    out["render"] = [render_case._bytes(v) for v in views]
    # mesh and indexed mesh
    mesh = g.mesh()
    assert _ascending(mesh.blocks["block"]) and int(mesh.blocks["n_vertices"].sum()) == 3 * mesh.n_triangles == len(mesh.xyz), vps
    assert (mesh.blocks["first_vertex"] == np.concatenate([[0], np.cumsum(mesh.blocks["n_vertices"])[:-1]])).all()
    assert mesh.stats["blocks_total"] == len(bi) and mesh.stats["triangles_total"] == mesh.n_triangles
    out["n_triangles"], out["triangles"] = mesh.n_triangles, _triangles(mesh)
    im = g.mesh_index()
    assert np.ascontiguousarray(im.xyz[im.indices]).tobytes() == np.ascontiguousarray(mesh.xyz).tobytes()
    out["n_vertices"], out["vertices"] = im.n_vertices, _vertices(im)
    # objects (before the ESDF: they read the TSDF)
    orec, ost = g.objects()
    out["object_ids"], out["object_records"], out["object_stats"] = unblock(g.object_ids(bi)), orec, ost
    # ESDF and its reads
    est = g.esdf_update(**ECFG)
    ref = g.esdf_refresh()
    assert ref["tiles_total"] == mesh_case.SAME_MAP_TILES and ref["tiles_stale"] == 0, ref          # the same residency at every size
    out["esdf"] = unblock(g.esdf_blocks(bi))
    out["esdf_stats"] = {k: est[k] for k in ("voxels_observed", "voxels_fixed", "voxels_clamped", "box_voxels")}
    out["sample"] = g.esdf_sample(sample_points())
    wp, nw = polyline()
    out["shorten"] = g.shorten_paths(wp, nw, radius_m=RADIUS)
    vrec, vst = g.view_gain(view_poses(), VIEW_K, *VIEW_SIZE, **VIEW_CFG)
    out["view_gain"] = (vrec, vst)
    # cost-to-go and frontiers
    nst = g.nav_update(pocket_centre(), radius_m=RADIUS)
    out["nav"] = unblock(g.nav_blocks(bi))
    frec, fst = g.frontiers(radius_m=RADIUS)
    out["frontier_ids"], out["frontier_records"] = unblock(g.frontier_ids(bi)), frec
    out["frontier_stats"] = fst
    if check_models:
        _check_models(g, out, views, mesh, im, (orec, ost), est, nst, (frec, fst), wp, nw)
    g.close()
    return out


def _check_models(g, out, views, mesh, im, objects, est, nst, frontiers, wp, nw):
    from tests import (esdf_model, esdf_read_model, frontier_model, mesh_index_model, mesh_model, nav_model, objects_model, path_shorten_model,
                       render_model, view_gain_model)
    bi = g.block_indices()
    for T, v in zip(cameras(), views):
        render_model.assert_same(v, render_model.model_of(g, T, render_case.K_EVEN, 64, 48), "render")
        assert v[4]["pixels_hit"] > 64 * 48 // 8 and v[4]["pixels_missed"] > 0, v[4]
    mesh_model.assert_same(mesh, mesh_model.model_of(g), "mesh")
    assert mesh.n_triangles > 4000 and set(np.unique(mesh.labels)) == {3, 7}, mesh.n_triangles
    mesh_index_model.assert_same(im, mesh_index_model.index_of(mesh), "indexed mesh")
    om = objects_model.model_of(g)
    objects_model.assert_same(objects, om, bi, g.object_ids(bi), "objects")
    assert objects[1]["objects"] >= 2, objects[1]
    em = esdf_model.model_of(g, ECFG)
    esdf_model.assert_same(g.esdf_blocks(bi), em.blocks(bi), "esdf")
    for k in ("voxels_observed", "voxels_fixed", "voxels_clamped"):
        assert est[k] == em.stats[k], (k, est, em.stats)
    assert est["voxels_fixed"] > 10000
    store = esdf_read_model.store_of(g)
    want = esdf_read_model.sample(store, sample_points(), VOXEL)
    esdf_read_model.assert_same(out["sample"], want, "esdf_sample")
    assert min(want["stats"].values()) > 100, want["stats"]
    ps = path_shorten_model.shorten(store, wp, nw, VOXEL, radius_m=RADIUS)
    path_shorten_model.assert_same(out["shorten"], ps, "path_shorten")
    assert ps["status"][0] == 0 and ps["n_waypoints"][0] < nw[0], (ps["status"], ps["n_waypoints"])
    vg = view_gain_model.model_of(g, view_poses(), VIEW_K, width=VIEW_SIZE[0], height=VIEW_SIZE[1], **VIEW_CFG)
    view_gain_model.assert_same(out["view_gain"], vg, "view_gain")
    assert out["view_gain"][1]["unknown_voxels"] > 0 and out["view_gain"][1]["free_voxels"] > 0
    field = nav_model.field(store, pocket_centre(), VOXEL, radius_m=RADIUS)
    nav_model.assert_field(g, nst, field, "nav")
    assert nst["voxels_reached"] > 20000 and nst["goals_used"] == 1, nst
    fm = frontier_model.model_of(g, field, radius_m=RADIUS)
    frontier_model.assert_same(frontiers, fm, bi, g.frontier_ids(bi), "frontiers")
    assert frontiers[1]["frontiers"] >= 1 and frontiers[1]["nav_field_used"] == 1, frontiers[1]


def same_partition(a, b, none=0xffffffff):
    """Two id fields over the same voxels describe the same partition: a bijection between the ids, none onto none; returns it."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    assert ((a == none) == (b == none)).all(), "the voxels without an id differ"
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    assert len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1])), "the ids do not map one to one"
    return pairs


def compare(ref, got, vps):
    what = "vps %d against vps 8: " % vps
    for k in ("tsdf", "sem", "esdf", "nav", "frontier_ids"):
        a, b = ref[k], got[k]
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a != b)
            raise AssertionError(what + "%s differs at %d voxels, first (z, y, x) = %s: %r vs %r" % (k, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])]))
    assert ref["render"] == got["render"], what + "render"
    assert (ref["n_triangles"], ref["n_vertices"]) == (got["n_triangles"], got["n_vertices"]), (what, got["n_triangles"], got["n_vertices"])
    assert ref["triangles"] == got["triangles"], what + "the triangles differ as a multiset"
    assert ref["vertices"] == got["vertices"], what + "the shared vertices differ as a multiset"
    assert ref["esdf_stats"] == got["esdf_stats"], (what, ref["esdf_stats"], got["esdf_stats"])
    from tests import esdf_read_model, path_shorten_model
    esdf_read_model.assert_same(got["sample"], ref["sample"], what + "esdf_sample")
    path_shorten_model.assert_same(got["shorten"], dict(ref["shorten"]), what + "path_shorten")
    assert got["view_gain"][0].tobytes() == ref["view_gain"][0].tobytes() and got["view_gain"][1] == ref["view_gain"][1], what + "view_gain"
    assert got["frontier_records"].tobytes() == ref["frontier_records"].tobytes() and got["frontier_stats"] == ref["frontier_stats"], what + "frontiers"
    # objects: the same partition (ids up to a bijection), the same voxel count per instance
    pairs = same_partition(ref["object_ids"], got["object_ids"])
    pairs = pairs[pairs[:, 0] != 0xffffffff]
    assert len(pairs) == len(ref["object_records"]) == len(got["object_records"]), (what, len(pairs))
    assert (ref["object_records"]["n_voxels"][pairs[:, 0]] == got["object_records"]["n_voxels"][pairs[:, 1]]).all(), what + "object sizes"
    for k in ("voxels_surface", "components", "objects", "voxels_in_objects", "largest_object_voxels"):
        assert ref["object_stats"][k] == got["object_stats"][k], (what, k)


TILE_BIAS = 1 << 17     # tile coordinates are packed as 18-bit fields: a block of (vps / 8)^3 tiles has its index within +-TILE_BIAS / (vps / 8)


def _coordinate_field(idx, vps):
    """Blocks whose voxels carry their own global coordinate: distance = x + 1024 (y mod 1024) + 2^20 (z mod 8) (exact in f32 for
    |x| < 2^20 ... as an integer below 2^24), priors[0] = -distance, weight 1; vectorised."""
    from kimera_semantics_amd import binding as B
    idx = np.asarray(idx, np.int32).reshape(-1, 3)
    lin = np.arange(vps ** 3, dtype=np.int64)
    local = np.stack([lin % vps, (lin // vps) % vps, lin // (vps * vps)], axis=1)
    gv = idx[:, None, :].astype(np.int64) * vps + local[None]
    value = (np.mod(gv[..., 0], 1 << 10) + 1024 * np.mod(gv[..., 1], 1 << 10) + (1 << 20) * np.mod(gv[..., 2], 8)).astype(np.float32)
    t, s = np.zeros(value.shape, B.TSDF_DTYPE), np.zeros(value.shape, B.SEM_DTYPE)
    t["distance"], t["weight"] = value, 1.0
    s["priors"][..., 0] = -value
    s["label"] = (np.mod(gv.sum(axis=-1), 21)).astype(np.uint8)
    s["color"] = mesh_case._label_colors()[s["label"]]      # (download() derives the semantic colour from the label)
    return idx, t, s


def _state(g):
    bi = g.block_indices()
    _, t, s = g.download(bi)
    return bi.tobytes(), np.sort(g.tile_keys()).tobytes(), t.tobytes(), s.tobytes()


def case_upload_limits(spec):
    """ks_upload_blocks at the rim of the packed tile-key range: the last block index on either side is taken and reads back, the
    first one beyond is KS_ERR_INDEX_RANGE and leaves the map as it was."""
    from kimera_semantics_amd import binding as B
    vps = spec["vps"]
    tpb = vps // 8
    lim = TILE_BIAS // tpb
    g = mesh_case._integrator(0, 64, 48, vps=vps)
    idx, t, s = _coordinate_field([(lim - 1, lim - 1, lim - 1), (-lim, -lim, -lim), (lim - 1, 0, -lim)], vps)
    g.upload(idx, t, s)
    keys = g.tile_keys()
    assert len(keys) == 3 * tpb ** 3 and len(np.unique(keys)) == len(keys), len(keys)
    bi = g.block_indices()
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
    assert bi.tobytes() == idx[order].tobytes(), bi
    _, dt, ds = g.download(idx)
    assert dt.tobytes() == t.tobytes() and ds.tobytes() == s.tobytes(), "the blocks at the rim do not read back"
    before = _state(g)
    fine = np.array([0, 0, 0], np.int32)
    for bad in ((lim, 0, 0), (0, -lim - 1, 0), (0, 0, lim), (-lim - 1, lim - 1, 0)):
        pair = np.array([fine, bad], np.int32)
        pi, pt, ps = _coordinate_field(pair, vps)
        try:
            g.upload(pi, pt, ps)
            raise AssertionError("block index %r accepted at %d voxels per side" % (bad, vps))
        except B.KsError as e:
            assert e.code == B.KS_ERR_INDEX_RANGE, (bad, e)
        assert _state(g) == before, "a refused upload changed the map"
    g.close()
    return dict(lim=lim)


def case_chunks(spec):
    """GPU tier only (about 330 MB each way): more blocks than one staging chunk of ks_upload_blocks / ks_download_blocks holds
    (256 MiB / (vps^3 * 92 B): 11 blocks at 64, 89 at 32), every voxel carrying its own coordinate."""
    import time
    from kimera_semantics_amd import binding as B
    vps, n = spec["vps"], spec["blocks"]
    chunk = (256 << 20) // (vps ** 3 * 92)
    assert chunk < n <= 2 * chunk
    idx = np.array([(x, 0, 0) for x in range(-(n // 2), n - n // 2)], np.int32)
    idx, t, s = _coordinate_field(idx, vps)
    g = mesh_case._integrator(0, 64, 48, vps=vps, max_tiles=2 * n * (vps // 8) ** 3)
    t0 = time.perf_counter()
    g.upload(idx, t, s)
    t1 = time.perf_counter()
    _, dt, ds = g.download(idx)
    t2 = time.perf_counter()
    print("chunk loop at %d voxels per side, %d blocks (chunks of %d): upload %.1f ms, download %.1f ms" % (vps, n, chunk, 1e3 * (t1 - t0), 1e3 * (t2 - t1)))
    assert dt["distance"].tobytes() == t["distance"].tobytes(), "distance differs after the round trip"
    assert ds["priors"][..., 0].tobytes() == s["priors"][..., 0].tobytes(), "priors[0] differs after the round trip"
    assert dt.tobytes() == t.tobytes() and ds.tobytes() == s.tobytes()
    only = np.zeros_like(dt)
    g._chk(B.lib().ks_download_blocks(g._h, idx.ctypes.data, len(idx), only.ctypes.data, None))
    assert only.tobytes() == t.tobytes(), "the tsdf-only download differs"
    _, rt, rs = g.download(idx[::-1])
    assert rt.tobytes() == t[::-1].tobytes() and rs.tobytes() == s[::-1].tobytes(), "the download in reversed order differs"
    g.close()
    return dict(upload_s=t1 - t0, download_s=t2 - t1)


def reference():
    if "ref" not in _REF:
        _REF["ref"] = collect(8, check_models=True)
    return _REF["ref"]


def run_case(spec):
    if spec.get("case") == "upload_limits":
        return case_upload_limits(spec)
    ref = reference()
    if spec["vps"] != 8:
        compare(ref, collect(spec["vps"]), spec["vps"])
    return dict(triangles=ref["n_triangles"], vertices=ref["n_vertices"], objects=len(ref["object_records"]), frontiers=len(ref["frontier_records"]))


# name -> spec: the same cases in both tiers ("vps8" is the model check alone; every other case repeats it in its own process on
# the functional model, and takes it from the cache on the GPU)
SPECS = {"vps%d" % v: dict(vps=v) for v in (8, 16, 32, 64)}
SPECS.update({"upload_limits_vps%d" % v: dict(case="upload_limits", vps=v) for v in (8, 16, 32, 64)})


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("BLOCK_SIZE_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
