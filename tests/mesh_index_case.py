"""The indexed-mesh cases, shared by both tiers: run_case(spec) drives whatever library the binding has loaded —
the GPU tier (tests/test_mesh_index_gpu.py) calls it in-process, the CPU tier (tests/test_mesh_index_cpu.py) runs it as a child
process on the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.mesh_index_case '<json spec>'
The checker is tests/mesh_index_model.py (NumPy, written from the contract), applied to the unshared mesh the same context
stores (tests/mesh_case.py ties that to the mesh model).  Every comparison is exact and nothing is left out."""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

from tests import mesh_index_model as IM
from tests.mesh_case import VOXEL, _frames, _integrator, make_field

NONE = 0xffffffff
ARRAYS = ("xyz", "normals", "rgba", "labels", "object_ids", "indices")


def _bytes(im):
    return b"".join(np.ascontiguousarray(getattr(im, k)).tobytes() for k in ARRAYS) + im.blocks.tobytes()


def check(g, mesh, what, expect_ids=None):
    """mesh = what g.mesh() just returned: the index of the stored mesh against the model, and the properties of §18."""
    im = g.mesh_index()
    model = IM.index_of(mesh)
    assert model["agree"], what + ": corners of one position disagree on colour or label in the UNSHARED mesh"
    IM.assert_same(im, model, what)
    assert im.blocks.tobytes() == mesh.blocks.tobytes(), what
    assert im.n_triangles == mesh.n_triangles and im.n_vertices == im.stats["vertices"] and len(im.indices) == im.stats["corners"] == len(mesh.xyz)
    # xyz[indices] is the unshared mesh; the vertices are pairwise distinct; the order rule
    assert np.ascontiguousarray(im.xyz[im.indices]).tobytes() == np.ascontiguousarray(mesh.xyz).tobytes(), what
    assert len(np.unique(np.ascontiguousarray(im.xyz).view(np.uint32).reshape(-1, 3), axis=0)) == im.n_vertices, what
    if len(im.indices):
        run_max = np.maximum.accumulate(im.indices.astype(np.int64))
        assert im.indices[0] == 0 and (np.diff(run_max) <= 1).all() and run_max[-1] == im.n_vertices - 1, what
        tri = im.indices.reshape(-1, 3)
        assert (tri[:, 0] != tri[:, 1]).all() and (tri[:, 1] != tri[:, 2]).all() and (tri[:, 0] != tri[:, 2]).all(), what
        assert im.stats["workspace_bytes"] > 0
    if expect_ids is None:
        assert (im.object_ids == NONE).all(), what
    else:
        assert im.object_ids.tobytes() == expect_ids(im.xyz).tobytes(), what
    return im


def case_upload(spec):
    g = _integrator(0, 64, 48, vps=spec["vps"])
    g.upload(*make_field(spec["field"], spec["vps"]))
    mesh = g.mesh()
    im = check(g, mesh, spec["field"])
    assert im.stats["vertices"] < im.stats["corners"] / 3 and im.stats["corners"] > 1500, im.stats
    again = g.mesh_index()
    assert _bytes(again) == _bytes(im) and again.stats == im.stats
    if spec["field"] == "two_label":
        assert set(np.unique(im.labels)) == {3, 7}
    g.close()
    return dict(im.stats)


def grid_field(kind, vps=8):
    """2 x 2 x 2 blocks around the origin; the distance is a function of the global voxel index (gx, gy, gz)."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    idx = np.array(list(itertools.product((-1, 0), repeat=3)), dtype=np.int32)
    lin = np.arange(vps ** 3)
    local = np.stack([lin % vps, (lin // vps) % vps, lin // (vps * vps)], axis=1)
    gv = idx[:, None, :].astype(np.int64) * vps + local[None]
    gx, gy, gz = (gv[..., k].astype(np.float32) for k in range(3))
    vs = np.float32(VOXEL)
    if kind == "exact_zeros":      # vertices exactly on voxel centres, reached from edges of two axes
        dist = (gx + gy) * vs
    elif kind == "plus_zero":      # t = 0.5 between the centres at -voxel / 2 and +voxel / 2: x = +0.0
        dist = (gx + np.float32(0.5)) * vs
    elif kind == "empty":          # no sign change anywhere
        dist = np.ones_like(gx)
    else:
        raise ValueError(kind)
    t = np.zeros(dist.shape, dtype=B.TSDF_DTYPE)
    s = np.zeros(dist.shape, dtype=B.SEM_DTYPE)
    assert dist.dtype == np.float32
    t["distance"], t["weight"] = dist, 1.0
    label = np.where(gz < 0, 3, 7).astype(np.uint8)
    lut = synth.default_label_colors()
    t["color"] = lut[label]
    s["label"], s["color"] = label, lut[label]
    s["priors"] = np.float32(-0.60205999132)
    np.put_along_axis(s["priors"], label[..., None].astype(np.int64), np.float32(-0.1), axis=-1)
    return idx, t, s


def case_grid(spec):
    from kimera_semantics_amd import binding as B
    g = _integrator(0, 64, 48, vps=8)
    g.upload(*grid_field(spec["field"]))
    mesh = g.mesh()
    im = check(g, mesh, spec["field"])
    if spec["field"] == "exact_zeros":
        # (counted with the NumPy mesh model: 480 kept triangles, 390 degenerate ones dropped, 1440 corners -> 272 vertices)
        assert mesh.stats["degenerate_dropped"] == 390 and (im.stats["corners"], im.stats["vertices"]) == (1440, 272), (mesh.stats, im.stats)
        centre = (np.round(im.xyz / np.float32(VOXEL) - np.float32(0.5)).astype(np.float32) + np.float32(0.5)) * np.float32(VOXEL)
        assert (centre == im.xyz).all(axis=1).any()          # vertices that ARE voxel centres
        assert set(np.unique(im.labels)) == {3, 7}
    elif spec["field"] == "plus_zero":
        assert im.n_vertices > 0 and (np.ascontiguousarray(im.xyz[:, 0]).view(np.uint32) == 0).all()   # +0.0, not -0.0
    else:
        assert mesh.n_triangles == 0 and im.stats == dict(corners=0, vertices=0, max_corners_per_vertex=0, workspace_bytes=0), im.stats
        L, nv, ni = B.lib(), C.c_size_t(7), C.c_size_t(7)
        assert L.ks_mesh_index_size(g._h, C.byref(nv), C.byref(ni)) == 0 and nv.value == 0 and ni.value == 0
        one = np.zeros(4, np.uint32)
        assert L.ks_mesh_index_download(g._h, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, 0, one.ctypes.data, 0) == 0
        assert not one.any()
    g.close()
    return dict(im.stats)


def case_integrated(spec):
    pipeline = spec.get("pipeline", 0)
    g = _integrator(spec["method"], 64, 48, pipeline=pipeline)
    frames = _frames(3, 64, 48)
    for f in frames[:2]:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    mesh = g.mesh()
    im = check(g, mesh, "integrated")
    assert len(np.unique(im.labels)) >= 2 and im.n_triangles >= 300
    if pipeline:
        # a frame in flight when the index is built: the call completes it, and still indexes the mesh that is STORED
        f = frames[2]
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        again = g.mesh_index()
        assert _bytes(again) == _bytes(im)
        check(g, g.mesh(only_stale=True), "after the third frame")
    g.close()
    return dict(im.stats)


def case_objects(spec):
    g = _integrator(0, 64, 48, vps=8)
    g.upload(*make_field("two_label", 8))
    mesh = g.mesh()
    check(g, mesh, "no object store")          # every id KS_OBJECT_NONE, and no error
    rec, st = g.objects()
    assert st["objects"] >= 2
    im = check(g, mesh, "objects stored", expect_ids=g.object_query)
    ids = set(np.unique(im.object_ids).tolist())
    assert len(ids - {NONE}) >= 2, ids
    g.close()
    return dict(ids=len(ids))


def _refused(g):
    from kimera_semantics_amd import binding as B
    L, nv, ni = B.lib(), C.c_size_t(), C.c_size_t()
    a = L.ks_mesh_index_size(g._h, C.byref(nv), C.byref(ni))
    b = L.ks_mesh_index_download(g._h, None, None, None, None, None, 0, None, 0)
    return a == b == B.KS_ERR_INVALID_ARG


def case_lifetime(spec):
    f1, f2 = _frames(2, 64, 48, step=40, hfov=50.0)
    g = _integrator(0, 64, 48)
    g.integrate(f1.T_G_C, f1.xyz, f1.rgba, f1.labels)
    im1 = check(g, g.mesh(), "frame 1")
    g.integrate(f2.T_G_C, f2.xyz, f2.rgba, f2.labels)
    assert _bytes(g.mesh_index(build=False)) == _bytes(im1)      # integrating leaves the snapshot
    m2 = g.mesh(only_stale=True)
    assert _refused(g)                                           # the update dropped it
    im2 = check(g, m2, "re-index after the refresh")
    assert _bytes(im2) != _bytes(im1)
    try:
        g.mesh(min_weight=-1.0)
        raise AssertionError("min_weight -1 accepted")
    except Exception as e:
        assert getattr(e, "code", None) == -1, e
    assert _refused(g)                                           # a failed update drops it too
    m2 = g.mesh()
    im2 = check(g, m2, "after the failed update")
    # removal of blocks leaves the stored mesh and its index until the next update
    blocks = g.block_indices()
    st = g.remove_blocks(blocks[: max(1, len(blocks) // 4)])
    assert st["blocks_removed"] >= 1, st
    assert _bytes(g.mesh_index(build=False)) == _bytes(im2)
    assert _bytes(g.mesh_index()) == _bytes(im2)                 # and a new index of the (unchanged) stored mesh is the same
    m3 = g.mesh(only_stale=True)
    assert _refused(g)
    check(g, m3, "after the removal")
    g.clear()
    assert _refused(g)
    from kimera_semantics_amd import binding as B
    assert B.lib().ks_mesh_index(g._h, None) == B.KS_ERR_INVALID_ARG    # no stored mesh after the clear
    g.close()
    # the same blocks uploaded in another order: the same bytes
    idx, t, s = make_field("holes", 8)
    perm = np.random.default_rng(5).permutation(len(idx))
    out = []
    for order in (np.arange(len(idx)), perm):
        h = _integrator(0, 64, 48, vps=8)
        h.upload(idx[order], t[order], s[order])
        out.append(_bytes(check(h, h.mesh(), "upload order")))
        h.close()
    assert out[0] == out[1]
    return {}


def case_read_only(spec):
    f1, f2 = _frames(2, 64, 48)
    g = _integrator(1, 64, 48)
    for f in (f1, f2):
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.esdf_update(min_distance_m=0.1, max_distance_m=0.4)
    rec, _ = g.objects()
    mesh = g.mesh()
    upd = g.updated_block_indices(reset=False)
    assert len(upd)
    im = check(g, mesh, "read-only", expect_ids=g.object_query)
    assert g.updated_block_indices(reset=False).tobytes() == upd.tobytes()
    m2 = g.mesh(only_stale=True)
    assert m2.stats["blocks_meshed"] == 0, m2.stats
    for k in ("xyz", "normals", "rgba", "labels", "blocks"):
        assert getattr(m2, k).tobytes() == getattr(mesh, k).tobytes(), k
    assert _bytes(g.mesh_index()) == _bytes(im)
    assert g.esdf_refresh()["tiles_stale"] == 0
    assert g.object_records().tobytes() == rec.tobytes()
    g.close()
    return {}


def case_errors(spec):
    from kimera_semantics_amd import binding as B
    L = B.lib()
    g = _integrator(0, 64, 48, vps=8)
    g.upload(*make_field("plane", 8))
    st = B.KsMeshIndexStats(corners=5, vertices=6, max_corners_per_vertex=7, workspace_bytes=8)
    nv, ni = C.c_size_t(), C.c_size_t()
    # no stored mesh; no index
    assert L.ks_mesh_index(g._h, C.byref(st)) == B.KS_ERR_INVALID_ARG and (st.corners, st.vertices, st.max_corners_per_vertex, st.workspace_bytes) == (0, 0, 0, 0)
    assert _refused(g)
    mesh = g.mesh()
    assert _refused(g)                      # a stored mesh, but no index built yet
    assert L.ks_mesh_index(g._h, None) == 0    # stats may be NULL
    im = g.mesh_index()
    assert L.ks_mesh_index_size(g._h, None, None) == 0
    assert L.ks_mesh_index_size(g._h, C.byref(nv), C.byref(ni)) == 0 and (nv.value, ni.value) == (im.n_vertices, len(im.indices))
    V, Cn = im.n_vertices, len(im.indices)
    bufs = dict(xyz=np.zeros((V, 3), np.float32), normals=np.zeros((V, 3), np.float32), rgba=np.zeros((V, 4), np.uint8), labels=np.zeros(V, np.uint8),
                object_ids=np.zeros(V, np.uint32), indices=np.zeros(Cn, np.uint32))
    # each too-small capacity, with every single output
    for k in ARRAYS[:5]:
        args = [bufs[n].ctypes.data if n == k else None for n in ARRAYS[:5]]
        assert L.ks_mesh_index_download(g._h, *args, V - 1, None, 0) == B.KS_ERR_INVALID_ARG, k
    assert L.ks_mesh_index_download(g._h, None, None, None, None, None, 0, bufs["indices"].ctypes.data, Cn - 1) == B.KS_ERR_INVALID_ARG
    assert L.ks_mesh_index_download(g._h, bufs["xyz"].ctypes.data, None, None, None, None, V, bufs["indices"].ctypes.data, Cn - 1) == B.KS_ERR_INVALID_ARG
    # every subset of NULL outputs: what is asked for arrives, what is not stays untouched
    for mask in range(64):
        for b in bufs.values():
            b[...] = 0xAB if b.dtype == np.uint8 else 7
        want = [k for i, k in enumerate(ARRAYS) if (mask >> i) & 1]
        args = [bufs[k].ctypes.data if k in want else None for k in ARRAYS[:5]]
        assert L.ks_mesh_index_download(g._h, *args, V if any(a is not None for a in args) else 0, bufs["indices"].ctypes.data if "indices" in want else None,
                                        Cn if "indices" in want else 0) == 0, mask
        for k in ARRAYS:
            if k in want:
                assert bufs[k].tobytes() == np.ascontiguousarray(getattr(im, k)).tobytes(), (mask, k)
            else:
                assert (bufs[k] == (0xAB if bufs[k].dtype == np.uint8 else 7)).all(), (mask, k)
    g.close()
    # a marcher context of the exact multi-GPU mode holds no voxel data
    marcher, owner = (_integrator(1, 64, 48) for _ in range(2))
    f = _frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    st = B.KsMeshIndexStats(corners=5)
    assert L.ks_mesh_index(marcher._h, C.byref(st)) == B.KS_ERR_UNSUPPORTED and st.corners == 0
    assert L.ks_mesh_index_size(marcher._h, C.byref(nv), C.byref(ni)) == B.KS_ERR_UNSUPPORTED
    assert L.ks_mesh_index_download(marcher._h, None, None, None, None, None, 0, None, 0) == B.KS_ERR_UNSUPPORTED
    check(owner, owner.mesh(), "the owner holds the map")
    marcher.close()
    owner.close()
    # a context in a failed state (the pool is full: sticky until a clear)
    small = _integrator(0, 64, 48, max_tiles=8)
    assert small.mesh().n_triangles == 0 and small.mesh_index().n_vertices == 0     # an empty map: a stored mesh, an (empty) index
    f = _frames(1, 64, 48)[0]
    try:
        small.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        raise AssertionError("a frame fitted 8 tiles")
    except B.KsError as e:
        assert e.code == B.KS_ERR_POOL_FULL, e
    st = B.KsMeshIndexStats(corners=5)
    assert L.ks_mesh_index(small._h, C.byref(st)) == B.KS_ERR_INVALID_ARG and st.corners == 0
    assert b"failed state" in L.ks_last_error(small._h)
    assert _refused(small)
    small.close()
    return {}


CASES = {"upload": case_upload, "grid": case_grid, "integrated": case_integrated, "objects": case_objects, "lifetime": case_lifetime,
         "read_only": case_read_only, "errors": case_errors}

# name -> spec: the same cases in both tiers
SPECS = {"upload_%s_vps%d" % (f, v): dict(case="upload", field=f, vps=v) for f in ("sphere", "plane", "two_label", "holes") for v in (8, 16)}
# vertices shared across the seams of 32^3 blocks ({-1,0}^3) and across the seam x = 0 of two 64^3 blocks
SPECS["upload_two_label_vps32"] = dict(case="upload", field="two_label", vps=32)
SPECS["upload_sphere_vps64"] = dict(case="upload", field="sphere", vps=64)
SPECS.update({
    "exact_zeros_on_voxel_centres": dict(case="grid", field="exact_zeros"),
    "coordinate_of_plus_zero": dict(case="grid", field="plus_zero"),
    "empty_mesh": dict(case="grid", field="empty"),
    "integrated_fast": dict(case="integrated", method=0),
    "integrated_merged": dict(case="integrated", method=1),
    "integrated_fast_frames_in_flight": dict(case="integrated", method=0, pipeline=12),
    "objects": dict(case="objects"),
    "lifetime": dict(case="lifetime"),
    "read_only": dict(case="read_only"),
    "errors": dict(case="errors"),
})


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("MESH_INDEX_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
