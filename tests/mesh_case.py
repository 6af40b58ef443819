"""The mesh cases, shared by both tiers: run_case(spec) drives whatever library the binding has loaded — the GPU tier
(tests/test_mesh_gpu.py) calls it in-process, the CPU tier (tests/test_mesh_cpu.py) runs it as a child process on the
host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.mesh_case '<json spec>'
The checker is tests/mesh_model.py (NumPy, written from the contract): every array bit for bit, in the same order."""
import json
import os
import sys

import numpy as np

VOXEL = 0.05
SPHERE_CENTRE = (0.0137, -0.0221, 0.0319)   # off the voxel grid (tests/test_mesh_cpu.py asserts the model drops no triangle here)
SPHERE_RADIUS = 0.6


# vps -> the blocks make_field covers, per axis (a fixed voxel extent, not a rounded length)
FIELD_BLOCKS = {8: (range(-2, 2),) * 3, 16: (range(-1, 1),) * 3, 32: (range(-1, 1),) * 3, 64: (range(-1, 1), range(0, 1), range(0, 1))}


def field_centre(vps):
    """Where make_field puts the sphere's centre (and the plane's foot) at this block size: the middle of its box."""
    off = np.array([0.0, 0.5 * vps * VOXEL, 0.5 * vps * VOXEL]) if vps == 64 else np.zeros(3)
    return np.array(SPHERE_CENTRE) + off


def make_field(kind, vps, seed=1):
    """Host-layout blocks (indices, tsdf, sem) of an analytic field, to upload().  What each block size covers:
      vps 8:  blocks {-2..1}^3 = [-0.8 m, 0.8 m)^3, 32^3 voxels, 64 one-tile blocks;
      vps 16: blocks {-1,0}^3  = the same 32^3 voxels, 8 blocks of 2^3 tiles;
      vps 32: blocks {-1,0}^3  = [-1.6 m, 1.6 m)^3, 64^3 voxels, 8 blocks of 4^3 tiles: the same surfaces, seams through the origin;
      vps 64: blocks {-1,0} x {0} x {0} = [-3.2 m, 3.2 m) x [0, 3.2 m)^2, two blocks of 8^3 tiles, the sphere and the plane moved by
              (0, 1.6 m, 1.6 m) to the middle of that box, so that the surface crosses the block seam x = 0.
    At 8 and 16 the bytes are those of every earlier version of this function (tests/test_mesh_cpu.py holds their hashes)."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    rx, ry, rz = FIELD_BLOCKS[vps]
    idx = np.array([(x, y, z) for x in rx for y in ry for z in rz], dtype=np.int32)
    nv = vps ** 3
    lin = np.arange(nv)
    local = np.stack([lin % vps, (lin // vps) % vps, lin // (vps * vps)], axis=1)
    centre = ((idx[:, None, :].astype(np.int64) * vps + local[None]).astype(np.float64) + 0.5) * VOXEL   # (nb, nv, 3)
    t = np.zeros((len(idx), nv), dtype=B.TSDF_DTYPE)
    s = np.zeros((len(idx), nv), dtype=B.SEM_DTYPE)
    if kind in ("sphere", "holes", "two_label"):
        dist = np.linalg.norm(centre - field_centre(vps), axis=-1) - SPHERE_RADIUS
    elif kind == "plane":
        n = np.array([0.31, -0.52, 0.79])
        dist = (centre - (field_centre(vps) - np.array(SPHERE_CENTRE))) @ (n / np.linalg.norm(n)) - 0.0613
    else:
        raise ValueError(kind)
    t["distance"] = dist.astype(np.float32)
    t["weight"] = 1.0
    label = np.full((len(idx), nv), 5, np.uint8)
    if kind == "two_label":
        label = np.where(centre[..., 0] < 0.0, 3, 7).astype(np.uint8)
    lut = synth.default_label_colors()
    t["color"] = lut[label]
    s["label"] = label
    s["color"] = lut[label]
    s["priors"] = np.float32(-0.60205999132)
    np.put_along_axis(s["priors"], label[..., None].astype(np.int64), np.float32(-0.1), axis=-1)
    keep = np.ones(len(idx), bool)
    if kind == "holes":
        rng = np.random.default_rng(seed)
        t["weight"][rng.random(t["weight"].shape) < 0.10] = 0.0
        keep = rng.random(len(idx)) >= 0.15   # some blocks absent
        if keep.all():                        # (the draw for the 8 blocks of vps 32 keeps them all: one block with three lower neighbours goes)
            keep[len(idx) - 1] = False
    return idx[keep], t[keep], s[keep]


SAME_MAP_BOX = ((-64, 64), (0, 64), (0, 64))     # global voxels [lo, hi) per axis: 16 x 8 x 8 tiles
SAME_MAP_TILES = 1024
SAME_MAP_CENTRE = (0.0137, 1.5779, 1.6319)       # off the voxel grid, on the seam x = 0 of every block size
SAME_MAP_RADIUS = 1.0
SAME_MAP_POCKET = ((26, 58), (6, 58), (6, 58))   # global voxels [lo, hi): outside the sphere, every voxel observed and free
_SAME_MAP = {}


def same_map_voxels():
    """The one voxel content of same_map(), in global voxel coordinates: (origin, tsdf[z, y, x], sem[z, y, x]) over SAME_MAP_BOX.
    A sphere surface (truncated at 4 voxels) with the labels 3 / 7 split at the plane y + z = 3.2 m, 10 % of the voxels with
    weight 0, except in SAME_MAP_POCKET (free, fully observed: room for the planner kernels)."""
    if "voxels" not in _SAME_MAP:
        from kimera_semantics_amd import binding as B
        from kimera_semantics_amd import synth
        (x0, x1), (y0, y1), (z0, z1) = SAME_MAP_BOX
        gz, gy, gx = np.meshgrid(np.arange(z0, z1), np.arange(y0, y1), np.arange(x0, x1), indexing="ij")
        centre = (np.stack([gx, gy, gz], axis=-1).astype(np.float64) + 0.5) * VOXEL
        t, s = np.zeros(gx.shape, B.TSDF_DTYPE), np.zeros(gx.shape, B.SEM_DTYPE)
        dist = np.linalg.norm(centre - np.array(SAME_MAP_CENTRE), axis=-1) - SAME_MAP_RADIUS
        t["distance"] = np.clip(dist, -4 * VOXEL, 4 * VOXEL).astype(np.float32)
        weight = np.where(np.random.default_rng(21).random(gx.shape) < 0.10, 0.0, 1.0).astype(np.float32)
        (px0, px1), (py0, py1), (pz0, pz1) = SAME_MAP_POCKET
        pocket = (gx >= px0) & (gx < px1) & (gy >= py0) & (gy < py1) & (gz >= pz0) & (gz < pz1)
        assert (dist[pocket] > 0.1).all()
        weight[pocket] = 1.0
        t["weight"] = weight
        label = np.where(centre[..., 1] + centre[..., 2] < 3.2, 3, 7).astype(np.uint8)
        lut = synth.default_label_colors()
        t["color"] = lut[label]
        s["label"], s["color"] = label, lut[label]
        s["priors"] = np.float32(-0.60205999132)
        np.put_along_axis(s["priors"], label[..., None].astype(np.int64), np.float32(-0.1), axis=-1)
        _SAME_MAP["voxels"] = (np.array([x0, y0, z0]), t, s)
    return _SAME_MAP["voxels"]


def to_blocks(origin, field, vps):
    """field[z, y, x] over a box of whole blocks starting at the global voxel `origin` -> (block indices ascending by (x, y, z),
    rows of vps^3 voxels in x + vps * (y + vps * z) order)."""
    nz, ny, nx = field.shape
    assert nx % vps == 0 and ny % vps == 0 and nz % vps == 0 and (np.asarray(origin) % vps == 0).all()
    bz, by, bx = nz // vps, ny // vps, nx // vps
    rows = field.reshape(bz, vps, by, vps, bx, vps).transpose(4, 2, 0, 1, 3, 5).reshape(bx * by * bz, vps ** 3)
    o = np.asarray(origin) // vps
    idx = np.array([(o[0] + x, o[1] + y, o[2] + z) for x in range(bx) for y in range(by) for z in range(bz)], dtype=np.int32)
    return idx, np.ascontiguousarray(rows)


def from_blocks(idx, rows, vps, box=SAME_MAP_BOX):
    """The inverse of to_blocks for blocks in any order: rows -> field[z, y, x] over `box` (every block of the box must be there)."""
    (x0, x1), (y0, y1), (z0, z1) = box
    out = np.zeros((z1 - z0, y1 - y0, x1 - x0), rows.dtype)
    seen = np.zeros(out.shape, bool)
    for b, row in zip(np.asarray(idx).reshape(-1, 3), rows):
        x, y, z = (int(b[0]) * vps - x0, int(b[1]) * vps - y0, int(b[2]) * vps - z0)
        out[z:z + vps, y:y + vps, x:x + vps] = row.reshape(vps, vps, vps)
        seen[z:z + vps, y:y + vps, x:x + vps] = True
    assert seen.all() and len(idx) * vps ** 3 == out.size, (len(idx), vps)
    return out


def same_map(vps):
    """Host-layout blocks (indices, tsdf, sem) of ONE voxel content over the voxel box [-64, 64) x [0, 64) x [0, 64), cut into
    blocks of vps^3: 1024 blocks at 8, 128 at 16, 16 at 32, 2 at 64 — the same 1024 resident tiles, block layout the only difference."""
    origin, t, s = same_map_voxels()
    idx, tb = to_blocks(origin, t, vps)
    return idx, tb, to_blocks(origin, s, vps)[1]


def planted_voxels(vps, blocks=((-1, 0, 0), (0, 0, 0))):
    """Global voxels at the local indices 0, vps - 1, vps (vps - 1) and vps^3 - 1 of each block: the four corners of the linear
    index range whose decoding l -> (l % vps, l / vps % vps, l / vps^2) a block export has to get right."""
    out = []
    for b in blocks:
        for l in (0, vps - 1, vps * (vps - 1), vps ** 3 - 1):
            out.append(tuple(int(b[a]) * vps + (l // vps ** a) % vps for a in range(3)))
    return out


def _label_colors():
    from kimera_semantics_amd import synth
    return synth.default_label_colors()


def _integrator(method, w, h, vps=16, pipeline=0, max_tiles=4096, **extra):
    from kimera_semantics_amd import binding as B
    from tests.util import COMMON
    return B.HipIntegrator(B.default_config(method=method, voxel_size=VOXEL, voxels_per_side=vps, truncation_distance=4 * VOXEL,
                                            max_tiles=max_tiles, max_points=w * h, pipeline_frames=pipeline, **dict(COMMON, **extra)))


def _frames(n, w, h, step=5, hfov=90.0):
    from kimera_semantics_amd import synth
    sc = synth.make_scene("room")
    return [synth.render_frame(sc, synth.trajectory_pose(step * k), w, h, hfov_deg=hfov, seed=40 + k) for k in range(n)]


def case_upload(spec):
    from tests import mesh_model as M
    vps = spec["vps"]
    g = _integrator(0, 64, 48, vps=vps)
    idx, t, s = make_field(spec["field"], vps)
    g.upload(idx, t, s)
    mesh = g.mesh()
    model = M.model_of(g)
    M.assert_same(mesh, model, spec["field"])
    assert mesh.n_triangles >= spec.get("triangles_at_least", 500), mesh.n_triangles
    assert mesh.stats["triangles_total"] == mesh.n_triangles and mesh.stats["degenerate_dropped"] == model["degenerate"], mesh.stats
    assert mesh.stats["blocks_meshed"] == mesh.stats["blocks_total"] == len(g.block_indices())
    if spec["field"] == "two_label":
        assert set(np.unique(mesh.labels)) == {3, 7}
    again = g.mesh()   # two runs give the same bytes
    M.assert_same(again, model, "second extraction")
    g.close()
    return dict(triangles=mesh.n_triangles)


def case_integrated(spec):
    from tests import mesh_model as M
    w, h = spec.get("size", [64, 48])
    g = _integrator(spec["method"], w, h, **spec.get("cfg", {}))
    for f in _frames(2, w, h):
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    mesh = g.mesh()
    M.assert_same(mesh, M.model_of(g), "integrated")
    assert mesh.n_triangles >= 300, mesh.n_triangles
    assert len(np.unique(mesh.labels)) >= 2
    g.close()
    return dict(triangles=mesh.n_triangles)


def _rows(a):
    return {tuple(int(v) for v in r) for r in np.asarray(a).reshape(-1, 3)}


def _by_block(m):
    """block -> bytes of its segment, of a Mesh or of the model's dict."""
    get = (lambda k: m[k]) if isinstance(m, dict) else (lambda k: getattr(m, k))
    out = {}
    for b in get("blocks"):
        a, n = int(b["first_vertex"]), int(b["n_vertices"])
        out[tuple(int(v) for v in b["block"])] = b"".join(np.ascontiguousarray(get(k)[a:a + n]).tobytes() for k in ("xyz", "normals", "rgba", "labels"))
    return out


def case_incremental(spec):
    """3c + 3d: only_stale refreshes == from scratch; the sync flags of the host are not the mesher's."""
    from tests import mesh_model as M
    w, h = spec.get("size", [64, 48])
    method = spec.get("method", 0)
    # the second pose looks at another part of the room: it touches only part of the map
    f1, f2 = _frames(2, w, h, step=spec.get("step", 40), hfov=spec.get("hfov", 50.0))
    g, fresh, never = (_integrator(method, w, h) for _ in range(3))
    g.integrate(f1.T_G_C, f1.xyz, f1.rgba, f1.labels)
    m1 = g.mesh(only_stale=False)
    model1 = M.model_of(g)
    M.assert_same(m1, model1, "after frame 1")
    stale_before = _rows(g.block_indices())
    g.integrate(f2.T_G_C, f2.xyz, f2.rgba, f2.labels)
    touched = _rows(g.updated_block_indices(reset=False))   # blocks written since the context was created (never reset here)
    m2 = g.mesh(only_stale=True)
    for c in (fresh, never):
        for f in (f1, f2):
            c.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    full = fresh.mesh(only_stale=False)
    model2 = M.model_of(fresh)
    M.assert_same(full, model2, "fresh context, both frames")
    M.assert_same(m2, model2, "only_stale refresh")
    assert m2.stats["blocks_meshed"] < m2.stats["blocks_total"], m2.stats
    assert m2.stats["blocks_total"] == len(g.block_indices())
    # changed blocks: every block whose model mesh differs, and nothing outside (stale blocks + their lower neighbours)
    changed = _rows(g.mesh_changed_blocks())
    a, b = _by_block(model1), _by_block(model2)
    differ = {k for k in set(a) | set(b) if a.get(k) != b.get(k)}
    assert differ and differ <= changed, sorted(differ - changed)[:5]
    # (the flags say which TILES frame 2 wrote; at block granularity that is within the blocks `updated` lists, which
    # have been accumulating since frame 1 — so bound it by what frame 2 can have touched: every block of the map that is
    # new, or listed by a context that saw frame 2 alone as its second frame)
    lower = lambda s: {(x - (o & 1), y - ((o >> 1) & 1), z - (o >> 2)) for (x, y, z) in s for o in range(8)}
    second = _integrator(method, w, h)
    second.integrate(f1.T_G_C, f1.xyz, f1.rgba, f1.labels)
    second.updated_block_indices(reset=True)
    second.integrate(f2.T_G_C, f2.xyz, f2.rgba, f2.labels)
    wrote = _rows(second.updated_block_indices(reset=False))
    second.close()
    assert changed == lower(wrote) & _rows(g.block_indices()), (len(changed), len(wrote))
    assert len(stale_before) > 0
    # nothing integrated: nothing to do
    m3 = g.mesh(only_stale=True)
    assert m3.stats["blocks_meshed"] == 0 and len(g.mesh_changed_blocks()) == 0, m3.stats
    M.assert_same(m3, model2, "idle refresh")
    # 3d: the host's flags are untouched by the mesher
    assert _rows(g.updated_block_indices(reset=False)) == _rows(never.updated_block_indices(reset=False)) == touched
    # an upload of one block re-meshes that block and its lower neighbours
    idx, t, s = g.download()
    k = int(np.argmax((t["weight"] > 0).sum(axis=1)))
    tb = t[k:k + 1].copy()
    tb["distance"] = -tb["distance"]
    g.upload(idx[k:k + 1], tb, s[k:k + 1])
    m4 = g.mesh(only_stale=True)
    blk = tuple(int(v) for v in idx[k])
    assert _rows(g.mesh_changed_blocks()) == lower({blk}) & _rows(idx), blk
    M.assert_same(m4, M.model_of(g), "after the upload of one block")
    # clearing the map empties the mesh
    g.clear()
    m5 = g.mesh(only_stale=True)
    assert m5.n_triangles == 0 and len(m5.blocks) == 0
    for c in (g, fresh, never):
        c.close()
    return dict(triangles=m2.n_triangles, meshed=m2.stats["blocks_meshed"], total=m2.stats["blocks_total"])


def case_errors(spec):
    import ctypes as C
    from kimera_semantics_amd import binding as B
    g = _integrator(0, 64, 48, vps=8)
    idx, t, s = make_field("plane", 8)
    g.upload(idx, t, s)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        try:
            g.mesh(min_weight=bad)
            raise AssertionError("min_weight %r accepted" % bad)
        except B.KsError as e:
            assert e.code == B.KS_ERR_INVALID_ARG, e
    m = g.mesh()
    assert m.n_triangles > 0
    L = B.lib()
    xyz = np.zeros((len(m.xyz) - 1, 3), np.float32)
    assert L.ks_mesh_download(g._h, None, 0, xyz.ctypes.data, None, None, None, len(xyz)) == B.KS_ERR_INVALID_ARG
    blocks = np.zeros(len(m.blocks) - 1, dtype=B.MESH_BLOCK_DTYPE)
    assert L.ks_mesh_download(g._h, blocks.ctypes.data, len(blocks), None, None, None, None, 0) == B.KS_ERR_INVALID_ARG
    n = C.c_size_t()
    out = np.zeros((1, 3), np.int32)
    assert L.ks_mesh_changed_blocks(g._h, out.ctypes.data, 1, C.byref(n)) == B.KS_ERR_INVALID_ARG and n.value == len(idx)
    # any of the four arrays may be NULL
    lab = np.zeros(len(m.xyz), np.uint8)
    assert L.ks_mesh_download(g._h, None, 0, None, None, None, lab.ctypes.data, len(lab)) == 0 and (lab == m.labels).all()
    g.close()
    # a marcher context of the exact multi-GPU mode holds no voxel data
    marcher, owner = (_integrator(1, 64, 48) for _ in range(2))
    f = _frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    try:
        marcher.mesh()
        raise AssertionError("a marcher context was meshed")
    except B.KsError as e:
        assert e.code == B.KS_ERR_UNSUPPORTED, e
    assert owner.mesh().n_triangles > 0   # (the owner holds the map)
    marcher.close()
    owner.close()
    return {}


CASES = {"upload": case_upload, "integrated": case_integrated, "incremental": case_incremental, "errors": case_errors}

# name -> spec: the same cases in both tiers
SPECS = {
    "upload_sphere_vps8": dict(case="upload", field="sphere", vps=8),
    "upload_sphere_vps16": dict(case="upload", field="sphere", vps=16),
    "upload_plane_vps8": dict(case="upload", field="plane", vps=8),
    "upload_plane_vps16": dict(case="upload", field="plane", vps=16),
    "upload_two_label_vps8": dict(case="upload", field="two_label", vps=8),
    "upload_two_label_vps16": dict(case="upload", field="two_label", vps=16),
    "upload_holes_vps8": dict(case="upload", field="holes", vps=8),
    "upload_holes_vps16": dict(case="upload", field="holes", vps=16),
    # 4^3 and 8^3 tiles per block: 32 and 256 passes of the count scan, cube addresses of 15 and 18 bits per block
    "upload_sphere_vps32": dict(case="upload", field="sphere", vps=32),
    "upload_holes_vps32": dict(case="upload", field="holes", vps=32),
    "upload_two_label_vps32": dict(case="upload", field="two_label", vps=32),
    "upload_sphere_vps64": dict(case="upload", field="sphere", vps=64),
    "integrated_fast_vps32": dict(case="integrated", method=0, cfg=dict(vps=32)),
    "integrated_fast": dict(case="integrated", method=0),
    "integrated_merged": dict(case="integrated", method=1),
    "incremental_equals_from_scratch": dict(case="incremental"),
    "errors": dict(case="errors"),
}


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("MESH_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
