"""The ESDF cases, shared by both tiers: run_case(spec) drives whatever library the binding has loaded — the GPU tier
(tests/test_esdf_gpu.py) calls it in-process, the CPU tier (tests/test_esdf_cpu.py) runs it as a child process on the
host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.esdf_case '<json spec>'
The checker is tests/esdf_model.py (NumPy, written from the contract): the bytes of every record of every block."""
import json
import os
import sys

import numpy as np

from tests import mesh_case

VOXEL = mesh_case.VOXEL          # 5 cm
MIN_DISTANCE = 0.1
RANDOM_SEED = 7                  # chosen on the CPU: case_random asserts what it is chosen for
_MODELS = {}                     # (field, vps, max_distance) -> (blocks, Model): a reference is computed once per process


def cfg_of(spec):
    return dict(min_distance_m=MIN_DISTANCE, max_distance_m=spec.get("max_distance_m", 0.4))


def random_field(idx, vps, seed, near=0.03, unobserved=0.10):
    """Not geometric: distances per voxel from {+-0.03, +-0.07 (sites, about 3 %), +-0.3}, labels 0..20, 10 % weight 0.
    near, unobserved: the two fractions (the draws are the same whatever they are)."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    rng = np.random.default_rng(seed)
    idx = np.asarray(idx, np.int32).reshape(-1, 3)
    shape = (len(idx), vps ** 3)
    t, s = np.zeros(shape, B.TSDF_DTYPE), np.zeros(shape, B.SEM_DTYPE)
    near = rng.random(shape) < near
    mag = np.where(near, rng.choice(np.array([0.03, 0.07], np.float32), shape), np.float32(0.3))
    t["distance"] = np.where(rng.random(shape) < 0.5, -mag, mag).astype(np.float32)
    t["weight"] = np.where(rng.random(shape) < unobserved, 0.0, 1.0).astype(np.float32)
    label = rng.integers(0, 21, shape).astype(np.uint8)
    lut = synth.default_label_colors()
    t["color"] = lut[label]
    s["label"], s["color"] = label, lut[label]
    s["priors"] = np.float32(-0.60205999132)
    np.put_along_axis(s["priors"], label[..., None].astype(np.int64), np.float32(-0.1), axis=-1)
    return idx, t, s


def make_field(kind, vps):
    if kind in ("sphere", "holes"):
        return mesh_case.make_field(kind, vps)
    if kind == "no_sites":   # the sphere with its band pushed out: every |d| >= 0.1
        idx, t, s = mesh_case.make_field("sphere", vps)
        d = t["distance"]
        t["distance"] = np.where(d < 0, -1, 1).astype(np.float32) * np.maximum(np.abs(d), np.float32(MIN_DISTANCE))
        return idx, t, s
    if kind == "random":
        idx, _, _ = mesh_case.make_field("sphere", vps)
        return random_field(idx, vps, RANDOM_SEED)
    if kind == "slab":       # a non-cubic box far from the origin, negative indices
        idx = np.array([(x, y, 0) for x in (3, 4, 5) for y in (-7, -6)], np.int32)
        return random_field(idx, vps, 11)
    raise ValueError(kind)


def _uploaded(kind, vps, **extra):
    g = mesh_case._integrator(0, 64, 48, vps=vps, **extra)
    idx, t, s = make_field(kind, vps)
    g.upload(idx, t, s)
    return g


def _model(g, spec, form):
    """The model of an uploaded analytic field, shared between the cases of one process."""
    from tests import esdf_model as M
    key = (spec["field"], spec["vps"], spec.get("max_distance_m", 0.4), form)
    if key not in _MODELS:
        _MODELS[key] = M.model_of(g, cfg_of(spec), form=form, keep_keys=(spec["field"] == "random"))
    return _MODELS[key]


def _check_stats(stats, model, what):
    for k in ("voxels_observed", "voxels_fixed", "voxels_clamped"):
        assert stats[k] == model.stats[k], (what, k, stats[k], model.stats[k])


def case_upload(spec):
    from tests import esdf_model as M
    g = _uploaded(spec["field"], spec["vps"])
    idx, rec, stats = g.esdf(**cfg_of(spec))
    model = _model(g, spec, spec.get("form", "brute"))
    M.assert_same(rec, model.blocks(idx), spec["field"])
    _check_stats(stats, model, spec["field"])
    nz, ny, nx = model.dense.shape
    assert stats["box_voxels"] == [nx, ny, nz], (stats, model.dense.shape)
    assert stats["voxels_observed"] > 1000
    if spec["field"] == "sphere":
        assert stats["voxels_clamped"] > 0 and rec["distance"].min() == -np.float32(cfg_of(spec)["max_distance_m"])
    if spec["field"] == "no_sites":
        obs = rec["flags"] == 1
        assert stats["voxels_fixed"] == 0 and (rec["flags"] <= 1).all() and obs.sum() == stats["voxels_observed"]
        assert (np.abs(rec["distance"][obs]) == np.float32(cfg_of(spec)["max_distance_m"])).all() and (rec["label"][obs] == 255).all()
    if spec["field"] == "random":
        tied = M.tied_voxels(model, M.reach(cfg_of(spec)["max_distance_m"], VOXEL))
        assert tied >= 1000, tied
    again = g.esdf(**cfg_of(spec))[1]   # two runs give the same bytes
    M.assert_same(again, rec, "second update")
    g.close()
    return dict(stats)


def case_integrated(spec):
    from tests import esdf_model as M
    w, h = spec.get("size", [64, 48])
    g = mesh_case._integrator(spec["method"], w, h)
    for f in mesh_case._frames(2, w, h):
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    idx, rec, stats = g.esdf(**cfg_of(spec))
    model = M.model_of(g, cfg_of(spec))
    M.assert_same(rec, model.blocks(idx), "integrated")
    _check_stats(stats, model, "integrated")
    near = np.unique(rec["label"][(rec["flags"] == 1) & (rec["label"] != 255)])
    assert len(near) >= 3, near
    g.close()
    return dict(stats, labels=len(near))


def sphere_blocks(vps, blocks_per_side):
    """The sphere of mesh_case.make_field over a cube of blocks_per_side^3 blocks around the origin."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    rng_b = range(-(blocks_per_side // 2), blocks_per_side // 2)
    idx = np.array([(x, y, z) for x in rng_b for y in rng_b for z in rng_b], dtype=np.int32)
    lin = np.arange(vps ** 3)
    local = np.stack([lin % vps, (lin // vps) % vps, lin // (vps * vps)], axis=1)
    centre = ((idx[:, None, :].astype(np.int64) * vps + local[None]).astype(np.float64) + 0.5) * VOXEL
    t, s = np.zeros((len(idx), vps ** 3), B.TSDF_DTYPE), np.zeros((len(idx), vps ** 3), B.SEM_DTYPE)
    t["distance"] = (np.linalg.norm(centre - np.array(mesh_case.SPHERE_CENTRE), axis=-1) - mesh_case.SPHERE_RADIUS).astype(np.float32)
    t["weight"] = 1.0
    label = np.where(centre[..., 2] < 0.0, 3, 7).astype(np.uint8)
    lut = synth.default_label_colors()
    t["color"] = lut[label]
    s["label"], s["color"] = label, lut[label]
    s["priors"] = np.float32(-0.60205999132)
    np.put_along_axis(s["priors"], label[..., None].astype(np.int64), np.float32(-0.1), axis=-1)
    return idx, t, s


def case_region(spec):
    """The sphere over 8^3 blocks of 8^3 voxels (64^3 voxels: large enough for the region's dilated box to be smaller than
    the map's), the region its central 2 x 2 x 2 blocks."""
    from tests import esdf_model as M
    g = mesh_case._integrator(0, 64, 48, vps=8)
    g.upload(*sphere_blocks(8, 8))
    idx, rec_full, stats_full = g.esdf(**cfg_of(spec))
    model = M.model_of(g, cfg_of(spec))
    M.assert_same(rec_full, model.blocks(idx), "full map")
    region = ([-1, -1, -1], [0, 0, 0])
    stats = g.esdf_update(region=region, **cfg_of(spec))
    rec = g.esdf_blocks(idx)
    M.assert_same(rec, model.blocks(idx, region=region), "region")
    inside = np.array([all(region[0][a] <= b[a] <= region[1][a] for a in range(3)) for b in idx])
    assert inside.sum() == 8
    # inside: the full-map result (the sites outside the region count); outside: default records
    assert rec[inside].tobytes() == rec_full[inside].tobytes()
    assert rec[~inside].tobytes() == M.default_records(rec[~inside].shape).tobytes()
    assert (rec[inside]["flags"] == 1).any() and (rec_full[~inside]["flags"] == 3).any()
    assert stats["voxels_observed"] == 8 * 512, stats
    assert 0 < stats["workspace_bytes"] < stats_full["workspace_bytes"], (stats, stats_full)
    g.close()
    return dict(stats)


def case_snapshot(spec):
    from kimera_semantics_amd import binding as B
    from tests import esdf_model as M
    w, h = 64, 48
    g = mesh_case._integrator(spec.get("method", 0), w, h)
    f1, f2 = mesh_case._frames(2, w, h, step=40, hfov=50.0)   # the second pose looks elsewhere: new tiles join the map
    g.integrate(f1.T_G_C, f1.xyz, f1.rgba, f1.labels)
    idx1, rec1, _ = g.esdf(**cfg_of(spec))
    model1 = M.model_of(g, cfg_of(spec))
    M.assert_same(rec1, model1.blocks(idx1), "after frame 1")
    g.integrate(f2.T_G_C, f2.xyz, f2.rgba, f2.labels)
    idx2 = g.block_indices()
    assert len(idx2) > len(idx1)
    # the stored ESDF is a snapshot: unchanged for the old blocks' voxels, default records where tiles joined later
    M.assert_same(g.esdf_blocks(idx2), model1.blocks(idx2), "snapshot after another frame")
    idx3, rec3, _ = g.esdf(**cfg_of(spec))
    M.assert_same(rec3, M.model_of(g, cfg_of(spec)).blocks(idx3), "second update")
    assert rec3.tobytes() != model1.blocks(idx3).tobytes()
    g.clear()
    try:
        g.esdf_blocks(idx1)
        raise AssertionError("download after clear() succeeded")
    except B.KsError as e:
        assert e.code == B.KS_ERR_INVALID_ARG, e
    g.close()
    return {}


def case_query(spec):
    from tests import esdf_model as M
    g = _uploaded("holes", 16)
    idx, rec, _ = g.esdf(**cfg_of(spec))
    model = _model(g, dict(spec, field="holes", vps=16), "separable")
    M.assert_same(rec, model.blocks(idx), "holes")
    rng = np.random.default_rng(3)
    ijk = rng.integers(-20, 20, (4096, 3))          # the map spans [-16, 16): some points lie outside it
    jitter = rng.uniform(-0.4, 0.4, (4096, 3))
    xyz = ((ijk + 0.5 + jitter) * VOXEL).astype(np.float32)
    got = g.esdf_query(xyz)
    want = model.at(ijk)
    M.assert_same(got, want, "query")
    outside = (ijk < -16).any(axis=1) | (ijk >= 16).any(axis=1)
    assert outside.sum() > 100 and (want["flags"][~outside] == 0).sum() > 100 and (want["flags"] == 1).sum() > 100
    g.close()
    return {}


def case_errors(spec):
    from kimera_semantics_amd import binding as B
    from tests import esdf_model as M
    g = _uploaded("sphere", 8)
    idx = g.block_indices()

    def refused(code, call):
        try:
            call()
        except B.KsError as e:
            assert e.code == code, e
            return e
        raise AssertionError("accepted")

    refused(B.KS_ERR_INVALID_ARG, lambda: g.esdf_blocks(idx))            # before any update
    refused(B.KS_ERR_INVALID_ARG, lambda: g.esdf_query(np.zeros((1, 3))))
    for name in ("min_weight", "min_distance_m", "max_distance_m"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused(B.KS_ERR_INVALID_ARG, lambda: g.esdf_update(**dict(cfg_of(spec), **{name: bad})))
    refused(B.KS_ERR_INVALID_ARG, lambda: g.esdf_update(min_distance_m=MIN_DISTANCE, max_distance_m=255.5 * VOXEL))   # R = 256
    refused(B.KS_ERR_INVALID_ARG, lambda: g.esdf_blocks(idx))            # ... and none of these stored anything
    e = refused(B.KS_ERR_UNSUPPORTED, lambda: g.esdf_update(max_workspace_bytes=4096, **cfg_of(spec)))
    assert e.stats["workspace_bytes"] > 4096 and "use_region" in str(e) and str(e.stats["workspace_bytes"]) in str(e), e
    st = g.esdf_update(min_distance_m=MIN_DISTANCE, max_distance_m=255 * VOXEL)   # R = 255 is served
    assert st["voxels_observed"] > 0 and st["voxels_clamped"] == 0
    far = dict(min_distance_m=MIN_DISTANCE, max_distance_m=255 * VOXEL)   # ... and equals the model at that window
    assert M.reach(far["max_distance_m"], VOXEL) == 255
    model = M.model_of(g, far)
    M.assert_same(g.esdf_blocks(idx), model.blocks(idx), "R = 255")
    _check_stats(st, model, "R = 255")
    g.close()
    # a marcher context of the exact multi-GPU mode holds no voxel data
    marcher, owner = (mesh_case._integrator(1, 64, 48) for _ in range(2))
    f = mesh_case._frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    refused(B.KS_ERR_UNSUPPORTED, lambda: marcher.esdf_update(**cfg_of(spec)))
    assert owner.esdf_update(**cfg_of(spec))["voxels_fixed"] > 0   # (the owner holds the map)
    marcher.close()
    owner.close()
    return {}


CASES = {"upload": case_upload, "integrated": case_integrated, "region": case_region, "snapshot": case_snapshot, "query": case_query,
         "errors": case_errors}

# name -> spec: the same cases in both tiers.  max_distance_m 0.4: R = 8, exactly one tile; 0.55: R = 11, a window that ends
# mid-tile.
SPECS = {}
for _field in ("sphere", "holes", "no_sites"):
    for _vps in (8, 16):
        for _r, _d in ((8, 0.4), (11, 0.55)):
            SPECS["upload_%s_vps%d_r%d" % (_field, _vps, _r)] = dict(case="upload", field=_field, vps=_vps, max_distance_m=_d)
# 4^3 tiles per block at the existing windows; 8^3 tiles per block with the surface across the seam of its two blocks
for _field in ("sphere", "holes"):
    for _r, _d in ((8, 0.4), (11, 0.55)):
        SPECS["upload_%s_vps32_r%d" % (_field, _r)] = dict(case="upload", field=_field, vps=32, max_distance_m=_d)
SPECS.update({
    "random_ties_vps32": dict(case="upload", field="random", vps=32, max_distance_m=0.4),
    "upload_sphere_vps64": dict(case="upload", field="sphere", vps=64, max_distance_m=0.4, form="separable"),
    "random_ties": dict(case="upload", field="random", vps=8, max_distance_m=0.4),
    "slab": dict(case="upload", field="slab", vps=16, max_distance_m=0.55),
    "integrated_fast": dict(case="integrated", method=0, max_distance_m=0.4),
    "integrated_merged": dict(case="integrated", method=1, max_distance_m=0.4),
    "region": dict(case="region", max_distance_m=0.55),
    "snapshot": dict(case="snapshot", max_distance_m=0.4),
    "query": dict(case="query", max_distance_m=0.4),
    "errors": dict(case="errors", max_distance_m=0.4),
})


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("ESDF_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
