"""The cases of the ESDF reads (ks_esdf_sample, ks_esdf_slice, ks_esdf_sweep; DESIGN.md, section "ESDF reads"), shared by both
tiers like those of tests/esdf_case.py: the GPU tier (tests/test_esdf_read_gpu.py) calls run_case in-process, the CPU tier
(tests/test_esdf_read_cpu.py) runs it as a child process on the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.esdf_read_case '<json spec>'
The checker is tests/esdf_read_model.py on the stored ESDF as the library hands it out (block_indices, esdf_blocks); every
comparison is byte for byte, statistics included.  Maps arrive through upload + esdf_update; the fields are those of
tests/esdf_case.py over [-0.8 m, 0.8 m)^3 (64 tiles), max_distance_m = 0.4."""
import ctypes
import json
import os
import sys

import numpy as np

from tests import esdf_case
from tests import esdf_read_model as M

VOXEL = esdf_case.VOXEL
HALF = 0.8                       # the fields' box is [-HALF, HALF)^3
TILE = 8 * VOXEL
MIXED_SEED = 5                   # chosen on the CPU: case_mixed asserts what it is chosen for
SWEEP_SEED = 9
ENDS_ON_A_SAMPLE = slice(272, 280)                     # rows of sweep_segments()
ENDS_RADIUS = float(np.float32(0.4) - np.float32(0.0625))   # max_distance_m - radius = 2^-4 exactly in f32
cfg_of = esdf_case.cfg_of
F = np.float32


def refused(code, call):
    from kimera_semantics_amd import binding as B
    try:
        call()
    except B.KsError as e:
        assert e.code == code, e
        return e
    raise AssertionError("accepted")


def _stored(spec, **extra):
    g = esdf_case._uploaded(spec.get("field", "sphere"), spec.get("vps", 8), **extra)
    g.esdf_update(**cfg_of(spec))
    return g


def mixed_points(seed, n=4001):
    """60 % uniform over the box and one tile beyond it, 40 % within a voxel of one of the box's faces (where a point's own voxel is
    stored and some corner is not)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-HALF - TILE, HALF + TILE, (n, 3))
    shell = np.nonzero(rng.random(n) < 0.4)[0]
    p[shell] = rng.uniform(-HALF, HALF, (len(shell), 3))
    axis, side = rng.integers(0, 3, len(shell)), rng.choice([-HALF, HALF], len(shell))
    p[shell, axis] = side + rng.uniform(-VOXEL, VOXEL, len(shell))
    return p.astype(F)


def check_sample(g, store, xyz, what):
    got = g.esdf_sample(xyz)
    want = M.sample(store, xyz, VOXEL)
    M.assert_same(got, want, what)
    return got, want


def case_mixed(spec):
    g = _stored(spec)
    store = M.store_of(g)
    xyz = mixed_points(MIXED_SEED)
    assert len(xyz) % 64 != 0
    got, want = check_sample(g, store, xyz, "mixed")
    share = {k: v / len(xyz) for k, v in want["stats"].items()}
    assert min(share.values()) >= 0.05, share
    assert sum(got["stats"].values()) == len(xyz)
    M.assert_same(g.esdf_sample(xyz), got, "second call")                       # two calls give the same bytes
    assert np.isnan(got["distance"][got["status"] == 0]).all() and (got["label"][got["status"] == 0] == 255).all()
    assert (got["gradient"][got["status"] == 2] != 0).any() and (got["gradient"][got["status"] != 2] == 0).all()
    # the nearest-voxel answers are those of ks_esdf_query
    q = g.esdf_query(xyz)
    near = got["status"] == 1
    assert near.any() and got["distance"][near].tobytes() == q["distance"][near].tobytes()
    known = got["status"] != 0
    assert (got["label"][known] == q["label"][known]).all() and (got["flags"][known] == q["flags"][known]).all()
    g.close()
    return dict(share)


def edge_points():
    c = lambda *ijk: [(v + 0.5) * VOXEL for v in ijk]               # a voxel centre: f = 0 on every axis
    pts = [c(0, 0, 0), c(-1, -1, -1), c(3, -4, 5), c(7, 7, 7), c(8, 8, 8), c(-16, -16, -16), c(15, 15, 15), c(-17, 0, 0), c(16, 0, 0),
           [0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, -0.0, 0.1], [VOXEL, 2 * VOXEL, -3 * VOXEL],   # cell faces: f = 0.5, n at its edge
           [TILE, 0.01, 0.01], [-TILE, -TILE, -TILE], [TILE - 0.5 * VOXEL, TILE + 0.5 * VOXEL, 0.0],    # tile seams
           [-0.31, -0.42, -0.53], [-HALF, -HALF, -HALF], [HALF, HALF, HALF], [-HALF + 0.5 * VOXEL, 0.0, 0.0],
           [6e4, 0.0, 0.0], [0.0, -6e4, 0.0], [6e4, 6e4, 6e4], [52428.75, 0.0, 0.0], [3e38, 0.0, 0.0],   # outside the packed range
           [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [np.nan, np.nan, np.nan]]
    rng = np.random.default_rng(2)
    grid = rng.integers(-18, 18, (60, 3)) * VOXEL * rng.choice([0.5, 1.0], (60, 1))   # more centres, faces and seams
    centres = (rng.integers(-16, 16, (60, 3)) + 0.5) * VOXEL
    return np.concatenate([np.array(pts, np.float64), grid, centres]).astype(F)


def case_edges(spec):
    g = _stored(spec)
    store = M.store_of(g)
    xyz = edge_points()
    got, want = check_sample(g, store, xyz, "edges")
    assert (got["status"][20:29] == 0).all() and set(np.unique(got["status"])) == {0, 1, 2}, got["status"]
    # f = 0 on every axis (in f32, as the contract computes it): the interpolant is the record of the voxel itself
    with np.errstate(invalid="ignore", over="ignore"):
        gf = xyz * M.inv_of(VOXEL) - F(0.5)
        on_centre = (gf == np.floor(gf)).all(axis=1) & (got["status"] == 2)
    assert on_centre.sum() >= 3, on_centre.sum()
    assert got["distance"][on_centre].tobytes() == g.esdf_query(xyz[on_centre])["distance"].tobytes()
    for k in range(len(xyz)):                                                   # n = 1, every point on its own
        one = g.esdf_sample(xyz[k])
        for name in ("distance", "gradient", "status", "label", "flags"):
            assert one[name].tobytes() == got[name][k:k + 1].tobytes(), (k, name, one[name], got[name][k])
    none = g.esdf_sample(np.zeros((0, 3), F))                                   # n = 0
    assert none["stats"] == dict(points_interpolated=0, points_nearest=0, points_unknown=0) and none["distance"].shape == (0,)
    assert g.esdf_sweep(np.zeros((0, 6), F))["stats"]["samples"] == 0
    g.close()
    return dict(want["stats"])


def case_snapshot(spec):
    vps = spec["vps"]
    g = _stored(spec)
    idx0 = g.block_indices()
    new = np.array([[int(idx0[:, 0].max()) + 1, 0, 0]], np.int32)               # beside the box, on its +x face
    lo = (new[0] * vps + 0.5) * VOXEL
    rng = np.random.default_rng(4)
    inside = (lo + rng.uniform(VOXEL, (vps - 2) * VOXEL, (300, 3))).astype(F)   # all eight corners in the new block
    g.upload(*esdf_case.random_field(new, vps, 81))
    before = g.esdf_sample(inside)
    assert (before["status"] == 0).all() and np.isnan(before["distance"]).all(), before["stats"]   # a snapshot: the block joined later
    M.assert_same(before, M.sample(M.store_of(g), inside, VOXEL), "before the refresh")
    g.esdf_refresh()
    store = M.store_of(g)
    after, want = check_sample(g, store, inside, "after the refresh")
    assert want["stats"]["points_unknown"] < 300 and want["stats"]["points_interpolated"] > 0, want["stats"]
    xyz = mixed_points(MIXED_SEED, 1501)
    check_sample(g, store, xyz, "the whole box after the refresh")
    # a removed block reads as default records at once: the store follows the tiles that moved
    gone = idx0[len(idx0) // 2][None]
    p_gone = ((gone[0] * vps + 0.5) * VOXEL + rng.uniform(VOXEL, (vps - 2) * VOXEL, (200, 3))).astype(F)
    assert (g.esdf_sample(p_gone)["status"] != 0).any()
    g.remove_blocks(gone)
    got = g.esdf_sample(p_gone)
    assert (got["status"] == 0).all(), got["stats"]
    store = M.store_of(g)
    check_sample(g, store, np.concatenate([xyz, p_gone, inside]), "after the removal")
    sw = sweep_segments(SWEEP_SEED)[:120]
    M.assert_same(g.esdf_sweep(sw), M.sweep(store, sw, VOXEL), "sweep after the removal")
    g.esdf_refresh()
    check_sample(g, M.store_of(g), np.concatenate([xyz, p_gone, inside]), "refreshed after the removal")
    g.close()
    return dict(want["stats"])


def case_chunks(spec):
    """Run with KS_DEBUG=1 KS_ESDF_READ_CHUNK=<chunk>: the same bytes as the model, which knows no chunks — and, in the GPU tier, as
    a context created without the switch."""
    chunk = spec["chunk"]
    assert os.environ.get("KS_DEBUG") == "1" and int(os.environ.get("KS_ESDF_READ_CHUNK", "0")) == chunk
    g = _stored(spec)
    store = M.store_of(g)
    xyz = mixed_points(MIXED_SEED, 1003)
    assert (len(xyz) - 1) // chunk >= 3 and len(xyz) % chunk != 0
    got, want = check_sample(g, store, xyz, "chunked sample")
    sw = sweep_segments(SWEEP_SEED)
    assert (len(sw) - 1) // chunk >= 1
    M.assert_same(g.esdf_sweep(sw), M.sweep(store, sw, VOXEL), "chunked sweep")
    o, du, dv = oblique_plane()
    assert 37 * 23 > 3 * chunk
    M.assert_same(g.esdf_slice(o, du, dv, 37, 23), M.slice_image(store, o, du, dv, 37, 23, VOXEL), "banded slice")
    os.environ.pop("KS_ESDF_READ_CHUNK")
    plain = _stored(spec)                                                       # (the switch is read when a context is created)
    os.environ["KS_ESDF_READ_CHUNK"] = str(chunk)
    M.assert_same(plain.esdf_sample(xyz), got, "unchunked call")
    plain.close()
    g.close()
    return dict(want["stats"])


def oblique_plane():
    """37 x 23 pixels of 4.1 cm through the sphere, no axis parallel to du or dv; it leaves the box at two corners."""
    du = np.array([0.8, 0.5, 0.33]) / np.linalg.norm([0.8, 0.5, 0.33]) * 0.041
    dv = np.cross([0.1, -0.3, 0.9], du)
    dv = dv / np.linalg.norm(dv) * 0.041
    origin = np.array([0.01, -0.02, 0.03]) - 18 * du - 11 * dv
    return origin.astype(F), du.astype(F), dv.astype(F)


def case_slice(spec):
    g = _stored(spec)
    store = M.store_of(g)
    o, du, dv = oblique_plane()
    w, h = 37, 23
    got = g.esdf_slice(o, du, dv, w, h)
    want = M.slice_image(store, o, du, dv, w, h, VOXEL)
    M.assert_same(got, want, "oblique")
    assert got["distance"].shape == (h, w) and got["gradient"].shape == (h, w, 3)
    # the plane lies inside the box but for two corners: nearly every pixel of the sphere is interpolated; with holes (a tenth of the
    # voxels unobserved: 0.9^8 = 43 % of the cells complete, less where a block is missing) the three statuses mix
    if spec["field"] == "sphere":
        assert want["stats"]["points_interpolated"] > w * h * 0.9, want["stats"]
    else:
        assert min(want["stats"].values()) >= w * h * 0.05, want["stats"]
    assert (got["distance"][got["status"] == 2] < 0).any()
    # axis-aligned, at the tile seam z = 0 (the cell face between the voxel layers -1 and 0), one pixel per voxel, beyond the box on all sides
    o2, du2, dv2 = np.array([-HALF - 3 * VOXEL, -HALF - 2 * VOXEL, 0.0], F), np.array([VOXEL, 0, 0], F), np.array([0, VOXEL, 0], F)
    w2, h2 = 39, 37
    got2 = g.esdf_slice(o2, du2, dv2, w2, h2)
    want2 = M.slice_image(store, o2, du2, dv2, w2, h2, VOXEL)
    M.assert_same(got2, want2, "seam")
    assert min(want2["stats"].values()) > 0, want2["stats"]
    # every output but one NULL
    for name in ("distance", "gradient", "status", "label", "flags"):
        only = g.esdf_slice(o, du, dv, w, h, outputs=(name,))
        assert set(only) == {name, "stats"} and only[name].tobytes() == got[name].tobytes() and only["stats"] == got["stats"], name
    assert g.esdf_slice(o, du, dv, w, h, outputs=("label",), stats=False)["label"].tobytes() == got["label"].tobytes()
    # one pixel, one row, one column
    for ww, hh in ((1, 1), (17, 1), (1, 9)):
        M.assert_same(g.esdf_slice(o2, du2, dv2, ww, hh), M.slice_image(store, o2, du2, dv2, ww, hh, VOXEL), "%d x %d" % (ww, hh))
    g.close()
    return dict(want["stats"])


def sweep_segments(seed):
    """About 300 segments over the box and beyond it: random ones of 0.05 - 1.5 m, through the sphere's surface, ending exactly on a
    sample, of zero length, with non-finite endpoints, and far too long."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-HALF - 0.2, HALF + 0.2, (240, 3))
    d = rng.normal(size=(240, 3))
    b = a + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.05, 1.5, (240, 1))
    seg = [np.concatenate([a, b], axis=1)]
    c = np.array(esdf_case.mesh_case.SPHERE_CENTRE)
    dirs = rng.normal(size=(24, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    seg.append(np.concatenate([c + dirs * 0.75, c + dirs * 0.3], axis=1))       # from free space through the surface
    seg.append(np.concatenate([c + dirs[:8] * 0.7, c + dirs[:8] * 0.74], axis=1))   # short, in free space, along the gradient
    k = np.arange(1, 9)[:, None] * 0.0625                                        # ENDS_ON_A_SAMPLE: in the corner of the box, where the ESDF is max_distance_m
    seg.append(np.concatenate([np.tile([[-0.75, -0.75, -0.75]], (8, 1)), np.array([[-0.75, -0.75, -0.75]]) + k * np.array([[1.0, 0, 0]])], axis=1))
    p = rng.uniform(-HALF, HALF, (8, 3))
    seg.append(np.concatenate([p, p], axis=1))                                   # zero length
    bad = np.concatenate([a[:6], b[:6]], axis=1)
    bad[0, 0], bad[1, 4], bad[2, 5], bad[3, 2] = np.nan, np.nan, np.inf, -np.inf
    bad[4, 3:] = bad[4, :3] + np.array([150.0, 0, 0])                            # longer than (max_samples - 2) * min_step = 102.35 m
    bad[5, :3], bad[5, 3:] = [3e38, 0, 0], [-3e38, 0, 0]                         # L overflows
    seg.append(bad)
    return np.concatenate(seg).astype(F)


def case_sweep(spec):
    g = _stored(spec)
    store = M.store_of(g)
    seg = sweep_segments(SWEEP_SEED)
    out = {}
    results = {}
    for name, cfg in (("default", {}), ("unknown_is_free", dict(unknown_is_free=1)), ("radius_0", dict(radius_m=0.0)),
                      ("radius_above_every_clearance", dict(radius_m=0.45)), ("min_step_1cm_few_samples", dict(min_step_m=0.01, max_samples=64)),
                      ("radius_10cm_unknown_is_free", dict(radius_m=0.1, unknown_is_free=1)), ("ends_on_a_sample", dict(radius_m=ENDS_RADIUS))):
        got = g.esdf_sweep(seg, **cfg)
        want = M.sweep(store, seg, VOXEL, **cfg)
        M.assert_same(got, want, name)
        st = want["stats"]
        assert st["segments_free"] + st["segments_collision"] + st["segments_unknown"] + st["segments_invalid"] == len(seg)
        results[name], out[name] = got, st
    d = results["default"]
    assert all(out["default"]["segments_" + k] > 0 for k in ("free", "collision", "unknown", "invalid")), out["default"]
    assert (d["status"] != results["unknown_is_free"]["status"]).any()
    inv = d["status"] == M.INVALID
    assert (d["t_stop"][inv] == 0).all() and np.isinf(d["min_clearance"][inv]).all() and (d["t_min"][inv] == 0).all() and (d["status"][-6:] == M.INVALID).all()
    # max_distance_m = 0.4: with a radius above it every known sample collides, at t = 0 where the start is known
    big = results["radius_above_every_clearance"]
    assert out["radius_above_every_clearance"]["segments_free"] == 0 and ((big["status"] == M.COLLISION) & (big["t_stop"] == 0)).sum() > 50
    assert out["min_step_1cm_few_samples"]["segments_invalid"] > out["default"]["segments_invalid"]   # L > 62 * 0.01
    free = d["status"] == M.FREE
    L = np.linalg.norm(seg[:, 3:].astype(np.float64) - seg[:, :3].astype(np.float64), axis=1)
    assert np.allclose(d["t_stop"][free], L[free], rtol=1e-6, atol=0)
    # clearance 2^-4 exactly at every sample of the rows ENDS_ON_A_SAMPLE: t = 0, 2^-4, 2^-3, ... reaches L = k * 2^-4 without the clamp
    if spec["field"] == "sphere":
        e = results["ends_on_a_sample"]
        assert (e["status"][ENDS_ON_A_SAMPLE] == M.FREE).all() and (e["min_clearance"][ENDS_ON_A_SAMPLE] == F(0.0625)).all(), e["min_clearance"][ENDS_ON_A_SAMPLE]
        assert (e["t_stop"][ENDS_ON_A_SAMPLE] == (np.arange(1, 9) * F(0.0625)).astype(F)).all() and (e["t_min"][ENDS_ON_A_SAMPLE] == 0).all()
    # every output but one NULL, and no stats
    for name in ("status", "t_stop", "min_clearance", "t_min"):
        only = g.esdf_sweep(seg, outputs=(name,), stats=False)
        assert only[name].tobytes() == d[name].tobytes(), name
    M.assert_same(g.esdf_sweep(seg), d, "second call")
    g.close()
    return out


def _snapshot_of(g):
    idx, t, s = g.download()
    n, nr = ctypes.c_size_t(), ctypes.c_size_t()
    from kimera_semantics_amd import binding as B
    assert B.lib().ks_count_updated_voxels(g._h, ctypes.byref(n), ctypes.byref(nr)) == 0
    return dict(updated=g.updated_block_indices(reset=False).tobytes(), counted=(n.value, nr.value), idx=idx.tobytes(), tsdf=t.tobytes(),
                sem=s.tobytes(), esdf=g.esdf_blocks(idx).tobytes())


def case_reads_only(spec):
    vps = spec["vps"]
    xyz, seg = mixed_points(MIXED_SEED, 700), sweep_segments(SWEEP_SEED)
    o, du, dv = oblique_plane()

    def prepared():
        g = _stored(spec)
        g.mesh()
        g.updated_block_indices(reset=True)
        g.upload(*esdf_case.random_field([(0, 0, 0)], vps, 91))       # written voxels: `updated`, `dirty`, both stale bits
        f = esdf_case.mesh_case._frames(1, 64, 48)[0]
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        return g

    def reads(g):
        g.esdf_sample(xyz)
        g.esdf_slice(o, du, dv, 37, 23)
        g.esdf_sweep(seg)

    def followers(g):
        return dict(stale=g.esdf_refresh()["tiles_stale"], meshed=g.mesh(only_stale=True).stats["blocks_meshed"])

    g = prepared()
    before = _snapshot_of(g)
    assert len(before["updated"]) > 0 and before["counted"][0] > 0
    reads(g)
    after = _snapshot_of(g)
    assert after == before, [k for k in before if before[k] != after[k]]
    with_reads = followers(g)
    g.close()
    g = prepared()                                                    # the same history without the reads
    without = followers(g)
    g.close()
    assert with_reads == without and with_reads["stale"] > 0 and with_reads["meshed"] > 0, (with_reads, without)
    return with_reads


def case_errors(spec):
    from kimera_semantics_amd import binding as B
    L = B.lib()
    vps = 8
    g = esdf_case._uploaded("sphere", vps)
    xyz, seg = mixed_points(MIXED_SEED, 100), sweep_segments(SWEEP_SEED)[:50]
    o, du, dv = oblique_plane()
    calls = [lambda: g.esdf_sample(xyz), lambda: g.esdf_slice(o, du, dv, 8, 8), lambda: g.esdf_sweep(seg),
             lambda: g.esdf_sample_device(8, 1, d_distance=8), lambda: g.esdf_slice_device(o, du, dv, 8, 8, d_distance=8),
             lambda: g.esdf_sweep_device(8, 1, d_status=8)]
    for call in calls:                                                          # no stored ESDF (the device addresses are never used)
        assert "no ESDF is stored" in str(refused(B.KS_ERR_INVALID_ARG, call))
    g.esdf_update(**cfg_of(spec))
    idx = g.block_indices()
    before = g.esdf_blocks(idx).tobytes()
    want = g.esdf_sample(xyz)
    st, ss, sc = B.KsEsdfSampleStats(), B.KsEsdfSweepStats(), g.esdf_sweep_config()
    d, s8 = np.zeros(100, F), np.zeros(100, np.uint8)
    P = lambda a: a.ctypes.data
    # NULL ctx
    assert L.ks_esdf_sample(None, P(xyz), 100, P(d), None, None, None, None, None) == B.KS_ERR_INVALID_ARG
    assert L.ks_esdf_sample_device(None, P(xyz), 100, P(d), None, None, None, None, None) == B.KS_ERR_INVALID_ARG
    assert L.ks_esdf_slice(None, P(o), P(du), P(dv), 8, 8, P(d), None, None, None, None, None) == B.KS_ERR_INVALID_ARG
    assert L.ks_esdf_slice_device(None, P(o), P(du), P(dv), 8, 8, P(d), None, None, None, None, None) == B.KS_ERR_INVALID_ARG
    assert L.ks_esdf_sweep(None, P(seg), 50, ctypes.byref(sc), P(s8), None, None, None, None) == B.KS_ERR_INVALID_ARG
    assert L.ks_esdf_sweep_device(None, P(seg), 50, ctypes.byref(sc), P(s8), None, None, None, None) == B.KS_ERR_INVALID_ARG
    assert L.ks_esdf_sweep_default_config(None) == B.KS_ERR_INVALID_ARG
    # NULL input with n > 0; every output NULL
    for fn in (L.ks_esdf_sample, L.ks_esdf_sample_device):
        assert fn(g._h, None, 100, P(d), None, None, None, None, ctypes.byref(st)) == B.KS_ERR_INVALID_ARG
        assert fn(g._h, P(xyz), 100, None, None, None, None, None, ctypes.byref(st)) == B.KS_ERR_INVALID_ARG
        assert fn(g._h, None, 0, None, None, None, None, None, ctypes.byref(st)) == 0      # n = 0 looks at no pointer
    for fn in (L.ks_esdf_slice, L.ks_esdf_slice_device):
        assert fn(g._h, P(o), P(du), P(dv), 8, 8, None, None, None, None, None, ctypes.byref(st)) == B.KS_ERR_INVALID_ARG
        assert fn(g._h, None, P(du), P(dv), 8, 8, P(d), None, None, None, None, ctypes.byref(st)) == B.KS_ERR_INVALID_ARG
    for fn in (L.ks_esdf_sweep, L.ks_esdf_sweep_device):
        assert fn(g._h, None, 50, ctypes.byref(sc), P(s8), None, None, None, ctypes.byref(ss)) == B.KS_ERR_INVALID_ARG
        assert fn(g._h, P(seg), 50, ctypes.byref(sc), None, None, None, None, ctypes.byref(ss)) == B.KS_ERR_INVALID_ARG
        assert fn(g._h, P(seg), 50, None, P(s8), None, None, None, ctypes.byref(ss)) == B.KS_ERR_INVALID_ARG
        assert fn(g._h, P(seg), 1 << 32, ctypes.byref(sc), P(s8), None, None, None, ctypes.byref(ss)) == B.KS_ERR_INVALID_ARG   # (refused before it is read)
        assert fn(g._h, None, 0, ctypes.byref(sc), None, None, None, None, ctypes.byref(ss)) == 0
    # the image and the plane
    for w, h in ((0, 8), (8, 0), (-1, 8), (8193, 8), (8, 8193)):
        refused(B.KS_ERR_INVALID_ARG, lambda: g.esdf_slice(o, du, dv, w, h))
        refused(B.KS_ERR_INVALID_ARG, lambda: g.esdf_slice_device(o, du, dv, w, h, d_distance=8))
    for bad in (np.nan, np.inf, -np.inf):
        for which in range(3):
            for axis in range(3):
                plane = [o.copy(), du.copy(), dv.copy()]
                plane[which][axis] = bad
                refused(B.KS_ERR_INVALID_ARG, lambda: g.esdf_slice(*plane, 8, 8))
                refused(B.KS_ERR_INVALID_ARG, lambda: g.esdf_slice_device(*plane, 8, 8, d_distance=8))
    # the sweep's configuration
    for name in ("radius_m", "min_step_m"):
        for bad in (-0.1, float("nan"), float("inf"), float("-inf")):
            refused(B.KS_ERR_INVALID_ARG, lambda: g.esdf_sweep(seg, **{name: bad}))
            refused(B.KS_ERR_INVALID_ARG, lambda: g.esdf_sweep_device(8, 1, d_status=8, **{name: bad}))
    for bad in (1, 0, -5, 65537):
        refused(B.KS_ERR_INVALID_ARG, lambda: g.esdf_sweep(seg, max_samples=bad))
        refused(B.KS_ERR_INVALID_ARG, lambda: g.esdf_sweep_device(8, 1, d_status=8, max_samples=bad))
    for ok in (2, 65536):
        M.assert_same(g.esdf_sweep(seg, max_samples=ok), M.sweep(M.store_of(g), seg, VOXEL, max_samples=ok), "max_samples %d" % ok)
    # ... and none of these changed the store or what the calls return
    assert g.esdf_blocks(idx).tobytes() == before
    M.assert_same(g.esdf_sample(xyz), want, "after the refusals")
    g.clear()
    for call in calls:
        refused(B.KS_ERR_INVALID_ARG, call)                                     # clear() drops the stored ESDF
    g.close()
    # a marcher context of the exact multi-GPU mode holds no voxel data
    from tests import mesh_case
    marcher, owner = (mesh_case._integrator(1, 64, 48) for _ in range(2))
    f = mesh_case._frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    for call in (lambda: marcher.esdf_sample(xyz), lambda: marcher.esdf_slice(o, du, dv, 8, 8), lambda: marcher.esdf_sweep(seg),
                 lambda: marcher.esdf_sample_device(8, 1, d_distance=8), lambda: marcher.esdf_slice_device(o, du, dv, 8, 8, d_distance=8),
                 lambda: marcher.esdf_sweep_device(8, 1, d_status=8)):
        refused(B.KS_ERR_UNSUPPORTED, call)
    owner.esdf_update(**cfg_of(spec))
    assert sum(owner.esdf_sample(xyz)["stats"].values()) == len(xyz)           # (the owner holds the map)
    marcher.close()
    owner.close()
    # a context in a failed state (the pool is full: sticky until a clear)
    small = mesh_case._integrator(0, 64, 48, max_tiles=8)
    try:
        small.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        raise AssertionError("a frame fitted 8 tiles")
    except B.KsError as e:
        assert e.code == B.KS_ERR_POOL_FULL, e
    for call in (lambda: small.esdf_sample(xyz), lambda: small.esdf_slice(o, du, dv, 8, 8), lambda: small.esdf_sweep(seg),
                 lambda: small.esdf_sample_device(8, 1, d_distance=8), lambda: small.esdf_slice_device(o, du, dv, 8, 8, d_distance=8),
                 lambda: small.esdf_sweep_device(8, 1, d_status=8)):
        assert "failed state" in str(refused(B.KS_ERR_INVALID_ARG, call))
    small.close()
    return {}


CASES = {"mixed": case_mixed, "edges": case_edges, "snapshot": case_snapshot, "chunks": case_chunks, "slice": case_slice, "sweep": case_sweep,
         "reads_only": case_reads_only, "errors": case_errors}

# name -> (spec, extra environment): the same cases in both tiers
SPECS = {}
for _field in ("sphere", "holes"):
    for _vps in (8, 16):
        for _case in ("mixed", "edges", "sweep"):
            SPECS["%s_%s_vps%d" % (_case, _field, _vps)] = (dict(case=_case, field=_field, vps=_vps), {})
SPECS.update({
    "slice_sphere_vps8": (dict(case="slice", field="sphere", vps=8), {}),
    "slice_holes_vps16": (dict(case="slice", field="holes", vps=16), {}),
    "snapshot_sphere_vps8": (dict(case="snapshot", field="sphere", vps=8), {}),
    "snapshot_holes_vps16": (dict(case="snapshot", field="holes", vps=16), {}),
    "chunks_holes_vps16": (dict(case="chunks", field="holes", vps=16, chunk=256), {"KS_DEBUG": "1", "KS_ESDF_READ_CHUNK": "256"}),
    "reads_only_sphere_vps8": (dict(case="reads_only", field="sphere", vps=8), {}),
    "errors": (dict(case="errors"), {}),
})


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("ESDF_READ_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
