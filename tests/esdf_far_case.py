"""ESDF cases in which the nearest site is FAR away, shared by both tiers like those of tests/esdf_case.py: the GPU tier
(tests/test_esdf_far_gpu.py) calls run_case in-process, the CPU tier (tests/test_esdf_far_cpu.py) runs it as a child process
on the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.esdf_far_case '<json spec>'
The checker is tests/esdf_model.py in its separable form: the bytes of every record of every block, and the three counts.

Where the other ESDF cases keep every winning site within about 16 voxels, these make the far end of the window decide:
R = 32, 33 (128 staged rows of k_esdf_axis exactly, and one over), 40 (the library's default), 64, 65 and 255 (the largest), that is
g = ceil(R / 8) = 4, 5, 5, 8, 9, 32 neighbour bricks of k_esdf_brick on either side.

  rod(axis, vps)  one block thick, 33 blocks of 8^3 (17 of 16^3) along `axis` from voxel LO = -128 to HI = 135 (143), the other
                  two block coordinates -3 and 5.  Four sites and no others: two positive ones in the plane a = LO, two negative
                  ones in the plane a = HI, so a positive voxel is served from the low end only and a negative one from the high
                  end only, over offsets up to HI - LO.  The positive pair (cross-section (1, 2) label 11, (4, 5) label 4, both
                  +0.03) ties in d2 on u + v = 6 at every a: the label decides.  The negative pair ((6, 5) -0.07 label 2, (3, 2)
                  -0.03 label 9) ties on u + v = 8: |distance| decides, against the order of the labels.  (One more rod is four
                  blocks wide: only there does a winning d2 reach 2^16, at R = 255 with 23 voxels and more across.)
  plate(thin)     12 x 12 x 1 (or 16 x 16 x 1) blocks of 8^3, the thin block coordinate 2, the others around 0; random sites with
                  probability 3e-4: each orientation makes another pair of passes do the long work.  (One more, with a tenth of the
                  sites, so that at R = 100 the winning site is up to 100 voxels away on two axes at once.)

Both put weight 0 on a random 5 % of the voxels, |distance| 0.3 with a random sign on every voxel that is no site, and random
labels 0..20.  The seeds were chosen on the CPU with the model alone; every case asserts on the model, before it looks at the
device's result, what the inputs are for (the floors below)."""
import json
import os
import sys

import numpy as np

from tests import esdf_case, mesh_case
from tests import esdf_model as M
from tests import esdf_refresh_case as RC

VOXEL = esdf_case.VOXEL
LO = -128
ROD_BLOCKS = {8: 33, 16: 17}
CROSS = (-3, 5)                   # the block coordinates of a rod on its other two axes, in axis order
ROD_SITES = (("lo", (1, 2), 0.03, 11), ("lo", (4, 5), 0.03, 4), ("hi", (6, 5), -0.07, 2), ("hi", (3, 2), -0.03, 9))
LOW_LABELS, HIGH_LABELS = (4, 11), (2, 9)
NEW_SITE = ((3, 2, 6), 0.03, 7)   # step (c) of the refresh: (along, u, v) in the middle block, distance, label
ROD_SEEDS = {(0, 8, 1): 101, (1, 8, 1): 102, (2, 8, 1): 103, (0, 16, 1): 104, (0, 8, 4): 105}   # (axis, vps, width)
PLATE_SEEDS = {(0, 12, 3e-4): 201, (1, 12, 3e-4): 202, (2, 12, 3e-4): 203, (2, 16, 3e-4): 204, (2, 16, 3e-5): 220}
PLATE_THIN = 2
# floors of what the inputs exercise, counted on the model alone: voxels decided by the secondary keys | found voxels with
# d2 >= (R - 8)^2 | at R = 255: found voxels below the clamp, distinct distances among them
ROD_FLOORS = {8: dict(tied=150, edge=400, unclamped=10000, distinct=5000),
              16: dict(tied=250, edge=1800, unclamped=50000, distinct=20000)}
WIDE_FLOOR = 20                   # found voxels with d2 >= 2^16, on the rod that is four blocks wide
PLATE_FLOORS = dict(tied=50, beyond_32=2000)
_MODELS = {}                      # (field, R) -> Model: a reference is computed once per process and left unchanged
AXES = "xyz"


def hi_of(vps):
    return LO + ROD_BLOCKS[vps] * vps - 1


def cfg_of(spec):
    cfg = esdf_case.cfg_of(spec)
    assert M.reach(cfg["max_distance_m"], VOXEL) == spec["R"], (cfg, spec)
    return cfg


def _others(axis):
    return [a for a in range(3) if a != axis]


def _put(t, s, j, e, distance, label):
    """Voxel e of block j becomes an observed voxel with this distance and label."""
    from kimera_semantics_amd import synth
    lut = synth.default_label_colors()
    t["distance"][j, e], t["weight"][j, e], t["color"][j, e] = distance, 1.0, lut[label]
    s["label"][j, e], s["color"][j, e] = label, lut[label]
    s["priors"][j, e] = np.float32(-0.60205999132)
    s["priors"][j, e, label] = np.float32(-0.1)


def _element(axis, vps, along, u, v):
    local = [0, 0, 0]
    local[axis], (local[_others(axis)[0]], local[_others(axis)[1]]) = along, (u, v)
    return local[0] + vps * (local[1] + vps * local[2])


def rod_block(axis, vps, a):
    """The block of the rod that holds the voxel `a` along the axis."""
    b = [0, 0, 0]
    b[axis], (b[_others(axis)[0]], b[_others(axis)[1]]) = a // vps, CROSS
    return tuple(b)


def rod_field(axis, vps, width=1):
    """width: blocks across, on the first of the other two axes (the sites are in the first of them)."""
    nb = ROD_BLOCKS[vps]
    idx = np.array([rod_block(axis, vps, LO + k * vps) for k in range(nb)], np.int32)
    step = np.eye(3, dtype=np.int32)[_others(axis)[0]]
    idx = np.concatenate([idx + w * step for w in range(width)])
    idx, t, s = esdf_case.random_field(idx, vps, ROD_SEEDS[axis, vps, width], near=0.0, unobserved=0.05)
    for end, (u, v), distance, label in ROD_SITES:
        _put(t, s, 0 if end == "lo" else nb - 1, _element(axis, vps, 0 if end == "lo" else vps - 1, u, v), distance, label)
    return idx, t, s


def plate_field(thin, side, sites=3e-4):
    r = range(-(side // 2), side // 2)
    idx = np.array([[PLATE_THIN if a == thin else (p, q)[_others(thin).index(a)] for a in range(3)] for p in r for q in r], np.int32)
    return esdf_case.random_field(idx, 8, PLATE_SEEDS[thin, side, sites], near=sites, unobserved=0.05)


def _uploaded(spec):
    vps = spec.get("vps", 8)
    g = mesh_case._integrator(0, 64, 48, vps=vps)
    g.upload(*(rod_field(spec["axis"], vps, spec.get("width", 1)) if spec["field"] == "rod" else plate_field(spec["axis"], spec.get("side", 12), spec.get("sites", 3e-4))))
    return g


def _model(g, spec):
    """The model of the field as uploaded, shared between the cases of one process."""
    key = (spec["field"], spec["axis"], spec.get("vps", 8), spec.get("width", 1), spec.get("side", 12), spec.get("sites", 3e-4), spec["R"])
    if key not in _MODELS:
        _MODELS[key] = M.model_of(g, cfg_of(spec), keep_keys=True)
    return _MODELS[key]


def _along(a, axis):
    """A dense [z, y, x] array with `axis` first."""
    return np.moveaxis(a, 2 - axis, 0)


def _far(dense):
    return dense["flags"] == 1


def _clamped(dense, spec):
    return _far(dense) & (np.abs(dense["distance"]) == np.float32(cfg_of(spec)["max_distance_m"]))


def _check_stats(stats, model, what):
    for k in ("voxels_observed", "voxels_fixed", "voxels_clamped"):
        assert stats[k] == model.stats[k], (what, k, stats[k], model.stats[k])


def rod_model_checks(model, spec):
    """What a rod is for, on the model alone."""
    axis, vps, R = spec["axis"], spec.get("vps", 8), spec["R"]
    hi, floors = hi_of(vps), ROD_FLOORS[vps]
    d = _along(model.dense, axis)
    assert model.origin[axis] == LO and d.shape[0] == hi - LO + 1 and model.stats["voxels_fixed"] == 4

    def labels(a, negative):
        p = d[a - LO]
        return p["label"][_far(p) & ((p["distance"] < 0) == negative)]

    # the last plane either end reaches, and the first one it does not
    assert set(labels(LO + R, False).tolist()) == set(LOW_LABELS), labels(LO + R, False)
    assert set(labels(LO + R + 1, False).tolist()) == {255}
    assert set(labels(hi - R, True).tolist()) == set(HIGH_LABELS), labels(hi - R, True)
    assert set(labels(hi - R - 1, True).tolist()) == {255}
    found, d2 = M.found_d2(model)
    out = dict(tied=M.tied_voxels(model, R, form="separable"), edge=int((found & (d2 >= (R - 8) ** 2)).sum()), d2_max=int(d2.max()))
    assert out["tied"] >= floors["tied"] and out["edge"] >= floors["edge"], (out, floors)
    assert out["d2_max"] >= R * R
    if spec.get("width", 1) > 1:   # d2 that does not fit 16 bits: the far corners of the wide rod
        out["wide"] = int((found & (d2 >= 65536)).sum())
        assert R == 255 and out["wide"] >= WIDE_FLOOR, out
    if R == 255:
        free = found & ~_clamped(model.dense, spec)
        out.update(unclamped=int(free.sum()), distinct=len(np.unique(model.dense["distance"][free])))
        assert out["unclamped"] >= floors["unclamped"] and out["distinct"] >= floors["distinct"], (out, floors)
    return out


def plate_model_checks(model, spec):
    R = spec["R"]
    found, d2 = M.found_d2(model)
    out = dict(tied=M.tied_voxels(model, R, form="separable"), beyond_32=int((found & (d2 > 1024)).sum()), d2_max=int(d2.max()),
               sites=model.stats["voxels_fixed"])
    if spec.get("sites", 3e-4) == 3e-4:
        assert out["tied"] >= PLATE_FLOORS["tied"] and out["beyond_32"] >= PLATE_FLOORS["beyond_32"], out
    else:   # the sparse plate: winning sites beyond two staged chunks of k_esdf_axis, and voxels that no site reaches
        out.update(beyond_64=int((found & (d2 > 4096)).sum()), clamped=model.stats["voxels_clamped"])
        assert out["sites"] >= 4 and out["tied"] >= 20 and out["beyond_64"] >= 5000 and out["clamped"] >= 1000, out
    return out


def case_update(spec):
    g = _uploaded(spec)
    model = _model(g, spec)
    out = (rod_model_checks if spec["field"] == "rod" else plate_model_checks)(model, spec)
    idx, rec, stats = g.esdf(**cfg_of(spec))
    M.assert_same(rec, model.blocks(idx), "update")
    _check_stats(stats, model, "update")
    nz, ny, nx = model.dense.shape
    assert stats["box_voxels"] == [nx, ny, nz], (stats, model.dense.shape)
    g.close()
    return dict(out, **{k: stats[k] for k in ("voxels_observed", "voxels_fixed", "voxels_clamped")})


def case_region(spec):
    """ks_esdf_update over a region of one block: the box is the region's tiles dilated by g = ceil(R / 8) tiles, clipped to
    the map's, and the sites outside the region count."""
    axis, R, vps = spec["axis"], spec["R"], 8
    grow = (R + 7) // 8
    g = _uploaded(spec)
    model = _model(g, spec)
    idx = g.block_indices()
    if spec["field"] == "rod":
        block = rod_block(axis, vps, LO + 32)          # four blocks above the low end
        want_box = {axis: 8 * (min(4, grow) + 1 + grow)}
        assert want_box[axis] < hi_of(vps) - LO + 1
        want_box.update({a: 8 for a in _others(axis)})
    else:
        side = spec.get("side", 12)
        block = tuple(PLATE_THIN if a == axis else -(side // 2) for a in range(3))   # a corner
        want_box = {a: 8 if a == axis else 8 * (1 + grow) for a in range(3)}
        assert all(want_box[a] < 8 * side for a in _others(axis))
    region = (list(block), list(block))
    want = model.blocks(idx, region=region)
    inside = (idx == np.array(block)).all(axis=1)
    assert inside.sum() == 1
    served = _far(want[inside]) & (want[inside]["label"] != 255)
    if spec["field"] == "rod":   # the low end serves the region from 32 .. 39 voxels away
        served &= np.isin(want[inside]["label"], LOW_LABELS)
    assert served.sum() >= 100, served.sum()
    stats = g.esdf_update(region=region, **cfg_of(spec))
    rec = g.esdf_blocks(idx)
    M.assert_same(rec, want, "region")
    assert rec[~inside].tobytes() == M.default_records(rec[~inside].shape).tobytes()
    assert stats["box_voxels"] == [want_box[a] for a in range(3)], (stats, want_box)
    w = want[inside]
    counts = dict(voxels_observed=int((w["flags"] & 1).sum()), voxels_fixed=int((w["flags"] == 3).sum()),
                  voxels_clamped=int((_far(w) & (np.abs(w["distance"]) == np.float32(cfg_of(spec)["max_distance_m"]))).sum()))
    for k, v in counts.items():
        assert stats[k] == v, (k, stats, counts)
    g.close()
    return dict(served=int(served.sum()), box=stats["box_voxels"], **counts)


def case_refresh(spec):
    """ks_esdf_refresh on a rod: after every step the whole store and the counts against the model of the map as it is now,
    and the tile counts from the tile coordinates."""
    axis, vps, R = spec["axis"], spec.get("vps", 8), spec["R"]
    hi, grow = hi_of(vps), (R + 7) // 8
    g = _uploaded(spec)
    first = g.esdf_update(**cfg_of(spec))
    _check_stats(first, _model(g, spec), "update")
    lo_block, hi_block, mid_block = (rod_block(axis, vps, a) for a in (LO, hi, 0))
    a_of = _along(np.broadcast_to(np.arange(LO, hi + 1).reshape([-1 if 2 - k == axis else 1 for k in range(3)]),
                                  _model(g, spec).dense.shape), axis)
    out = {}

    if spec.get("width", 1) > 1:
        # the wide rod is here for the final rule of the refresh at d2 >= 2^16: one label of the low-end block changes (label 11
        # becomes 12: still the larger of the pair), every tile is within reach of it and is recomputed, and the positive voxels
        # in the far corners are served across 255 voxels along the rod and 23 and more across it
        idx1, t, s = g.download(np.array([lo_block], np.int32))
        (u, v), distance = ROD_SITES[0][1], ROD_SITES[0][2]
        _put(t, s, 0, _element(axis, vps, 0, u, v), distance, 12)
        g.upload(idx1, t, s)
        found, d2 = M.found_d2(M.model_of(g, cfg_of(spec), keep_keys=True))
        out["wide"] = int((found & (d2 >= 65536)).sum())
        assert out["wide"] >= WIDE_FLOOR, out
        st = g.esdf_refresh()
        _, rec, _ = RC.check_map(g, st, spec, "low end written again")
        RC.check_counts(g, st, [lo_block], spec)
        assert st["tiles_recomputed"] == st["tiles_total"] and (rec["label"] == 12).sum() > 1000
        g.close()
        return dict(out, recomputed=st["tiles_recomputed"])

    # (a) the low-end block changes sign: its sites serve the negative voxels now, and no positive voxel has a site
    g.upload(*RC._flipped(g, lo_block))
    st = g.esdf_refresh()
    _, _, model_a = RC.check_map(g, st, spec, "(a) low end flipped")
    RC.check_counts(g, st, [lo_block], spec)
    if vps == 8:
        assert st["tiles_total"] == 33 and st["tiles_recomputed"] == min(33, 1 + grow), st
    da = _along(model_a.dense, axis)
    positive = _far(da) & (da["distance"] > 0)
    assert positive.sum() > 1000 and (da["label"][positive] == 255).all()
    out["a"] = st["tiles_recomputed"]

    # (b) the high-end block loses its weight: every negative voxel it served has lost its sites
    served = _far(da) & (da["distance"] < 0) & np.isin(da["label"], HIGH_LABELS)
    assert served.sum() > 500
    g.upload(*RC._zero_weight(g, hi_block))
    st = g.esdf_refresh()
    _, _, model_b = RC.check_map(g, st, spec, "(b) high end unobserved")
    RC.check_counts(g, st, [hi_block], spec)
    db = _along(model_b.dense, axis)
    still = served & _far(db)
    assert (db["flags"][a_of > hi - vps] == 0).all() and still.sum() == served[a_of <= hi - vps].sum() > 500
    assert not np.isin(db["label"][still], HIGH_LABELS).any()
    lost = still & (a_of > LO + R)                  # ... and those the flipped low end does not reach have none at all
    assert (db["label"][lost] == 255).all() and (lost.sum() > 100) == (LO + R + 8 <= hi - vps), (lost.sum(), R)
    # more clamped voxels among those that are still observed, and the device's total is the model's (check_map)
    kept = a_of <= hi - vps
    out["b"] = [int(_clamped(da, spec)[kept].sum()), int(_clamped(db, spec)[kept].sum())]
    assert out["b"][1] > out["b"][0], out
    assert st["voxels_clamped"] == model_b.stats["voxels_clamped"] and st["voxels_observed"] < first["voxels_observed"]

    # (c) one new positive site in the middle of the rod: positive voxels have a site again
    (along, u, v), distance, label = NEW_SITE
    idx1, t, s = g.download(np.array([mid_block], np.int32))
    _put(t, s, 0, _element(axis, vps, along, u, v), distance, label)
    g.upload(idx1, t, s)
    st = g.esdf_refresh()
    _, _, model_c = RC.check_map(g, st, spec, "(c) a new site in the middle")
    RC.check_counts(g, st, [mid_block], spec)
    dc = _along(model_c.dense, axis)
    positive = _far(dc) & (dc["distance"] > 0)
    within = np.abs(a_of - along) <= R
    assert positive[within].sum() > 1000 and (dc["label"][positive & within] == label).all() and (dc["label"][positive & ~within] == 255).all()
    assert st["voxels_fixed"] == 3     # (the two of the low end, and this one)
    out["c"] = st["tiles_recomputed"]
    assert len(g.esdf_changed_blocks()) > 0
    g.close()
    return out


CASES = {"update": case_update, "region": case_region, "refresh": case_refresh}
RADII = (32, 33, 40, 64, 65, 255)


def _spec(case, field, axis, R, **kw):
    return dict(case=case, field=field, axis=axis, R=R, max_distance_m=R * VOXEL, **kw)


SPECS = {}
for _case in ("update", "refresh"):
    for _axis in range(3):
        for _r in RADII:
            SPECS["%s_rod_%s_vps8_r%d" % (_case, AXES[_axis], _r)] = _spec(_case, "rod", _axis, _r, vps=8)
    for _r in (40, 255):
        SPECS["%s_rod_x_vps16_r%d" % (_case, _r)] = _spec(_case, "rod", 0, _r, vps=16)
for _axis in range(3):
    SPECS["update_plate_thin_%s_r40" % AXES[_axis]] = _spec("update", "plate", _axis, 40)
    for _r in (40, 100):
        SPECS["region_rod_%s_r%d" % (AXES[_axis], _r)] = _spec("region", "rod", _axis, _r)
for _case in ("update", "refresh"):
    SPECS["%s_wide_rod_x_vps8_r255" % _case] = _spec(_case, "rod", 0, 255, vps=8, width=4)
SPECS["update_plate_thin_z_r100_16x16"] = _spec("update", "plate", 2, 100, side=16)
SPECS["update_sparse_plate_thin_z_r100_16x16"] = _spec("update", "plate", 2, 100, side=16, sites=3e-5)
SPECS["region_plate_thin_z_r40"] = _spec("region", "plate", 2, 40)


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("ESDF_FAR_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
