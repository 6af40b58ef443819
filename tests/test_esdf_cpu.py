"""CPU tier of the batch ESDF (DESIGN.md, section "ESDF").
1. the NumPy model (tests/esdf_model.py) on its own: its separable form equals its brute-force form, and on an analytic
   sphere it is the distance to the sphere to within a voxel diagonal — the yardstick is validated before it judges anything;
2. the DEVICE CODE on the host functional model (tools/emu) against the model, bit for bit: one child process per case
   (tests/esdf_case.py), started side by side like those of tests/test_emu_parity.py;
3. the new symbols and struct layouts through the binding."""
import ctypes
import json
import sys

import numpy as np
import pytest

from tests import esdf_case, esdf_model, mesh_case
from tests import test_emu_parity as EP


def _both_forms(kind, vps, max_distance_m):
    idx, t, s = esdf_case.make_field(kind, vps)
    cfg = dict(min_distance_m=esdf_case.MIN_DISTANCE, max_distance_m=max_distance_m)
    a = esdf_model.esdf_from_blocks(idx, t, s["label"], vps, esdf_case.VOXEL, form="brute", **cfg)
    b = esdf_model.esdf_from_blocks(idx, t, s["label"], vps, esdf_case.VOXEL, form="separable", **cfg)
    return idx, a, b


@pytest.mark.parametrize("kind,vps,max_distance_m", [("random", 8, 0.4), ("holes", 16, 0.55)])
def test_separable_model_equals_brute_force_model(kind, vps, max_distance_m):
    idx, a, b = _both_forms(kind, vps, max_distance_m)
    esdf_model.assert_same(b.blocks(idx), a.blocks(idx), kind)
    assert a.stats == b.stats and a.stats["voxels_fixed"] > 500
    assert (a.dense["flags"] == 1).sum() > 5000 and (a.dense["flags"] == 0).sum() > 1000


def test_separable_tie_count_equals_brute_force_tie_count():
    """tied_voxels in both forms on the random field of the ties case: the separable form counts the rods and plates of
    tests/esdf_far_case.py, whose windows the brute form cannot walk."""
    idx, t, s = esdf_case.make_field("random", 8)
    m = esdf_model.esdf_from_blocks(idx, t, s["label"], 8, esdf_case.VOXEL, form="brute", keep_keys=True,
                                    min_distance_m=esdf_case.MIN_DISTANCE, max_distance_m=0.4)
    R = esdf_model.reach(0.4, esdf_case.VOXEL)
    brute, separable = esdf_model.tied_voxels(m, R), esdf_model.tied_voxels(m, R, form="separable")
    assert R == 8 and brute == separable >= 1000, (brute, separable)
    found, d2 = esdf_model.found_d2(m)
    assert found.sum() > 5000 and d2[found].min() >= 1 and d2[found].max() <= 3 * R * R and (d2[~found] == 0).all()


def test_conditions_that_keep_the_cases_at_32_and_64_voxels_per_side_from_being_empty():
    """What case_upload asserts beside the comparison, with the model alone (separable form) on the fields of the new cases."""
    for name, spec in esdf_case.SPECS.items():
        if spec["case"] != "upload" or spec["vps"] < 32 or spec.get("max_distance_m") != 0.4:
            continue
        idx, t, s = esdf_case.make_field(spec["field"], spec["vps"])
        m = esdf_model.esdf_from_blocks(idx, t, s["label"], spec["vps"], esdf_case.VOXEL, form="separable", keep_keys=(spec["field"] == "random"),
                                        min_distance_m=esdf_case.MIN_DISTANCE, max_distance_m=0.4)
        assert m.stats["voxels_observed"] > 1000 and m.stats["voxels_fixed"] > 500, (name, m.stats)
        if spec["field"] == "sphere":
            assert m.stats["voxels_clamped"] > 0 and m.blocks(idx)["distance"].min() == -np.float32(0.4), name
        if spec["field"] == "random":
            assert esdf_model.tied_voxels(m, 8, form="separable") >= 1000, name


def test_model_on_an_analytic_sphere_is_the_distance_to_the_sphere():
    vps = 8
    idx, t, s = esdf_case.make_field("sphere", vps)
    m = esdf_model.esdf_from_blocks(idx, t, s["label"], vps, esdf_case.VOXEL, min_distance_m=esdf_case.MIN_DISTANCE, max_distance_m=0.55)
    nz, ny, nx = m.dense.shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = (np.stack([x, y, z], axis=-1) + m.origin + 0.5) * esdf_case.VOXEL
    true = np.linalg.norm(p - np.array(mesh_case.SPHERE_CENTRE), axis=-1) - mesh_case.SPHERE_RADIUS
    d = m.dense["distance"].astype(np.float64)
    assert (m.dense["flags"] & 1).all()
    band = m.dense["flags"] == 3
    assert (np.abs(true[band]) < esdf_case.MIN_DISTANCE + 1e-6).all() and np.abs(d[band] - true[band]).max() < 1e-6
    free = (m.dense["flags"] == 1) & (np.abs(d) < 0.55)          # away from the clamp
    assert free.sum() > 10000
    assert np.abs(d[free] - true[free]).max() <= np.sqrt(3.0) * esdf_case.VOXEL
    assert (np.sign(d[free]) == np.sign(true[free])).all() and (m.dense["label"][free] == 5).all()
    clamped = (m.dense["flags"] == 1) & (np.abs(d) == np.float32(0.55))
    assert clamped.sum() == m.stats["voxels_clamped"] > 0 and (np.abs(true[clamped]) > 0.55 - np.sqrt(3.0) * esdf_case.VOXEL).all()


# ---- 2. the device code on the functional model: one child per case, started together by test_emu_parity's fixture ----
for _name, _spec in esdf_case.SPECS.items():
    EP.JOBS["test_esdf_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.esdf_case", json.dumps(_spec)], {}, 900, 30 if _spec["case"] in ("region", "errors", "snapshot") else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(esdf_case.SPECS))
def test_esdf_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "ESDF_CASE_OK" in out, out[-3000:] + err[-3000:]


def test_esdf_symbols_and_struct_layouts():
    from kimera_semantics_amd import binding as B
    for sym in ("ks_esdf_default_config", "ks_esdf_update", "ks_esdf_download_blocks", "ks_esdf_query"):
        assert sym in B.ABI_SYMBOLS and hasattr(B.lib(), sym), sym
    assert ctypes.sizeof(B.KsEsdfConfig) == 48 and B.KsEsdfConfig.max_workspace_bytes.offset == 40 and B.KsEsdfConfig.region_min.offset == 16
    assert ctypes.sizeof(B.KsEsdfStats) == 56 and B.KsEsdfStats.workspace_bytes.offset == 48
    assert B.ESDF_DTYPE.itemsize == 8 and B.ESDF_DTYPE == esdf_model.RECORD_DTYPE
    cfg = B.KsEsdfConfig()
    assert B.lib().ks_esdf_default_config(ctypes.byref(cfg)) == 0
    assert cfg.min_weight == np.float32(1e-6) and cfg.min_distance_m == np.float32(0.2) and cfg.max_distance_m == 2.0
    assert cfg.use_region == 0 and cfg.max_workspace_bytes == 8 << 30
    assert B.lib().ks_esdf_default_config(None) == B.KS_ERR_INVALID_ARG
