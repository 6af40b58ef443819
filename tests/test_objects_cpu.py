"""CPU tier of the object instances (DESIGN.md, section "Object instances").
1. the NumPy model (tests/objects_model.py) on its own: per label it equals scipy.ndimage.label with the full 3 x 3 x 3 structure,
   and the analytic sphere is exactly one object of label 5 centred on the sphere — the yardstick is validated before it judges
   anything; the hand-built fields hold what the cases say they hold;
2. the DEVICE CODE on the host functional model (tools/emu) against the model, byte for byte: one child process per case
   (tests/objects_case.py), started side by side like those of tests/test_emu_parity.py.
Part 1 needs no library: it judges the yardstick against scipy and so passes wherever the model and the fields exist.  What fails
without the feature is part 2, tests/test_objects_gpu.py and tests/test_objects_abi.py."""
import json
import sys

import numpy as np
import pytest

from tests import mesh_case, objects_case
from tests import objects_model as M
from tests import test_emu_parity as EP


def _model(kind, vps, **cfg):
    idx, t, s = objects_case.make_field(kind, vps)
    return M.objects_from_blocks(idx, t, s["label"], vps, objects_case.VOXEL, **cfg), (idx, t, s)


@pytest.mark.parametrize("kind,vps", [("random", 8), ("random", 16), ("seams", 8), ("serpentine", 16)])
def test_model_equals_scipy_label_per_label(kind, vps):
    from scipy import ndimage
    m, (idx, t, s) = _model(kind, vps, min_voxels=1)
    _, D, W, L = M.dense_from_blocks(idx, t, s["label"], vps)
    part, lab = M.taking_part(D, W, L, objects_case.VOXEL, dict(M.DEFAULTS))
    flat = np.arange(part.size).reshape(part.shape)

    def canonical(comp, n):   # per voxel the smallest flat index of its component: the partition, whatever the numbering
        low = np.full(n + 1, part.size, np.int64)
        np.minimum.at(low, comp[part], flat[part])
        return np.where(part, low[comp], -1)

    total, want = 0, np.full(part.shape, -1, np.int64)
    for label in np.unique(lab[part]):
        got, n = ndimage.label(part & (lab == label), structure=np.ones((3, 3, 3), int))
        sel = got > 0
        want[sel] = got[sel] - 1 + total
        total += n
    assert total == m.stats["components"] > 0
    assert (canonical(m.components, total) == canonical(want, total)).all()
    sizes = np.bincount(want[part])
    assert sorted(sizes) == sorted(m.records["n_voxels"].tolist())


def test_model_on_the_analytic_sphere_is_one_object_centred_on_it():
    m, _ = _model("sphere", 8)
    assert len(m.records) == 1 and m.records["label"][0] == 5 and m.stats["components"] == 1, m.stats
    c = m.centroids(objects_case.VOXEL)[0]
    assert np.abs(c - np.array(mesh_case.SPHERE_CENTRE)).max() < objects_case.VOXEL, c
    r = m.records[0]
    assert r["n_voxels"] == m.stats["voxels_surface"] > 1000 and (m.ids != M.NONE).sum() == r["n_voxels"]
    lo, hi = (np.array(mesh_case.SPHERE_CENTRE) - mesh_case.SPHERE_RADIUS) / objects_case.VOXEL, (np.array(mesh_case.SPHERE_CENTRE) + mesh_case.SPHERE_RADIUS) / objects_case.VOXEL
    assert (np.abs(r["bb_min"] - lo) < 2).all() and (np.abs(r["bb_max"] - hi) < 2).all()


def test_fields_hold_what_the_cases_are_chosen_for():
    for vps in (8, 16, 32):
        m, _ = _model("seams", vps, min_voxels=1)
        assert objects_case._by_first(m.records) == objects_case.SEAMS_EXPECTED
        m, _ = _model("serpentine", vps)
        assert len(m.records) == 2 and (m.records["n_voxels"] == objects_case.SERPENTINE_VOXELS).all()
        m, _ = _model("random", vps, min_voxels=1)
        n = m.records["n_voxels"]
        assert (n > 1000).sum() >= 1 and (n == 1).sum() >= 100 and objects_case.crossing_a_seam(m.records) >= 20
        assert m.stats["components"] > _model("random", vps)[0].stats["objects"] > 0


# ---- 2. the device code on the functional model: one child per case, started together by test_emu_parity's fixture ----
for _name, _spec in objects_case.SPECS.items():
    EP.JOBS["test_objects_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.objects_case", json.dumps(_spec)], {}, 900, 40 if _spec["case"] in ("lifetime", "errors") else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(objects_case.SPECS))
def test_objects_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "OBJECTS_CASE_OK" in out, out[-3000:] + err[-3000:]
