"""CPU tier of the view rendering (DESIGN.md, section "View rendering").
1. the NumPy model (tests/render_model.py) on analytic fields: hit points on the sphere and on the plane, normals against
   the sphere's own — the yardstick is validated before it judges anything;
2. the conditions that keep the shared cases (tests/render_case.py) from being empty, with the model alone;
3. the round trip depth image -> map -> rendered depth, a statement about the contract, with the model on the map the
   functional model integrates;
4. the DEVICE CODE on the host functional model (tools/emu) against the model, bit for bit: one child process per case,
   started side by side like those of tests/test_emu_parity.py."""
import json
import sys

import numpy as np
import pytest

from tests import mesh_case, render_case, render_model
from tests import test_emu_parity as EP

VOXEL = render_case.VOXEL
_VIEWS = {}


def view(field, camera="front", size=(61, 45), vps=8):
    """The model's view of an analytic field, computed once per process."""
    key = (field, camera, size, vps)
    if key not in _VIEWS:
        idx, t, s = mesh_case.make_field(field, vps)
        K = render_case.K_ODD if size == (61, 45) else render_case.K_EVEN
        _VIEWS[key] = render_model.render_from_blocks(idx, t, s, vps, VOXEL, render_case.CAMERAS[camera], K, size[0], size[1])
    return _VIEWS[key]


def fraction(m):
    return m["stats"]["pixels_hit"] / float(m["hit"].size)


def test_model_hit_points_lie_on_the_sphere():
    m = view("sphere")
    p = m["p_hit"][m["hit"]].astype(np.float64)
    err = np.abs(np.linalg.norm(p - np.array(mesh_case.SPHERE_CENTRE), axis=1) - mesh_case.SPHERE_RADIUS) / VOXEL
    print("sphere: largest distance of a hit point from the sphere = %.4f voxel over %d hits" % (err.max(), len(p)))
    assert len(p) > 1000 and err.max() < 0.1          # (measured: 0.028 voxel; the mesh test allows 0.2 on the same field)
    d = m["depth"][m["hit"]]
    assert np.isfinite(d).all() and (d > 0.3).all() and (d < 1.2).all()
    assert np.isnan(m["depth"][~m["hit"]]).all() and (m["labels"][~m["hit"]] == 255).all() and (m["labels"][m["hit"]] == 5).all()
    assert not m["rgba"][~m["hit"]].any() and not m["normals"][~m["hit"]].any()


def test_model_hit_points_lie_on_the_plane():
    m = view("plane", camera="back")
    n = np.array([0.31, -0.52, 0.79])
    p = m["p_hit"][m["hit"]].astype(np.float64)
    err = np.abs(p @ (n / np.linalg.norm(n)) - 0.0613) / VOXEL
    print("plane: largest distance of a hit point from the plane = %.2e voxel over %d hits" % (err.max(), len(p)))
    assert len(p) > 1000 and err.max() < 1e-3          # (trilinear interpolation of a linear field is exact up to rounding)
    nrm = m["normals"][m["hit"]].astype(np.float64)
    inner = np.linalg.norm(nrm, axis=1) > 0           # (at the rim of the box a normal's six samples are not all valid)
    assert inner.sum() > 0.8 * len(p)
    # the gradient of a linear field is exact up to the rounding of six samples (a few 1e-7 of its length): far below 0.01
    # degrees (the angle from the cross product: the arc cosine of a rounded 1 - 1e-8 would itself be off by more)
    sine = np.linalg.norm(np.cross(nrm[inner], n / np.linalg.norm(n)), axis=1)
    print("plane: largest angle between a normal and the plane's = %.2e degrees" % np.degrees(np.arcsin(sine.max())))
    assert np.degrees(np.arcsin(sine.max())) < 0.01 and (nrm[inner] @ n > 0).all()


SPHERE_NORMAL_MEASURED_DEG = 0.089   # the largest angle the model shows on this view (the test prints the exact figure)


def test_model_normals_agree_with_the_spheres():
    m = view("sphere")
    p = m["p_hit"][m["hit"]].astype(np.float64) - np.array(mesh_case.SPHERE_CENTRE)
    true = p / np.linalg.norm(p, axis=1)[:, None]
    nrm = m["normals"][m["hit"]].astype(np.float64)
    assert (np.abs(np.linalg.norm(nrm, axis=1) - 1.0) < 1e-5).all()   # (every one of the six samples is valid on this view)
    ang = np.degrees(np.arccos(np.clip((nrm * true).sum(axis=1), -1, 1)))
    print("sphere: largest angle between a normal and the sphere's = %.4f degrees" % ang.max())
    assert ang.max() < 2 * SPHERE_NORMAL_MEASURED_DEG


def test_conditions_that_keep_the_cases_from_being_empty():
    assert 0.5 <= fraction(view("sphere")) <= 0.9
    assert 0.5 <= fraction(view("sphere", size=(64, 48))) <= 0.9
    assert fraction(view("plane", camera="back", size=(64, 48))) >= 0.5
    for vps in (8, 16):
        assert fraction(view("holes", size=(64, 48), vps=vps)) >= 0.05
    assert fraction(view("sphere", camera="corner", size=(64, 48))) >= 0.1
    inside = view("sphere", camera="inside", size=(64, 48))
    assert inside["stats"]["pixels_hit"] == 0 and inside["stats"]["samples"] > 64 * 48 * 20   # all samples are negative, then invalid
    assert view("plane", camera="front", size=(64, 48))["stats"]["pixels_hit"] == 0
    two = view("two_label", size=(64, 48))
    assert {3, 7} <= set(np.unique(two["labels"]))
    left = two["p_hit"][..., 0] < -VOXEL
    assert (two["labels"][two["hit"] & left] == 3).all() and (two["labels"][two["hit"] & (two["p_hit"][..., 0] > VOXEL)] == 7).all()


# ---- 3. + 4. one child per case on the functional model, started together by test_emu_parity's fixture ----
for _name, _spec in render_case.SPECS.items():
    EP.JOBS["test_render_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.render_case", json.dumps(_spec)], {}, 900, 20 if _spec["case"] in ("integrated", "side_effects") else 5)
EP.JOBS["test_round_trip_of_a_depth_image_through_the_map"] = (
    [sys.executable, "-m", "tests.render_case", json.dumps(dict(case="round_trip"))], {}, 900, 20)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(render_case.SPECS))
def test_render_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "RENDER_CASE_OK" in out, out[-3000:] + err[-3000:]


def test_round_trip_of_a_depth_image_through_the_map(emu_jobs, request):
    """Two frames of the room integrated, the MODEL's view from the second frame's own pose and intrinsics against that
    frame's input depth where both are valid: the median absolute difference stays below twice what was measured here
    (render_case.ROUND_TRIP_MEASURED_M), and below two voxels whatever was measured — more means the stepping rule is wrong."""
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "RENDER_CASE_OK" in out, out[-3000:] + err[-3000:]
