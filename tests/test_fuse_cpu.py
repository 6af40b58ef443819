"""CPU tier of submap fusion (ks_fuse_map).
1. the NumPy model (tests/fuse_model.py) on its own: a plane field fused into an empty map under 20 random poses reproduces the plane at
   the destination centres (a trilinear sample of a linear function is exact up to f32 rounding), the nearest corner is one of the eight
   and the one nearest to the point, the inverse pose undoes the pose — the yardstick is validated before it judges anything;
2. the DEVICE CODE on the host functional model (tools/emu) against the model, byte for byte: one child process per case
   (tests/fuse_case.py), started side by side like those of tests/test_emu_parity.py.
Part 1 needs no library and passes on its own.  What fails without the feature is part 2, tests/test_fuse_gpu.py and tests/test_fuse_abi.py."""
import json
import sys

import numpy as np
import pytest

from tests import fuse_case
from tests import fuse_model as M
from tests import test_emu_parity as EP

VOXEL = 0.05
F = np.float32
# |d_a - plane| at the destination centres.  The construction has no discretisation error; what remains is f32 rounding: of the stored
# distances (|d| <= 2.5 m: half an ulp is 1.2e-7 m), of the point (coordinates of 2 m through a rotation: a few ulps of 2.4e-7 m, times
# |n| = 1) and of the three interpolation steps.  The 20 poses below measure 7.4e-7 m at worst (printed by the test); the bound leaves
# a factor of 2.7.
PLANE_TOLERANCE = 2e-6


def _random_pose(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return np.concatenate([q, rng.uniform(-0.3, 0.3, 3)]).astype(F)


def _plane_blocks(n, o, vps=8, half=3):
    """d = n . x - o at the voxel centres of the blocks [-half, half)^3: coordinates within +-1.2 m."""
    from kimera_semantics_amd import binding as B
    r = range(-half, half)
    idx = np.array([(x, y, z) for x in r for y in r for z in r], np.int32)
    lin = np.arange(vps ** 3)
    local = np.stack([lin % vps, (lin // vps) % vps, lin // (vps * vps)], axis=1)
    centre = ((idx[:, None, :].astype(np.int64) * vps + local[None]).astype(np.float64) + 0.5) * float(F(VOXEL))
    t, s = np.zeros((len(idx), vps ** 3), B.TSDF_DTYPE), np.zeros((len(idx), vps ** 3), B.SEM_DTYPE)
    t["distance"] = (centre @ n - o).astype(F)
    t["weight"] = 1.0
    s["priors"] = M.PRIOR_INIT
    s["priors"][..., 4] = F(-0.1)                                     # (the fold recomputes the label from the priors)
    s["label"] = 4
    return idx, t, s


def _empty(vps=8):
    from kimera_semantics_amd import binding as B
    return np.zeros((0, 3), np.int32), np.zeros((0, vps ** 3), B.TSDF_DTYPE), np.zeros((0, vps ** 3), B.SEM_DTYPE)


def test_model_reproduces_a_plane_under_random_poses():
    from kimera_semantics_amd import synth
    rng = np.random.default_rng(11)
    worst = 0.0
    for k in range(20):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        o = float(rng.uniform(-0.4, 0.4))
        src = _plane_blocks(n, o)
        T = _random_pose(rng)
        R = M.fuse(_empty() + (8,), src + (8,), T, VOXEL, label_rgba=synth.default_label_colors())
        assert R.voxels_fused > 40 ** 3 // 2, R.voxels_fused            # most of the 48^3 box arrives
        # the plane at the destination centres: through the EXACT inverse of the pose the call reads (f64)
        w, v, t = M.pose64(T)
        j, l = np.nonzero(R.touched)
        vox = R.idx[j].astype(np.int64) * 8 + np.stack([l % 8, (l // 8) % 8, l // 64], axis=1)
        c = (vox.astype(np.float64) + 0.5) * float(F(VOXEL))
        p = np.stack(M._rotate64(w, [-v[0], -v[1], -v[2]], [c[:, a] - t[a] for a in range(3)]), axis=1)
        err = np.abs(R.tsdf["distance"][j, l].astype(np.float64) - (p @ n - o)).max()
        print("pose %d: %d voxels, max |d_a - plane| = %.3g m" % (k, len(j), err))
        worst = max(worst, err)
        assert err <= PLANE_TOLERANCE, (k, err)
        assert (R.tsdf["weight"][j, l] == 1.0).all() and (R.sem["label"][j, l] == 4).all()
        assert (R.tsdf["weight"][~R.touched] == 0).all()
    print("worst of 20 poses: %.3g m" % worst)


def test_nearest_corner_is_one_of_the_eight_and_the_nearest():
    rng = np.random.default_rng(5)
    src = _plane_blocks(np.array([0.0, 0.0, 1.0]), 0.0, half=2)
    S = M.Dense(*src, 8)
    nz, ny, nx = S.shape
    p = rng.uniform(-0.7, 0.7, (20000, 3)).astype(F)                       # (the field covers [-0.8 m, 0.8 m): every corner is inside)
    p[:2000] = (np.round(p[:2000] / F(VOXEL)) * F(VOXEL)).astype(F)          # points on voxel faces and centres: f = 0, 0.5 and their neighbours
    p[2000:4000] = ((np.round(p[2000:4000] / F(VOXEL)) + F(0.5)) * F(VOXEL)).astype(F)
    inv = F(1.0 / np.float64(F(VOXEL)))
    ok, d_a, w_a, near, (iv, nk) = M.sample(S, p, inv, 1e-4)
    assert ok.all()
    l = iv - S.org
    lowest = (l[:, 2] * ny + l[:, 1]) * nx + l[:, 0]
    offs = np.array([(k & 1) + nx * (((k >> 1) & 1) + ny * (k >> 2)) for k in range(8)])
    assert ((near[:, None] - lowest[:, None]) == offs[None, :]).any(axis=1).all()
    assert (near - lowest == offs[nk]).all()
    # ... and the voxel whose centre is nearest to the point (a tie goes up): within half a voxel on every axis
    g = p.astype(np.float64) * float(inv) - 0.5
    corner = iv + np.stack([nk & 1, (nk >> 1) & 1, nk >> 2], axis=1)
    assert (np.abs(g - corner) <= 0.5 + 1e-4).all()
    assert len(np.unique(nk)) == 8


def test_inverse_pose_undoes_the_pose():
    rng = np.random.default_rng(7)
    x = rng.uniform(-1.2, 1.2, (1000, 3)).astype(F)
    for _ in range(20):
        T = _random_pose(rng)
        Ti = M.inverse_pose(T)
        assert Ti.dtype == F and abs(float(np.linalg.norm(Ti[:4].astype(np.float64))) - 1.0) < 1e-7
        back = M.transform(Ti, M.transform(T, x))
        assert np.abs(back - x).max() < 2e-6, np.abs(back - x).max()          # a few ulps of coordinates of 2 m
    assert M.inverse_pose([1, 0, 0, 0, 0, 0, 0]).tolist() == [1, 0, 0, 0, 0, 0, 0]
    assert M.inverse_pose([2, 0, 0, 0, 0.5, -1, 2]).tolist() == [1, 0, 0, 0, -0.5, 1, -2]   # normalised, translation negated


def test_fields_and_poses_hold_what_the_cases_are_chosen_for():
    for vps in (8, 16):
        assert len(fuse_case.sphere_field(vps)[0]) * (vps // 8) ** 3 == 64
    idx, t, s = fuse_case.holes_field()
    assert 30 <= len(idx) < 64 and 0.05 < (t["weight"] == 0).mean() < 0.2
    for name, T in fuse_case.POSES.items():
        assert T.dtype == F and abs(float(np.linalg.norm(T[:4].astype(np.float64))) - 1.0) < 1e-6, name
    assert set(fuse_case.SPECS) >= {"identity_empty", "shift_voxels", "shift_half", "yaw90", "generic_empty", "generic_vps", "overlap_color", "overlap_prob",
                                    "holes", "chunked", "upload_order", "in_flight", "products", "syncs", "pool_growth", "out_of_range", "empty_source"}


# ---- 2. the device code on the functional model: one child per case, started together by test_emu_parity's fixture ----
for _name, _spec in fuse_case.SPECS.items():
    EP.JOBS["test_fuse_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.fuse_case", json.dumps(_spec)], {}, 900, 60 if _spec["case"] == "in_flight" else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(fuse_case.SPECS))
def test_fuse_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "FUSE_CASE_OK" in out, out[-3000:] + err[-3000:]
