"""CPU tier of "one map, four block sizes" (tests/block_size_case.py).
1. the fixture on its own: mesh_case.same_map(vps) is one voxel content at 8, 16, 32 and 64 voxels per side, every block of its
   box present, and holds what the readers need (a surface, two labels, unobserved voxels, a free pocket);
2. the DEVICE CODE on the host functional model (tools/emu): every reader of the map at 16, 32 and 64 against its own result at 8,
   which the same process checks against the NumPy models — one child process per block size, started side by side like those of
   tests/test_emu_parity.py;
3. the two integrator tests that take a block size (tests/test_parity_gpu.py), unchanged, at 64 voxels per side on the functional
   model: the merged single frame against the oracle, and the voxel-level sync (k_export_dirty's block and linear index)."""
import json
import sys

import numpy as np
import pytest

from tests import block_size_case, mesh_case
from tests import test_emu_parity as EP


def test_same_map_is_one_voxel_content_in_four_layouts():
    origin, t0, s0 = mesh_case.same_map_voxels()
    (x0, x1), (y0, y1), (z0, z1) = mesh_case.SAME_MAP_BOX
    assert tuple(origin) == (x0, y0, z0) and t0.shape == (z1 - z0, y1 - y0, x1 - x0)
    for vps in (8, 16, 32, 64):
        idx, t, s = mesh_case.same_map(vps)
        want = {(x, y, z) for x in range(x0 // vps, x1 // vps) for y in range(y0 // vps, y1 // vps) for z in range(z0 // vps, z1 // vps)}
        assert {tuple(int(v) for v in b) for b in idx} == want and len(idx) == len(want) == mesh_case.SAME_MAP_TILES * 512 // vps ** 3
        assert t.shape == s.shape == (len(idx), vps ** 3)
        # the host layout, restated: voxel l of block b is the global voxel b * vps + (l % vps, l / vps % vps, l / vps^2)
        rng = np.random.default_rng(vps)
        for j, l in zip(rng.integers(0, len(idx), 200), rng.integers(0, vps ** 3, 200)):
            gx, gy, gz = (int(idx[j][a]) * vps + (l // vps ** a) % vps for a in range(3))
            assert t[j, l].tobytes() == t0[gz - z0, gy - y0, gx - x0].tobytes() and s[j, l].tobytes() == s0[gz - z0, gy - y0, gx - x0].tobytes()
        assert mesh_case.from_blocks(idx[::-1], t[::-1], vps).tobytes() == t0.tobytes()


def test_same_map_holds_what_the_readers_need():
    _, t, s = mesh_case.same_map_voxels()
    unobserved = (t["weight"] == 0).mean()
    assert 0.07 < unobserved < 0.10          # 10 % of the voxels outside the pocket (a sixth of the box)
    assert (t["distance"] < 0).any() and set(np.unique(s["label"])) == {3, 7}
    # the surface crosses the seam x = 0 of every block size (column 64 of the box), and the seams y = 32, z = 32 of all but 64
    sign = t["distance"] < 0
    assert sign[:, :, 63].any() and sign[:, :, 64].any() and sign[31].any() and sign[32].any() and sign[:, 31].any() and sign[:, 32].any()
    (px0, px1), (py0, py1), (pz0, pz1) = mesh_case.SAME_MAP_POCKET
    pocket = t[pz0:pz1, py0:py1, px0 + 64:px1 + 64]
    assert (pocket["weight"] == 1).all() and (pocket["distance"] >= np.float32(0.1)).all()
    # the fixed polyline and the goal of the cost-to-go field lie in the pocket, more than the robot's radius from its walls
    wp, nw = block_size_case.polyline()
    lo = (np.array([px0, py0, pz0]) + 4) * mesh_case.VOXEL
    hi = (np.array([px1, py1, pz1]) - 4) * mesh_case.VOXEL
    for p in (wp[0], block_size_case.pocket_centre()):
        assert (p >= lo).all() and (p <= hi).all()
    assert nw[0] == wp.shape[1] > 10


for _name, _spec in block_size_case.SPECS.items():
    EP.JOBS["test_readers_on_the_host_do_not_depend_on_the_block_size[%s]" % _name] = (
        [sys.executable, "-m", "tests.block_size_case", json.dumps(_spec)], {}, 900, 25)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(block_size_case.SPECS))
def test_readers_on_the_host_do_not_depend_on_the_block_size(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "BLOCK_SIZE_CASE_OK" in out, out[-3000:] + err[-3000:]


EP.JOBS["test_integrator_cases_at_64_voxels_per_side_on_the_functional_model"] = (
    [sys.executable, "-m", "pytest", "tests/test_parity_gpu.py", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k",
     "test_merged_single_frame_exact and 64 or test_voxel_level_sync_rebuilds_the_map and 64"], {"KS_TESTS_ON_FUNCTIONAL_MODEL": "1"}, 1200, 70)


def test_integrator_cases_at_64_voxels_per_side_on_the_functional_model(emu_jobs, request):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "2 passed" in out and "skipped" not in out.splitlines()[-1], out[-3000:] + err[-2000:]
