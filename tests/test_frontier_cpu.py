"""CPU tier of the exploration frontiers (DESIGN.md, section "Exploration frontiers").
1. the NumPy model (tests/frontier_model.py) on its own, before it judges anything: on the random field its frontier mask and its
   components equal an independent computation with scipy.ndimage (binary shifts, label with the full 3 x 3 x 3 structure); the cube
   and the room give their closed forms; the faces field gives its hand-written table, the voxel with a NaN distance included; the
   random field holds what its seed is chosen for.  The stores are made by hand (frontier_case.hand_store): no library is needed;
2. the DEVICE CODE on the host functional model (tools/emu) against the model, byte for byte: one child process per case
   (tests/frontier_case.py), started side by side like those of tests/test_emu_parity.py.
What fails without the feature is part 2 and tests/test_frontier_gpu.py."""
import json
import sys

import numpy as np
import pytest

from tests import frontier_case as C
from tests import frontier_model as M
from tests import nav_case
from tests import nav_model as N
from tests import test_emu_parity as EP


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vps", [8, 16])
def test_model_equals_scipy_on_the_random_field(vps):
    from scipy import ndimage
    store = C.hand_store(C.random_voxels(), vps)
    m = M.frontiers(store, radius_m=C.SMALL, min_voxels=1, vps=vps)
    observed = np.pad((store.flags & 1) != 0, 1)
    free = np.pad(store.dist >= np.float32(C.SMALL), 1) & observed
    cross = ndimage.generate_binary_structure(3, 1)
    want = (free & ndimage.binary_dilation(~observed, structure=cross))[1:-1, 1:-1, 1:-1]
    assert (m.part == want).all() and want.sum() > 1000
    faces = ndimage.convolve((~observed).astype(np.int64), cross.astype(np.int64), mode="constant", cval=1)[1:-1, 1:-1, 1:-1]
    assert m.stats["unknown_faces"] == int(faces[want].sum())
    got, n = ndimage.label(want, structure=np.ones((3, 3, 3), int))
    assert n == m.stats["components"] == m.stats["frontiers"]
    flat = np.arange(want.size).reshape(want.shape)

    def canonical(comp):   # per voxel the smallest flat index of its component: the partition, whatever the numbering
        low = np.full(n + 1, want.size, np.int64)
        np.minimum.at(low, comp[want], flat[want])
        return np.where(want, low[comp], -1)

    assert (canonical(m.components) == canonical(got - 1)).all()
    assert sorted(np.bincount(got[want])[1:]) == sorted(m.records["n_voxels"].tolist())
    words = M.O.pack_coord3(m.records["first_voxel"])
    assert (words[1:] > words[:-1]).all()


@pytest.mark.parametrize("vps", [8, 16])
def test_model_gives_the_closed_forms_of_cube_and_room(vps):
    m = M.frontiers(C.hand_store(C.cube_voxels(), vps), radius_m=C.SMALL, vps=vps)
    assert M.by_first(m.records) == {(-5, -5, -5): (488, 600)} and m.stats["components"] == 1 and m.stats["voxels_traversable"] == 1000
    r = m.records[0]
    assert tuple(r["bb_min"]) == (-5, -5, -5) and tuple(r["bb_max"]) == (4, 4, 4) and tuple(r["sum"]) == (-244, -244, -244)
    assert r["nav_cost"] == N.UNREACHED and tuple(r["nav_voxel"]) == (-5, -5, -5) and (m.ids != M.NONE).sum() == 488
    m = M.frontiers(C.hand_store(C.room_voxels(False), vps), radius_m=C.SMALL, min_voxels=1, vps=vps)
    assert len(m.records) == 0 and m.stats["components"] == 0 and (m.ids == M.NONE).all()
    m = M.frontiers(C.hand_store(C.room_voxels(True), vps), radius_m=C.SMALL, min_voxels=1, vps=vps)
    assert M.by_first(m.records) == {(5, -1, -1): (4, 4)} and m.stats["components"] == 1
    # bounds: two patches; a voxel outside them still is the unobserved neighbour it is
    store = C.hand_store(C.cube_voxels(), vps)
    m = M.frontiers(store, radius_m=C.SMALL, use_bounds=1, bounds_min=(-5, -4, -4), bounds_max=(4, 3, 3), vps=vps)
    assert M.by_first(m.records) == {(-5, -4, -4): (64, 64), (4, -4, -4): (64, 64)}
    m = M.frontiers(store, radius_m=C.SMALL, use_bounds=1, bounds_min=(-5, -5, -5), bounds_max=(4, 4, 4), vps=vps)
    assert M.by_first(m.records) == {(-5, -5, -5): (488, 600)}


@pytest.mark.parametrize("vps", [8, 16])
def test_model_gives_the_hand_table_of_the_faces_field(vps):
    vox, resident = C.faces_field(nan=True)
    store = C.hand_store(vox, vps, resident)
    nan_at = np.array([(48 * 25 + 19, 19, 19)], np.int64)
    d, flags, _ = store.records(nan_at)
    assert np.isnan(d[0]) and flags[0] == 1
    for radius, table in ((C.SMALL, C.FACES_EXPECTED), (C.RADIUS_EQUAL, C.FACES_EXPECTED), (C.RADIUS_ABOVE, C.FACES_EXPECTED_ABOVE)):
        m = M.frontiers(store, radius_m=radius, min_voxels=1, vps=vps)
        assert M.by_first(m.records) == table, (radius, M.by_first(m.records))
        assert m.at(nan_at)[0] == M.NONE                            # observed, and a NaN is not traversable
    # the same field without the NaN voxel (what an upload can make) gives the same table
    vox, resident = C.faces_field()
    assert M.by_first(M.frontiers(C.hand_store(vox, vps, resident), radius_m=C.SMALL, min_voxels=1, vps=vps).records) == C.FACES_EXPECTED
    # each neighbour block is what its item says: absent, resident, observed
    blocks = {tuple(int(v) for v in b) for b in (np.array(sorted(set(vox) | set(resident))) // vps)}
    assert (15 // vps, 19 // vps, 19 // vps) not in blocks and (15, 19, 19) not in vox
    assert (63 // vps, 19 // vps, 19 // vps) in blocks and (63, 19, 19) not in vox and vox[(111, 19, 19)] == C.WALL


def test_random_field_holds_what_its_seed_is_chosen_for():
    for vps in (8, 16, 32):
        m = M.frontiers(C.hand_store(C.random_voxels(), vps), radius_m=C.SMALL, min_voxels=1, vps=vps)
        n = m.records["n_voxels"]
        assert m.stats["components"] >= 100 and (n == 1).sum() >= 5 and n.max() >= 300 and C.crossing_a_seam(m.records) >= 20
        m8 = M.frontiers(C.hand_store(C.random_voxels(), vps), radius_m=C.SMALL, vps=vps)
        assert 0 < m8.stats["frontiers"] < m8.stats["components"] == m.stats["components"]


def test_model_join_takes_the_smallest_cost_then_the_smallest_voxel():
    from tests import test_nav_cpu
    vox = nav_case.open_box_voxels()
    store = test_nav_cpu.store_of_voxels(vox, 8)
    field = N.field(store, test_nav_cpu.centres([nav_case.OPEN_BOX_GOAL]), C.VOXEL)
    m = M.frontiers(store, field, radius_m=0.3)
    assert field.at([(-8, 5, 3)])[0] == field.at([(2, 15, 3)])[0] == 100
    r = m.records[0]
    assert len(m.records) == 1 and r["n_voxels"] == 24 ** 3 - 22 ** 3 and r["nav_cost"] == 100 and tuple(r["nav_voxel"]) == (-8, 5, 3)
    assert m.stats["nav_field_used"] == 1


# ---- 2. the device code on the functional model: one child per case, started together by test_emu_parity's fixture ----
for _name, _spec in C.SPECS.items():
    EP.JOBS["test_frontier_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.frontier_case", json.dumps(_spec)], {}, 900, 40 if _spec["case"] in ("lifetime", "errors", "reads_only", "integrated") else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(C.SPECS))
def test_frontier_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "FRONTIER_CASE_OK" in out, out[-3000:] + err[-3000:]
