"""CPU tier of block removal.
1. the NumPy model (tests/remove_model.py) on its own: the float32 rule against a float64 evaluation on blocks chosen away from the
   threshold (and what the rule does AT a threshold f32 can represent), the removed sets, the slot arithmetic, the tile lists of the
   locality cases — the yardstick is validated before it judges anything, and the fields hold what the cases say they hold;
2. the DEVICE CODE on the host functional model (tools/emu) against the model and the fresh-context yardstick, byte for byte: one
   child process per case (tests/remove_case.py), started side by side like those of tests/test_emu_parity.py.
Part 1 needs no library and passes on its own.  What fails without the feature is part 2, tests/test_remove_gpu.py and
tests/test_remove_abi.py."""
import json
import sys

import numpy as np
import pytest

from tests import remove_case
from tests import remove_model as M
from tests import test_emu_parity as EP

VOXEL = remove_case.VOXEL


def _grid(n, lo):
    r = range(lo, lo + n)
    return np.array([(x, y, z) for x in r for y in r for z in r], np.int32)


@pytest.mark.parametrize("vps", [8, 16, 32])
def test_f32_rule_equals_f64_away_from_the_threshold(vps):
    rng = np.random.default_rng(vps)
    blocks = _grid(9, -4)
    checked = 0
    for _ in range(200):
        centre = rng.uniform(-2.0, 2.0, 3)
        radius = float(rng.uniform(0.0, 4.0))
        gap = np.abs(M.distance_f64(blocks, centre, VOXEL, vps) - float(np.float32(radius))).min()
        if gap <= 1e-3:
            continue
        far = M.assert_away_from_threshold(blocks, centre, radius, VOXEL, vps)   # (asserts f32 == f64 itself)
        checked += 1
        assert far.dtype == bool and len(far) == len(blocks)
    assert checked > 100


def test_rule_judges_the_origin_not_the_centre_and_is_strict():
    vps, bs = 16, np.float32(VOXEL) * np.float32(16)
    blocks = np.array([(1, 0, 0), (2, 0, 0), (-2, 0, 0), (0, 0, 0)], np.int32)
    # origins at 0.8, 1.6, -1.6 and 0 m along x; a block of 0.8 m whose ORIGIN is at 1.6 m has its centre at 2.0 m
    assert M.distant_f32(blocks, (0, 0, 0), 1.7, VOXEL, vps).tolist() == [False, False, False, False]
    assert M.distant_f32(blocks, (0, 0, 0), 1.5, VOXEL, vps).tolist() == [False, True, True, False]
    # strict: a block exactly at the radius stays (2 * bs is exact in f32, and so is its square against itself)
    r = float(np.float32(2) * bs)
    assert M.distant_f32(blocks, (0, 0, 0), r, VOXEL, vps).tolist() == [False, False, False, False]
    assert M.distant_f32(blocks, (0, 0, 0), float(np.nextafter(np.float32(r), np.float32(0))), VOXEL, vps).tolist() == [False, True, True, False]
    assert M.distant_f32(blocks, (0, 0, 0), 0.0, VOXEL, vps).tolist() == [True, True, True, False]


def test_every_operation_of_the_rule_is_f32():
    """A block whose f32 and f64 verdicts differ exists (that is why the cases stay away from the threshold): the f32 restatement finds it."""
    vps = 8
    blocks = _grid(21, -10)
    centre = (0.013, -0.007, 0.021)
    d = M.distance_f64(blocks, centre, VOXEL, vps)
    differ = 0
    for k in np.argsort(d)[10:400]:
        for r in (np.float32(d[k]), np.nextafter(np.float32(d[k]), np.float32(0)), np.nextafter(np.float32(d[k]), np.float32(9))):
            differ += int(M.distant_f32(blocks[k:k + 1], centre, float(r), VOXEL, vps)[0] != (d[k] > float(r)))
    assert differ > 0


def test_removed_sets_and_kept_rows():
    res = _grid(3, 0)
    listed = [(0, 0, 0), (5, 5, 5), (2, 2, 2), (0, 0, 0), (1, 0, 2)]
    got = M.removed_of_list(res, listed)
    assert got.tolist() == [[0, 0, 0], [1, 0, 2], [2, 2, 2]]
    vals = np.arange(len(res))
    kidx, kv = M.kept_of(res, got, vals)
    assert len(kidx) == len(res) - 3 == len(kv) and not ({(0, 0, 0), (1, 0, 2), (2, 2, 2)} & {tuple(r) for r in kidx.tolist()})
    assert (res[kv] == kidx).all()
    far = M.removed_of_distance(res, (0.0, 0.0, 0.0), 0.3, VOXEL, 8)       # block size 0.4 m: only the origin block is within 0.3 m
    assert len(far) == len(res) - 1 and (0, 0, 0) not in {tuple(r) for r in far.tolist()}
    far = M.removed_of_distance(res, (0.0, 0.0, 0.0), 0.5, VOXEL, 8)       # ... and its three face neighbours within 0.5 m
    assert len(far) == len(res) - 4 and not ({(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)} & {tuple(r) for r in far.tolist()})
    assert len(M.removed_of_list(res, [])) == 0 and M.removed_of_list(res, []).shape == (0, 3)


def test_slot_arithmetic():
    assert M.moves_needed([True] * 5) == (5, 0)
    assert M.moves_needed([False] * 5) == (0, 0)
    assert M.moves_needed([False, False, True, True, True]) == (3, 2)        # lowest slots leave: the two highest move down
    assert M.moves_needed([True, True, True, False, False]) == (3, 0)        # highest slots leave: no move
    assert M.moves_needed([True, False] * 4) == (4, 2)
    assert M.moves_needed([False, False, False, False, True, False, True]) == (2, 2)   # more holes than tail survivors
    rng = np.random.default_rng(0)
    for _ in range(50):
        keep = rng.random(40) < rng.random()
        nt2, moves = M.moves_needed(keep)
        assert moves == int((~keep[:nt2]).sum()) <= int((~keep).sum())       # as many survivors above as holes below


@pytest.mark.parametrize("vps", [8, 16])
def test_fields_hold_what_the_cases_are_chosen_for(vps):
    for field in (remove_case.box_field(vps), remove_case.sphere_field(vps), remove_case.two_clusters(vps)):
        idx = field[0]
        tiles = len(idx) * (vps // 8) ** 3
        assert 40 <= tiles <= 120 and len({tuple(r) for r in idx.tolist()}) == len(idx), tiles
    # the distance queries of the cases stay away from the threshold, and remove part of the field
    idx = remove_case.box_field(vps)[0]
    spec = remove_case.SPECS["distance_vps%d" % vps]
    n = [int(M.assert_away_from_threshold(idx, c, r, VOXEL, vps).sum()) for c, r in spec["queries"]]
    assert n[0] == 0 and all(0 < k < len(idx) for k in n[1:]), n


# ---- 2. the device code on the functional model: one child per case, started together by test_emu_parity's fixture ----
_LONG = ("integrate", "flags", "sliding", "errors", "esdf", "locality")
for _name, _spec in remove_case.SPECS.items():
    EP.JOBS["test_remove_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.remove_case", json.dumps(_spec)], {}, 900, 40 if _spec["case"] in _LONG else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(remove_case.SPECS))
def test_remove_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "REMOVE_CASE_OK" in out, out[-3000:] + err[-3000:]
