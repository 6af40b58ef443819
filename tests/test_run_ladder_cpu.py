"""CPU tier of the voxel update at the run-length hand-overs between its kernels (csrc/ks_k_apply.h; tests/run_ladder_case.py).
1. the preconditions on their own, no library involved (the oracle's ray caster and grid rule): every frame of the full ladder holds ONE
   run of exactly its length in the sensor's voxel and no other as long, the `merged` sites their bundles, the bundle hand-over its
   points per end voxel, the batches their combined lengths, the single tile its one tile — a geometry that stops holding its edge
   fails here, without a GPU;
2. the DEVICE CODE on the host functional model (tools/emu) against the oracle: one child process per spec, started side by side like
   those of tests/test_emu_parity.py — a sub-ladder (31, 32, 33, 34, 256, 257, 1024, 1025, then 32 / 33 again on visited voxels)
   per route, and the whole ladder twice for the integer sums (1/z^2 weights) and for k_apply_runs with blended colours."""
import json
import sys

import numpy as np
import pytest

from tests import run_ladder_case as R
from tests import test_emu_parity as EP


def _quiet(_):
    pass


@pytest.mark.parametrize("method", [0, 1])
def test_every_frame_of_the_ladder_holds_one_run_of_its_length(method):
    sp = R.ladder(method=method)
    assert sp["lengths"] == (R.MERGED_LADDER if method else R.LADDER) and sp["second"] == sp["lengths"]
    assert R.ladder_precondition(sp, _quiet) == sp["lengths"]
    # the frames are at least 2 m apart: shell + truncation = 0.8 m, no voxel shared
    pos = np.array([R.position(k) for k in range(len(sp["lengths"]))])
    d = np.linalg.norm(pos[:, None] - pos[None], axis=2) + 10 * np.eye(len(pos))
    assert d.min() >= 2.0


def test_mixed_sites_hold_bundles_of_two_with_different_labels():
    sp = R.ladder(method=1, lengths=[32, 33, 257, 1025], mixed=True)
    R.ladder_precondition(sp, _quiet)
    xyz, labels, n = R.sites_cloud(33, R.position(1), mixed=True)
    ends = R.voxel_of(xyz + np.asarray(R.position(1), R.F))
    _, inverse, counts = np.unique(ends, axis=0, return_inverse=True, return_counts=True)
    assert n == 33 and sorted(set(counts.tolist())) == [1, 2] and (counts == 2).sum() == 8
    for v in np.nonzero(counts == 2)[0]:
        assert len(set(labels[inverse.ravel() == v].tolist())) == 2


def test_a_cloud_that_does_not_hold_its_length_is_refused():
    xyz, _ = R.shell_cloud(33)
    cells = R.ray_cells(R.CENTRE, xyz, False)
    R.check_run(33, R.CENTRE, cells, "run of 33", _quiet)
    assert R.rays_through(R.CENTRE, xyz, [0, 0, 0], False).all()    # (tests/xl_case.py's reading of the same ray caster)
    with pytest.raises(AssertionError, match="precondition"):
        R.check_run(32, R.CENTRE, cells, "run of 32", _quiet)
    with pytest.raises(AssertionError, match="precondition"):       # two shells from one position: the neighbours' runs reach the length asked for
        R.check_run(33, R.CENTRE, cells + cells[:20] * 3, "run of 33", _quiet)


def test_bundle_hand_over_cloud_holds_its_points_per_end_voxel():
    for permute in (False, True):
        xyz, labels = R.bundle_cloud(permute)
        assert len(xyz) == sum(R.BUNDLE_SIZES) and labels.min() >= 1 and labels.max() <= 19
    assert {31, 32, 33, 34} <= set(R.BUNDLE_SIZES)
    assert sorted(R.bundle_cloud(True)[0].tolist()) == sorted(R.bundle_cloud(False)[0].tolist())


@pytest.mark.parametrize("pipeline", [8, 16])
def test_batches_hold_their_combined_lengths(pipeline):
    nb, frames = R.batch_precondition(dict(pipeline=pipeline), _quiet)
    assert nb == pipeline // 2 and len(frames) == 4 * nb
    assert [sum(s) for s in R.BATCH_SUMS[nb]] == R.BATCH_TARGETS == [32, 33, 1024, 1025]


def test_single_tile_frames_stay_inside_the_tile_and_reach_past_33():
    frames = R.single_tile_precondition(dict(lengths=R.SINGLE_TILE), _quiet)
    assert [n for n, _, _ in frames] == R.SINGLE_TILE and max(R.SINGLE_TILE) == 129
    (n, xyz, cells), = R.single_tile_precondition(dict(head_at=1023), _quiet)
    assert n > 32 and sum(len(c) for c in cells) - n == 1023        # the sensor voxel's run begins on the last pair of a tile of 1024
    for n, xyz, cells in R.single_tile_precondition(dict(lengths=R.WINDOW_EDGE, head_mod=[64, 63]), _quiet):
        assert (sum(len(c) for c in cells) - n) % 64 == 63          # ... on the last lane of a window of 64


def test_specs_cover_every_route_mode_and_weight():
    gpu = R.gpu_specs()
    for route in R.ROUTES:
        for cm in (0, 1):
            for cw in (0, 1):
                assert "ladder-fast-%s-cm%d-cw%d" % (route, cm, cw) in gpu
    assert {"ladder-fast-default-cm1-cw1-pipeline2", "ladder-fast-lanes-cm1-cw1-pipeline2"} <= set(gpu)
    for name, sp in list(gpu.items()) + list(R.emu_specs().items()):
        assert json.loads(json.dumps(sp)) == sp, name
        if sp["kind"] == "ladder" and not sp["method"]:
            assert len(sp["lengths"]) + len(sp["second"]) <= 72 and max(sp["lengths"]) <= 2049


# ---- 2. the device code on the functional model: one child per spec, started together by test_emu_parity's fixture ----
EMU = R.emu_specs()
for _name, _spec in EMU.items():
    EP.JOBS["test_run_lengths_on_the_functional_model_equal_oracle[%s]" % _name] = (
        [sys.executable, "-m", "tests.run_ladder_case", json.dumps(_spec)], {}, 900, 30 if len(_spec.get("lengths", ())) > 10 else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", list(EMU))
def test_run_lengths_on_the_functional_model_equal_oracle(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    print(out[-4000:])
    assert rc == 0 and "RUN_LADDER_OK" in out, out[-3000:] + err[-3000:]
