"""CPU tier of the navigation field (DESIGN.md, section "Navigation field").
1. the NumPy model (tests/nav_model.py) on its own, before it judges anything: it equals scipy.sparse.csgraph.dijkstra on the
   explicit 26-neighbour graph of random fields; in an all-traversable box the cost is the closed form 10 a + 4 b + 3 c; along every
   model path consecutive waypoints are adjacent and the step costs sum to the start's cost; the hand-built fields hold what
   their cases are chosen for;
2. the DEVICE CODE on the host functional model (tools/emu) against the model, byte for byte: one child process per case
   (tests/nav_case.py), started side by side like those of tests/test_emu_parity.py.
Part 1 needs no library.  What fails without the feature is part 2, tests/test_nav_gpu.py and tests/test_nav_abi.py."""
import json
import sys

import numpy as np
import pytest

from tests import esdf_read_model as E
from tests import nav_case
from tests import nav_model as M
from tests import test_emu_parity as EP

F = np.float32
VS = nav_case.VOXEL
RECORD = np.dtype([("distance", "<f4"), ("flags", "u1"), ("label", "u1"), ("pad", "u1", (2,))])   # the layout of ks_esdf_download_blocks


def store_of_voxels(vox, vps, distance=0.4):
    """The stored ESDF of a field of nav_case: the free voxels observed at `distance`, default records elsewhere."""
    at = sorted({tuple(int(c) // vps for c in p) for p in vox})
    row = {b: j for j, b in enumerate(at)}
    rec = np.zeros((len(at), vps ** 3), RECORD)
    rec["label"] = 255
    for x, y, z in vox:
        j, l = row[(x // vps, y // vps, z // vps)], (x % vps) + vps * ((y % vps) + vps * (z % vps))
        rec["distance"][j, l], rec["flags"][j, l] = distance, 1
    return E.Store(np.array(at, np.int32).reshape(-1, 3), rec, vps)


def centres(vox):
    return ((np.asarray(vox, np.float64).reshape(-1, 3) + 0.5) * VS).astype(F)


def components(vox):
    from scipy import ndimage
    v = np.asarray(vox, np.int64)
    lo = v.min(axis=0)
    dense = np.zeros(tuple(v.max(axis=0) - lo + 1), bool)
    dense[tuple((v - lo).T)] = True
    return ndimage.label(dense, structure=np.ones((3, 3, 3), int))[1]


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vps,p,cap", [(8, 0.12, 0), (16, 0.12, 0), (8, 0.3, 0), (16, 0.3, 37)])
def test_model_equals_scipy_dijkstra_on_the_explicit_graph(vps, p, cap):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    vox = nav_case.random_voxels(seed=21 + vps, p=p)
    store = store_of_voxels(vox, vps)
    rng = np.random.default_rng(vps)
    goals = centres([vox[i] for i in rng.choice(len(vox), 5, replace=False)])
    fld = M.field(store, goals, VS, radius_m=0.3, max_cost=cap)
    number = {v: i for i, v in enumerate(vox)}
    rows, cols, w = [], [], []
    for v, i in number.items():
        for o, step in zip(M.OFFSETS, M.STEP):
            j = number.get((v[0] + int(o[0]), v[1] + int(o[1]), v[2] + int(o[2])))
            if j is not None:
                rows.append(i), cols.append(j), w.append(int(step))
    graph = coo_matrix((w, (rows, cols)), shape=(len(vox), len(vox))).tocsr()
    sources = [number[tuple(int(c) for c in g)] for g in M.voxel_of(goals, VS)[0]]
    d = dijkstra(graph, directed=True, indices=sources, min_only=True)
    limit = cap if cap else M.MAX_COST
    want = np.where(np.isfinite(d) & (d <= limit), d, M.UNREACHED).astype(np.uint32)
    got = fld.at(np.array(vox))
    assert (got == want).all(), np.argwhere(got != want)[:5]
    assert (want == M.UNREACHED).any() and (want <= M.MAX_COST).sum() > 5
    assert fld.stats == dict(voxels_traversable=len(vox), voxels_reached=int((want <= M.MAX_COST).sum()), goals_used=5, goals_blocked=0,
                             largest_cost=int(want[want <= M.MAX_COST].max()))
    # every other voxel of the blocks is blocked
    assert (fld.cost == M.BLOCKED).sum() == fld.cost.size - len(vox)


@pytest.mark.parametrize("vps", [8, 16])
def test_model_in_an_open_box_is_the_closed_form(vps):
    vox = nav_case.open_box_voxels()
    fld = M.field(store_of_voxels(vox, vps), centres([nav_case.OPEN_BOX_GOAL]), VS)
    d = np.sort(np.abs(np.array(vox) - np.array(nav_case.OPEN_BOX_GOAL)), axis=1)
    assert (fld.at(np.array(vox)) == 10 * d[:, 2] + 4 * d[:, 1] + 3 * d[:, 0]).all()


def test_model_paths_step_between_adjacent_voxels_and_sum_to_the_cost():
    vox = nav_case.random_voxels()
    fld = M.field(store_of_voxels(vox, 8), nav_case.random_goals(vox), VS)
    starts = nav_case.path_starts()
    out = M.paths(fld, starts, 600)
    assert set(np.unique(out["status"])) == {M.REACHED, M.UNREACHABLE, M.PATH_BLOCKED}
    checked = 0
    for k in np.nonzero(out["status"] == M.REACHED)[0]:
        ijk = M.voxel_of(out["waypoints"][k, :out["n_waypoints"][k]], VS)[0]
        steps = np.abs(np.diff(ijk, axis=0))
        assert (steps.max(axis=1) == 1).all() if len(steps) else True
        assert sum(M.COST[int(s.sum())] for s in steps) == out["cost"][k] and fld.at(ijk[-1:])[0] == 0
        assert (M.voxel_of(starts[k:k + 1], VS)[0][0] == ijk[0]).all()
        checked += 1
    assert checked > 50
    short = M.paths(fld, starts, 7)
    assert (short["status"] == M.TRUNCATED).sum() > 0 and (short["n_waypoints"][short["status"] == M.TRUNCATED] == 7).all()
    assert (short["waypoints"][short["status"] == M.TRUNCATED] == out["waypoints"][short["status"] == M.TRUNCATED][:, :7]).all()


def test_fields_hold_what_the_cases_are_chosen_for():
    # seams: four pairs, each on its own, at exactly the step costs
    vox = nav_case.seams_voxels()
    assert components(vox) == 4
    fld = M.field(store_of_voxels(vox, 8), centres([a for a, _, _ in nav_case.SEAM_PAIRS]), VS)
    for a, b, cost in nav_case.SEAM_PAIRS:
        assert fld.at([a])[0] == 0 and fld.at([b])[0] == cost
        assert tuple(np.array(a) >> 3) != tuple(np.array(b) >> 3) and int(np.abs(np.array(a) - np.array(b)).sum()) == {10: 1, 14: 2, 17: 3}[cost]
    assert tuple((np.array(nav_case.SEAM_PAIRS[2][1]) >> 3) - (np.array(nav_case.SEAM_PAIRS[2][0]) >> 3)) == (-1, 1, 0)
    # serpentine: one corridor; the way back winds at least 100 steps inside one tile and enters one tile at least four times
    path = nav_case.serpentine_path()
    assert components(path) == 1 and len({tuple(np.array(p) >> 3) for p in path}) >= 16
    fld = M.field(store_of_voxels(path, 8), centres(path[:1]), VS)
    assert fld.stats["voxels_reached"] == len(path) and fld.stats["largest_cost"] == fld.at(path[-1:])[0] > 3000
    walk = M.paths(fld, centres(path[-1:]), 1024)
    assert walk["status"][0] == M.REACHED
    tiles = [tuple(t) for t in M.voxel_of(walk["waypoints"][0, :walk["n_waypoints"][0]], VS)[0] >> 3]
    runs = [t for k, t in enumerate(tiles) if k == 0 or tiles[k - 1] != t]      # the tiles in the order the walk enters them
    assert max(runs.count(t) for t in set(runs)) >= 4, runs
    assert tiles.count((0, 0, 0)) >= 100
    two = M.field(store_of_voxels(path, 8), centres([path[0], path[-1]]), VS)
    assert abs(two.stats["largest_cost"] - fld.stats["largest_cost"] // 2) <= 20
    # random: at least three components, reached and unreached voxels, five goals that do not count
    vox = nav_case.random_voxels()
    assert components(vox) >= 3
    goals = nav_case.random_goals(vox)
    fld = M.field(store_of_voxels(vox, 8), goals, VS)
    assert fld.stats["goals_blocked"] == nav_case.RANDOM_GOALS_BLOCKED and fld.stats["goals_used"] == len(goals) - nav_case.RANDOM_GOALS_BLOCKED
    assert 500 < fld.stats["voxels_reached"] < fld.stats["voxels_traversable"] - 100, fld.stats
    seams = (np.array(vox) >> 3)
    assert len({tuple(t) for t in seams}) == 64


# ---- 2. the device code on the functional model: one child per case, started together by test_emu_parity's fixture ----
for _name, (_spec, _env) in nav_case.SPECS.items():
    EP.JOBS["test_nav_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.nav_case", json.dumps(_spec)], dict(_env), 900, 40 if _spec["case"] in ("lifetime", "errors", "reads_only") else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(nav_case.SPECS))
def test_nav_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "NAV_CASE_OK" in out, out[-3000:] + err[-3000:]
