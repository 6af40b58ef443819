"""CPU tier of the rooms (DESIGN.md, section "Rooms").
1. the NumPy model (tests/rooms_model.py) on its own, before it judges anything: its core components against scipy.ndimage.label with
   the full 3 x 3 x 3 structure, its costs and rooms against scipy.sparse.csgraph.dijkstra run per room (the minimum taken with ties
   to the smaller index), its links against a plain loop over the voxels, the closed form of the two rooms, and what the random
   field's seed is chosen for.  The stores are made by the ESDF model (rooms_case.model_store): no library is needed;
2. the DEVICE CODE on the host functional model (tools/emu) against the model, byte for byte: one child process per case
   (tests/rooms_case.py), started side by side like those of tests/test_emu_parity.py.
What fails without the feature is part 2, tests/test_rooms_abi.py and tests/test_rooms_gpu.py."""
import json
import sys

import numpy as np
import pytest

from tests import nav_model as N
from tests import rooms_case as C
from tests import rooms_model as M
from tests import test_emu_parity as EP

CFG = dict(free_distance_m=C.SMALL, core_distance_m=0.1)


@pytest.fixture(scope="module")
def random_models():
    """vps -> (store, model with min_core_voxels 1, model with 8) of the random field: computed once, never changed."""
    out = {}
    for vps in (8, 16):
        store = C.model_store(C.random_voxels(), vps)
        out[vps] = (store, M.rooms(store, min_core_voxels=1, vps=vps, **CFG), M.rooms(store, min_core_voxels=8, vps=vps, **CFG))
    return out


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vps", [8, 16])
def test_model_components_equal_scipy_label(random_models, vps):
    from scipy import ndimage
    store, m, _ = random_models[vps]
    with np.errstate(invalid="ignore"):
        core = ((store.flags & 1) != 0) & (store.dist >= np.float32(0.1))
    assert (core == m.core).all() and core.sum() > 1000
    got, n = ndimage.label(core, structure=np.ones((3, 3, 3), int))
    assert n == m.stats["components"] == m.stats["rooms"]
    flat = np.arange(core.size).reshape(core.shape)

    def canonical(comp):   # per voxel the smallest flat index of its component: the partition, whatever the numbering
        low = np.full(n + 1, core.size, np.int64)
        np.minimum.at(low, comp[core], flat[core])
        return np.where(core, low[comp], -1)

    assert (canonical(m.components) == canonical(got - 1)).all()
    assert sorted(np.bincount(got[core])[1:]) == sorted(m.records["n_core_voxels"].tolist())
    words = M.O.pack_coord3(m.records["first_voxel"])
    assert (words[1:] > words[:-1]).all()


@pytest.mark.parametrize("vps", [8, 16])
def test_model_growth_equals_dijkstra_per_room(random_models, vps):
    """cost and room of every free voxel: scipy's Dijkstra from the cores of one room at a time, the minimum over the rooms with ties
    to the smaller index."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    store, _, m = random_models[vps]
    free = m.free
    nz, ny, nx = free.shape
    node = np.full(free.shape, -1, np.int64)
    node[free] = np.arange(free.sum())
    pad = np.pad(node, 1, constant_values=-1)
    rows, cols, w = [], [], []
    for (dx, dy, dz), step in zip(N.OFFSETS, N.STEP):
        other = pad[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
        hit = (node >= 0) & (other >= 0)
        rows.append(node[hit]), cols.append(other[hit]), w.append(np.full(hit.sum(), step, np.float64))
    graph = coo_matrix((np.concatenate(w), (np.concatenate(rows), np.concatenate(cols))), shape=(free.sum(),) * 2).tocsr()
    n_rooms = len(m.records)
    best = np.full(free.sum(), np.inf)
    room = np.full(free.sum(), -1, np.int64)
    core_room = np.where(m.core & (m.ids != M.NONE) & (m.cost == 0), m.ids.astype(np.int64), -1)
    for r in range(n_rooms):
        d = dijkstra(graph, directed=False, indices=node[core_room == r], min_only=True)
        better = d < best                                # (strictly: a tie stays with the smaller index)
        best[better], room[better] = d[better], r
    reached = np.isfinite(best)
    want_cost = np.where(reached, best, float(N.UNREACHED)).astype(np.uint32)
    want_room = np.where(reached, room, int(M.NONE)).astype(np.uint32)
    assert n_rooms >= 20 and (m.cost[free] == want_cost).all() and (m.ids[free] == want_room).all()
    assert (m.cost[~free] == N.BLOCKED).all() and (m.ids[~free] == M.NONE).all() and (~reached).sum() == m.stats["voxels_unassigned"] >= 1
    # ties exist, so the rule that breaks them is exercised: a voxel equally far from the cores of two rooms
    ties = 0
    for r in range(min(n_rooms, 6)):
        d = dijkstra(graph, directed=False, indices=node[core_room == r], min_only=True)
        ties += int(((d == best) & (room != r)).sum())
    assert ties > 0


def test_model_links_equal_a_plain_loop(random_models):
    store, _, m = random_models[8]
    nz, ny, nx = m.ids.shape
    ids = m.ids.astype(np.int64)
    bits = np.ascontiguousarray(store.dist, np.float32).view(np.uint32)
    links = {}
    for z, y, x in zip(*np.nonzero(m.ids != M.NONE)):
        r, seen = ids[z, y, x], set()
        for dx, dy, dz in N.OFFSETS:
            a, b, c = z + dz, y + dy, x + dx
            if 0 <= a < nz and 0 <= b < ny and 0 <= c < nx and ids[a, b, c] != int(M.NONE) and ids[a, b, c] != r:
                seen.add(int(ids[a, b, c]))
        for q in seen:
            v = (int(bits[z, y, x]), tuple(int(t) for t in (np.array([x, y, z]) + store.org)), int(r))
            links.setdefault((min(r, q), max(r, q)), []).append(v)
    assert sorted(links) == [(int(l["room_a"]), int(l["room_b"])) for l in m.links] and len(links) >= 10
    for l in m.links:
        contacts = links[(int(l["room_a"]), int(l["room_b"]))]
        top = max(c[0] for c in contacts)
        door = min(c for c in contacts if c[0] == top)
        assert (l["n_contacts"], l["clearance_bits"], tuple(l["door_voxel"]), l["door_room"]) == (len(contacts), top, door[1], door[2]), l
    assert m.stats["contacts"] == sum(len(v) for v in links.values())
    assert m.records["n_links"].tolist() == [sum(1 for k in links if i in k) for i in range(len(m.records))]


@pytest.mark.parametrize("vps", [8, 16])
def test_model_gives_the_closed_form_of_the_two_rooms(vps):
    store = C.model_store(C.two_rooms_voxels(), vps)
    d, _, _ = store.records(np.array([(-8, -2, -2)], np.int64))
    assert d[0].tobytes() == np.float32(C.CORE_EQUAL).tobytes() == np.float32(0.2).tobytes()
    m = M.rooms(store, free_distance_m=C.SMALL, core_distance_m=C.CORE_EQUAL, vps=vps)
    C.assert_two_rooms(m.records, m.links, m.stats)
    assert (m.at(np.array([(0, y, z) for y in (-1, 0) for z in (-1, 0)], np.int64)) == 0).all()        # the door: a cost tie, to room 0
    # one float32 above: 16 core voxels a room (tests/rooms_case.py, case_two_rooms, says why it is not 12); below 17 there is no room
    m = M.rooms(store, free_distance_m=C.SMALL, core_distance_m=C.CORE_ABOVE, min_core_voxels=13, vps=vps)
    assert M.by_first(m.records) == {(-7, -1, -1): (16, 1104), (4, -1, -1): (16, 1100)}
    planes = [(x, y, z) for x in (-7, -6, -5) for y in (-1, 0) for z in (-1, 0)]
    assert m.core[tuple((np.array(planes) - store.org).T[::-1])].all() and len(planes) == 12
    m = M.rooms(store, free_distance_m=C.SMALL, core_distance_m=C.CORE_ABOVE, min_core_voxels=17, vps=vps)
    assert len(m.records) == 0 and len(m.links) == 0 and m.stats["voxels_unassigned"] == m.stats["voxels_free"] == 2204
    assert (m.ids == M.NONE).all() and (m.cost[m.free] == N.UNREACHED).all()


def test_random_field_holds_what_its_seed_is_chosen_for(random_models):
    for vps in (8, 16):
        _, m1, m8 = random_models[vps]
        C.assert_random_is_what_its_seed_is_for(m1, m8)


def test_model_join_takes_the_smallest_cost_then_the_smallest_room():
    store = C.model_store(C.two_rooms_voxels(), 8)
    oid = np.full(store.shape, M.NONE, np.uint32)

    def put(voxels, i):
        for v in voxels:
            l = np.array(v) - store.org
            oid[l[2], l[1], l[0]] = i

    put([(-8, -2, -2), (-11, 0, 0)], 0)                  # a core of room 0: cost 0
    put([(1, -1, -1), (-1, -1, -1)], 1)                  # one voxel in each room at the same cost: the smaller room
    put([(3, -1, -1), (-1, 0, 0)], 2)                    # nearer to the cores of room 1
    put([(-12, 0, 0)], 3)                                # a wall voxel: not assigned
    m = M.rooms(store, (5, oid), free_distance_m=C.SMALL, core_distance_m=C.CORE_EQUAL, vps=8)
    at = lambda *voxels: tuple((np.array(voxels) - store.org).T[::-1])
    assert m.dist[at((1, -1, -1), (-1, -1, -1), (3, -1, -1), (-1, 0, 0))].tolist() == [30, 30, 10, 30]
    assert m.ids[at((1, -1, -1), (-1, -1, -1), (3, -1, -1), (-1, 0, 0))].tolist() == [1, 0, 1, 0]
    assert m.room_of_object.tolist() == [0, 0, 1, int(M.NONE), int(M.NONE)] and m.records["n_objects"].tolist() == [2, 1]
    assert m.stats["objects_seen"] == 5 and m.stats["objects_joined"] == 3


# ---- 2. the device code on the functional model: one child per case, started together by test_emu_parity's fixture ----
for _name, _spec in C.SPECS.items():
    EP.JOBS["test_rooms_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.rooms_case", json.dumps(_spec)], {}, 900, 40 if _spec["case"] in ("lifetime", "errors", "reads_only") else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(C.SPECS))
def test_rooms_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "ROOMS_CASE_OK" in out, out[-3000:] + err[-3000:]
