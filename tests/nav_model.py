"""The yardstick of the navigation-field tests: a NumPy restatement of the contract (DESIGN.md, section "Navigation field"), written
from the contract and not from the kernels: the field is computed by Dijkstra's algorithm over cost levels, not by relaxation.

    field(store, goals, voxel_size, radius_m=0.3, max_cost=0)  -> Field    store: esdf_read_model.Store / store_of(integrator)
    Field.at(ijk) / .query(xyz) / .blocks(idx, vps) / .stats
    paths(field, starts, max_waypoints)                        -> dict(status, cost, n_waypoints, waypoints, stats)

A voxel outside the downloaded blocks reads as a default ESDF record (esdf_read_model), so it is not traversable and reads BLOCKED."""
import numpy as np

from tests import esdf_read_model as E

F = np.float32
BLOCKED, UNREACHED, MAX_COST = 0xffffffff, 0xfffffffe, 0xffffff00
COST = {1: 10, 2: 14, 3: 17}
# the 26 offsets in the order of the contract: o = 0..26, o != 13, (x, y, z) = (o % 3 - 1, (o / 3) % 3 - 1, o / 9 - 1)
OFFSETS = np.array([(o % 3 - 1, (o // 3) % 3 - 1, o // 9 - 1) for o in range(27) if o != 13], np.int64)
STEP = np.array([COST[int(np.abs(d).sum())] for d in OFFSETS], np.int64)
REACHED, UNREACHABLE, PATH_BLOCKED, TRUNCATED, INVALID = 0, 1, 2, 3, 4
STAT_KEYS = ("voxels_traversable", "voxels_reached", "goals_used", "goals_blocked", "largest_cost")
WAYPOINT_FILL = F(-7.0)          # what HipIntegrator.nav_paths leaves in the rows the library does not write
_INF = np.int64(1) << 40


def voxel_of(xyz, voxel_size):
    """(ijk int64 (n, 3), ok): the voxel ks_esdf_query takes for each point; ok is False for non-finite points and outside the packed range."""
    p = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.floor(p * E.inv_of(voxel_size) + E.EPS)
        ok = np.isfinite(p).all(axis=1) & (np.abs(g) < E.LIM).all(axis=1)
    assert g.dtype == F
    return np.where(ok[:, None], g, F(0)).astype(np.int64), ok


def traversable_of(store, radius_m):
    """Dense [z, y, x] bool: observed and distance >= radius (f32; False for a NaN)."""
    with np.errstate(invalid="ignore"):
        return ((store.flags & 1) != 0) & (store.dist >= F(radius_m))


class Field:
    def __init__(self, org, cost, stats, voxel_size):
        self.org, self.cost, self.stats, self.voxel_size = org, cost, stats, voxel_size   # cost: dense [z, y, x] uint32

    def at(self, ijk):
        l = np.asarray(ijk, np.int64).reshape(-1, 3) - self.org
        shape = np.array(self.cost.shape[::-1])
        ok = ((l >= 0) & (l < shape)).all(axis=1)
        l = np.clip(l, 0, shape - 1)
        return np.where(ok, self.cost[l[:, 2], l[:, 1], l[:, 0]], BLOCKED).astype(np.uint32)

    def query(self, xyz):
        ijk, ok = voxel_of(xyz, self.voxel_size)
        return np.where(ok, self.at(ijk), BLOCKED).astype(np.uint32)

    def blocks(self, indices, vps):
        idx = np.asarray(indices, np.int64).reshape(-1, 3)
        lin = np.arange(vps ** 3)
        local = np.stack([lin % vps, (lin // vps) % vps, lin // (vps * vps)], axis=1)
        return self.at((idx[:, None, :] * vps + local[None]).reshape(-1, 3)).reshape(len(idx), vps ** 3)


def field(store, goals, voxel_size, radius_m=0.3, max_cost=0):
    cap = int(max_cost) if max_cost else MAX_COST
    trav = traversable_of(store, radius_m)
    nz, ny, nx = trav.shape
    # a border of one blocked voxel: a neighbour's flat index never wraps
    pad = np.zeros((nz + 2, ny + 2, nx + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = trav
    sy, sz = nx + 2, (nx + 2) * (ny + 2)
    free = pad.reshape(-1)
    flat_off = OFFSETS[:, 0] + sy * OFFSETS[:, 1] + sz * OFFSETS[:, 2]
    dist = np.full(free.size, _INF, np.int64)
    g, ok = voxel_of(goals, voxel_size)
    l = g - store.org
    ok &= ((l >= 0) & (l < np.array([nx, ny, nz]))).all(axis=1)
    gi = np.where(ok, (l[:, 0] + 1) + sy * (l[:, 1] + 1) + sz * (l[:, 2] + 1), 0)
    ok &= free[gi]
    seeds = np.unique(gi[ok])
    dist[seeds] = 0
    # Dijkstra by cost levels: every node with the smallest unsettled cost c is final; its neighbours take c + w if that is lower
    import heapq
    levels, buckets = [0] if len(seeds) else [], {0: [seeds]}
    while levels:
        c = heapq.heappop(levels)
        nodes = np.unique(np.concatenate(buckets.pop(c)))
        nodes = nodes[dist[nodes] == c]
        if len(nodes) == 0:
            continue
        nb = nodes[:, None] + flat_off[None, :]
        cand = np.broadcast_to(c + STEP[None, :], nb.shape)
        better = free[nb] & (cand < dist[nb]) & (cand <= cap)
        nbs, cs = nb[better], cand[better]
        np.minimum.at(dist, nbs, cs)
        for value in np.unique(cs):
            if value not in buckets:
                buckets[value] = []
                heapq.heappush(levels, int(value))
            buckets[value].append(nbs[cs == value])
    d = dist.reshape(pad.shape)[1:-1, 1:-1, 1:-1]
    reached = d < _INF
    cost = np.where(trav, np.where(reached, d, UNREACHED), BLOCKED).astype(np.uint32)
    stats = dict(voxels_traversable=int(trav.sum()), voxels_reached=int(reached.sum()), goals_used=int(ok.sum()), goals_blocked=int(len(ok) - ok.sum()),
                 largest_cost=int(d[reached].max()) if reached.any() else 0)
    return Field(store.org.copy(), cost, stats, voxel_size)


def paths(fld, starts, max_waypoints):
    """All starts walk together, one step per round for those still on their way."""
    v, ok = voxel_of(starts, fld.voxel_size)
    n = len(v)
    cost = np.where(ok, fld.at(v), BLOCKED).astype(np.uint32)
    status = np.where(cost == BLOCKED, PATH_BLOCKED, np.where(cost > MAX_COST, UNREACHABLE, TRUNCATED)).astype(np.uint8)
    n_wp = np.zeros(n, np.uint32)
    wp = np.full((n, max_waypoints, 3), WAYPOINT_FILL, F)
    cur = cost.astype(np.int64)
    live = status == TRUNCATED
    v = v.copy()
    for it in range(max_waypoints):
        at = np.nonzero(live)[0]
        if len(at) == 0:
            break
        wp[at, it] = (v[at].astype(F) + F(0.5)) * F(fld.voxel_size)
        n_wp[at] = it + 1
        done = cur[at] == 0
        status[at[done]] = REACHED
        live[at[done]] = False
        at = at[~done]
        chosen = np.full(len(at), -1, np.int64)
        for o in range(26):
            u = fld.at(v[at] + OFFSETS[o]).astype(np.int64)
            hit = (chosen < 0) & (u <= MAX_COST) & (u + STEP[o] == cur[at])
            chosen[hit] = o
        lost = chosen < 0
        status[at[lost]] = INVALID
        live[at[lost]] = False
        at, chosen = at[~lost], chosen[~lost]
        v[at] += OFFSETS[chosen]
        cur[at] -= STEP[chosen]
    stats = dict(paths_reached=int((status == REACHED).sum()), paths_unreachable=int((status == UNREACHABLE).sum()),
                 paths_blocked=int((status == PATH_BLOCKED).sum()), paths_truncated=int((status == TRUNCATED).sum()), waypoints=int(n_wp.sum()))
    return dict(status=status, cost=cost, n_waypoints=n_wp, waypoints=wp, stats=stats)


def model_of(g, goals, **cfg):
    """The model's field for the ESDF an integrator has stored."""
    from tests import mesh_case
    return field(E.store_of(g), goals, mesh_case.VOXEL, **cfg)


def assert_field(g, got_stats, model, what=""):
    """The library's field against the model: every block of the map, a ring of absent blocks around it, and the five contractual statistics."""
    idx = g.block_indices()
    got, want = g.nav_blocks(idx), model.blocks(idx, g.vps)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: the field differs at %d voxels, first block %s local %d: %#x vs %#x" % (
            what, len(bad), idx[bad[0][0]], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])]))
    assert {k: got_stats[k] for k in STAT_KEYS} == model.stats, (what, got_stats, model.stats)
    return idx, got


def assert_paths(got, want, what=""):
    for k in ("status", "cost", "n_waypoints", "waypoints"):
        if k in got:
            a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
            assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
            if a.tobytes() != b.tobytes():
                bad = np.nonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1))[0]
                raise AssertionError("%s: %s differs at %d of %d starts, first %d: %r vs %r" % (what, k, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]]))
    if got.get("stats") is not None:
        assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
