"""NumPy restatement of the rooms contract (DESIGN.md, section "Rooms"), written from the contract and not from the kernels: the
yardstick of tests/test_rooms_cpu.py and tests/test_rooms_gpu.py.

    rooms(store, objects=None, **cfg) -> Model     store: esdf_read_model.Store; objects: (n_objects, dense ids [z, y, x]) or None
    model_of(g, **cfg)                             ... of the ESDF (and the objects) an integrator has stored
    assert_same(got, model, block_idx, ids, costs, what)   every record and link byte, every contractual stat, both planes

The dense store of tests/nav_model.py, the core components by the plain union-find of tests/objects_model.py, and the growth by
Dijkstra's algorithm over cost levels that carries the pair (cost, room): when level c is taken, every neighbour one step nearer is
final, so a node's room is the smallest room among the neighbours u with cost(u) + w(u, v) == c.  Links by shifting the dense room
array 26 times.  tests/test_rooms_cpu.py validates it against scipy (ndimage.label, csgraph.dijkstra per room) and a closed form
before it judges anything."""
import heapq

import numpy as np

from tests import nav_model as N
from tests import objects_model as O

F = np.float32
NONE = O.NONE
DEFAULTS = dict(free_distance_m=0.0, core_distance_m=0.5, min_core_voxels=64, max_cost=0, max_rounds=0, use_bounds=0, bounds_min=(0, 0, 0),
                bounds_max=(0, 0, 0))
ROOM_DTYPE = np.dtype([("first_voxel", "<i4", (3,)), ("n_core_voxels", "<u4"), ("bb_min", "<i4", (3,)), ("bb_max", "<i4", (3,)),
                       ("sum", "<i8", (3,)), ("n_voxels", "<u4"), ("largest_cost", "<u4"), ("clearance_bits", "<u4"),
                       ("centre_voxel", "<i4", (3,)), ("n_links", "<u4"), ("n_objects", "<u4")])
LINK_DTYPE = np.dtype([("room_a", "<u4"), ("room_b", "<u4"), ("n_contacts", "<u4"), ("clearance_bits", "<u4"), ("door_voxel", "<i4", (3,)),
                       ("door_room", "<u4")])
STAT_KEYS = ("voxels_free", "voxels_core", "components", "rooms", "voxels_assigned", "voxels_unassigned", "largest_room_voxels", "largest_cost",
             "links", "contacts", "objects_seen", "objects_joined")
_INF = np.int64(1) << 40
_BIG = np.int64(1) << 40


def unpack_coord3(word):
    w = np.asarray(word, np.uint64)
    m = np.uint64(0x1fffff)
    return np.stack([(w >> np.uint64(42)) & m, (w >> np.uint64(21)) & m, w & m], axis=-1).astype(np.int64) - O.BIAS


def classes(store, c):
    """Dense [z, y, x] bool: (free, core)."""
    with np.errstate(invalid="ignore"):
        free = ((store.flags & 1) != 0) & (store.dist >= F(c["free_distance_m"]))
        if c["use_bounds"]:
            lo, hi = np.asarray(c["bounds_min"], np.int64), np.asarray(c["bounds_max"], np.int64)
            nz, ny, nx = free.shape
            z, y, x = np.meshgrid(*(np.arange(n) + o for n, o in zip((nz, ny, nx), store.org[::-1])), indexing="ij")
            free &= (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (z >= lo[2]) & (z <= hi[2])
        core = free & (store.dist >= F(c["core_distance_m"]))
    return free, core


def grow(free, seed_room, cap):
    """Dense (cost int64 with _INF where unreached, room int64 with _BIG there) from seed_room [z, y, x] (>= 0 on the seeds, -1
    elsewhere): the lexicographic minimum of (path cost, room of the path's start) over the free voxels, 26-connected."""
    nz, ny, nx = free.shape
    pad = np.zeros((nz + 2, ny + 2, nx + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = free
    sy, sz = nx + 2, (nx + 2) * (ny + 2)
    ok = pad.reshape(-1)
    off = N.OFFSETS[:, 0] + sy * N.OFFSETS[:, 1] + sz * N.OFFSETS[:, 2]
    dist = np.full(ok.size, _INF, np.int64)
    room = np.full(ok.size, _BIG, np.int64)
    sr = np.full(pad.shape, -1, np.int64)
    sr[1:-1, 1:-1, 1:-1] = seed_room
    seeds = np.nonzero(sr.reshape(-1) >= 0)[0]
    dist[seeds] = 0
    room[seeds] = sr.reshape(-1)[seeds]
    levels, buckets = ([0], {0: [seeds]}) if len(seeds) else ([], {})
    while levels:
        c = heapq.heappop(levels)
        nodes = np.unique(np.concatenate(buckets.pop(c)))
        nodes = nodes[dist[nodes] == c]
        if len(nodes) == 0:
            continue
        nb = nodes[:, None] + off[None, :]
        if c > 0:                                       # every neighbour one step nearer is final: the smallest room among them
            pred = ok[nb] & (dist[nb] + N.STEP[None, :] == c)
            room[nodes] = np.where(pred, room[nb], _BIG).min(axis=1)
        cand = np.broadcast_to(c + N.STEP[None, :], nb.shape)
        better = ok[nb] & (cand < dist[nb]) & (cand <= cap)
        nbs, cs = nb[better], cand[better]
        np.minimum.at(dist, nbs, cs)
        for value in np.unique(cs):
            if value not in buckets:
                buckets[value] = []
                heapq.heappush(levels, int(value))
            buckets[value].append(nbs[cs == value])
    inner = (slice(1, -1),) * 3
    return dist.reshape(pad.shape)[inner], room.reshape(pad.shape)[inner]


class Model(O.Model):
    """ids: the room plane; cost: the cost plane (dense [z, y, x] uint32); records, links, room_of_object, stats."""

    def cost_blocks(self, indices):
        m = O.Model(self.origin, self.cost, None, None, self.vps)
        return m.blocks(indices)


def rooms(store, objects=None, **cfg):
    c = dict(DEFAULTS, **{k: v for k, v in cfg.items() if v is not None and k != "vps"})
    vps = cfg.get("vps", 8)
    cap = int(c["max_cost"]) if c["max_cost"] else N.MAX_COST
    free, core = classes(store, c)
    comp, nc = O.components_of(core, np.zeros(core.shape, np.int64))
    nz, ny, nx = free.shape
    gz, gy, gx = np.meshgrid(*(np.arange(n) + o for n, o in zip((nz, ny, nx), store.org[::-1])), indexing="ij")
    xyz_all = np.stack([gx, gy, gz], axis=-1).astype(np.int64)
    word_all = O.pack_coord3(xyz_all.reshape(-1, 3)).reshape(free.shape) if free.size else np.zeros(free.shape, np.uint64)
    bits_all = np.ascontiguousarray(store.dist, F).view(np.uint32)
    # the rooms: components of at least min_core_voxels, ascending by their smallest core voxel
    k = comp[core]
    n_core = np.bincount(k, minlength=nc).astype(np.int64)
    first = np.full(nc, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(first, k, word_all[core])
    keep = np.nonzero(n_core >= int(c["min_core_voxels"]))[0]
    keep = keep[np.argsort(first[keep], kind="stable")]
    nr = len(keep)
    final_of = np.full(nc + 1, -1, np.int64)
    final_of[keep] = np.arange(nr)
    seed_room = final_of[comp]                           # (component -1 reads the last entry: -1)
    dist, room = grow(free, seed_room, cap)
    assigned = free & (dist < _INF)
    rec = np.zeros(nr, ROOM_DTYPE)
    ids = np.where(assigned, room, int(NONE)).astype(np.uint32)
    cost = np.where(free, np.where(assigned, dist, N.UNREACHED), N.BLOCKED).astype(np.uint32)
    r = room[assigned]
    xyz = xyz_all[assigned]
    if nr:
        rec["first_voxel"], rec["n_core_voxels"] = unpack_coord3(first[keep]), n_core[keep]
        rec["n_voxels"] = np.bincount(r, minlength=nr)
        bb_min, bb_max = np.full((nr, 3), np.iinfo(np.int64).max), np.full((nr, 3), np.iinfo(np.int64).min)
        np.minimum.at(bb_min, r, xyz)
        np.maximum.at(bb_max, r, xyz)
        sums = np.zeros((nr, 3), np.int64)
        np.add.at(sums, r, xyz)
        big = np.zeros(nr, np.int64)
        np.maximum.at(big, r, dist[assigned])
        rec["bb_min"], rec["bb_max"], rec["sum"], rec["largest_cost"] = bb_min, bb_max, sums, big
        # the clearance: first the largest bits among the room's cores, then the smallest voxel attaining them
        seeds = seed_room >= 0
        sr, sb, sw = seed_room[seeds], bits_all[seeds].astype(np.int64), word_all[seeds]
        clear = np.zeros(nr, np.int64)
        np.maximum.at(clear, sr, sb)
        at = np.full(nr, np.iinfo(np.uint64).max, np.uint64)
        best = sb == clear[sr]
        np.minimum.at(at, sr[best], sw[best])
        rec["clearance_bits"], rec["centre_voxel"] = clear, unpack_coord3(at)
    # the links: (voxel, other room) incidences, each voxel once per other room
    lab = np.full((nz + 2, ny + 2, nx + 2), -1, np.int64)
    lab[1:-1, 1:-1, 1:-1] = np.where(assigned, room, -1)
    own = lab[1:-1, 1:-1, 1:-1]
    pairs = []
    for dx, dy, dz in N.OFFSETS:
        other = lab[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
        hit = (own >= 0) & (other >= 0) & (other != own)
        flat = np.nonzero(hit.reshape(-1))[0]
        pairs.append(np.stack([flat, other.reshape(-1)[flat]], axis=1))
    pairs = np.unique(np.concatenate(pairs), axis=0) if pairs else np.zeros((0, 2), np.int64)
    flat, q = pairs[:, 0], pairs[:, 1]
    rr = own.reshape(-1)[flat]
    a, b = np.minimum(rr, q), np.maximum(rr, q)
    key = a * (1 << 32) + b
    link_keys = np.unique(key)
    links = np.zeros(len(link_keys), LINK_DTYPE)
    j = np.searchsorted(link_keys, key)
    if len(link_keys):
        links["room_a"], links["room_b"] = link_keys >> 32, link_keys & 0xffffffff
        links["n_contacts"] = np.bincount(j, minlength=len(link_keys))
        cb, cw = bits_all.reshape(-1)[flat].astype(np.int64), word_all.reshape(-1)[flat]
        clear = np.zeros(len(link_keys), np.int64)
        np.maximum.at(clear, j, cb)
        at = np.full(len(link_keys), np.iinfo(np.uint64).max, np.uint64)
        best = cb == clear[j]
        np.minimum.at(at, j[best], cw[best])
        door = unpack_coord3(at)
        links["clearance_bits"], links["door_voxel"] = clear, door
        l = door - store.org
        links["door_room"] = own[l[:, 2], l[:, 1], l[:, 0]]
        rec["n_links"] = np.bincount(np.concatenate([links["room_a"], links["room_b"]]).astype(np.int64), minlength=nr)
    # the join with the objects: the minimum of (cost, room) over each object's assigned voxels
    n_obj, room_of = 0, np.zeros(0, np.uint32)
    if objects is not None:
        n_obj, oid = objects
        room_of = np.full(n_obj, NONE, np.uint32)
        m = assigned & (oid != NONE) & (oid < n_obj)
        pair = dist[m] * (1 << 32) + room[m]
        best = np.full(n_obj, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(best, oid[m].astype(np.int64), pair)
        joined = best != np.iinfo(np.int64).max
        room_of[joined] = (best[joined] & 0xffffffff).astype(np.uint32)
        rec["n_objects"] = np.bincount(room_of[joined].astype(np.int64), minlength=nr)
    stats = dict(voxels_free=int(free.sum()), voxels_core=int(core.sum()), components=nc, rooms=nr, voxels_assigned=int(assigned.sum()),
                 voxels_unassigned=int(free.sum() - assigned.sum()), largest_room_voxels=int(rec["n_voxels"].max()) if nr else 0,
                 largest_cost=int(rec["largest_cost"].max()) if nr else 0, links=len(links), contacts=int(len(pairs)), objects_seen=int(n_obj),
                 objects_joined=int((room_of != NONE).sum()))
    m = Model(store.org.copy(), ids, rec, stats, vps, components=comp)
    m.cost, m.links, m.room_of_object, m.free, m.core, m.dist = cost, links, room_of, free, core, dist
    return m


def dense_ids(store, idx, ids, vps):
    """Per-voxel ids of host-layout blocks as a dense [z, y, x] array over the store's box (NONE elsewhere)."""
    out = np.full(store.shape, NONE, np.uint32)
    for j, b in enumerate(np.asarray(idx, np.int64).reshape(-1, 3)):
        x, y, z = b * vps - store.org
        out[z:z + vps, y:y + vps, x:x + vps] = ids[j].reshape(vps, vps, vps)
    return out


def model_of(g, with_objects=True, **cfg):
    from tests import esdf_read_model as E
    store = E.store_of(g)
    objects = None
    if with_objects:
        from kimera_semantics_amd import binding as B
        try:
            n_objects = len(g.object_records())
        except B.KsError as e:                            # (no stored objects: the join does not apply)
            assert e.code == B.KS_ERR_INVALID_ARG and "no objects are stored" in str(e), e
            n_objects = None
        if n_objects is not None:
            idx = g.block_indices()
            objects = (n_objects, dense_ids(store, idx, g.object_ids(idx), g.vps))
    return rooms(store, objects, vps=g.vps, **cfg)


def workspace_bytes(n_tiles, stats):
    """DESIGN.md, "Rooms": 13 bytes per voxel and 12 per tile of the store, 12 + 160 of counts and counters, 340 per core component, 48
    per contact, 48 per link, 12 per object seen."""
    return (13 * 512 + 12) * n_tiles + 172 + 340 * stats["components"] + 48 * stats["contacts"] + 48 * stats["links"] + 12 * stats["objects_seen"]


def by_first(rec):
    return {tuple(int(v) for v in r["first_voxel"]): (int(r["n_core_voxels"]), int(r["n_voxels"])) for r in rec}


def _same_bytes(a, b, what, name):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        bad = [i for i in range(len(a)) if a[i].tobytes() != b[i].tobytes()]
        raise AssertionError("%s: %d of %d %s differ, first %d: %r vs %r" % (what, len(bad), len(a), name, bad[0], a[bad[0]], b[bad[0]]))


def assert_same(got, model, idx, ids, costs, what=""):
    """got = (records, links, stats) of HipIntegrator.rooms(); ids, costs = room_ids(idx), room_costs(idx)."""
    rec, links, stats = got
    assert np.asarray(rec).dtype.itemsize == 96 and model.records.dtype.itemsize == 96 and np.asarray(links).dtype.itemsize == 32
    for key in STAT_KEYS:
        assert stats[key] == model.stats[key], (what, key, stats[key], model.stats[key], stats, model.stats)
    _same_bytes(rec, model.records, what, "records")
    _same_bytes(links, model.links, what, "links")
    for name, have, want in (("ids", ids, model.blocks(idx)), ("costs", costs, model.cost_blocks(idx))):
        have = np.ascontiguousarray(have)
        assert have.shape == want.shape and have.dtype == np.uint32, (what, name, have.shape, want.shape)
        if have.tobytes() != want.tobytes():
            bad = np.argwhere(have != want)
            raise AssertionError("%s: %d of %d %s differ, first at %r: %#x vs %#x" % (what, len(bad), have.size, name, tuple(bad[0]), have[tuple(bad[0])],
                                                                                      want[tuple(bad[0])]))
