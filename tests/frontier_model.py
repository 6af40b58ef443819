"""NumPy restatement of the frontier contract (DESIGN.md, section "Exploration frontiers"), written from the contract and not from
the kernels: the yardstick of tests/test_frontier_cpu.py and tests/test_frontier_gpu.py.

    frontiers(store, field=None, **cfg) -> Model      store: esdf_read_model.Store; field: nav_model.Field of the same store, or None
    model_of(g, field=None, **cfg)                    ... of the ESDF an integrator has stored
    assert_same(got, model, block_idx, ids, what)     every record byte, every stat except workspace_bytes, every voxel id

The dense store of tests/nav_model.py with a border of one unobserved voxel (a voxel outside the store's tiles reads the default
record), six shifted observed arrays for the face test, the 13 forward offsets as an edge list and a plain union-find
(tests/objects_model.py) for the clusters.  tests/test_frontier_cpu.py validates it against scipy.ndimage.label and against closed
forms before it judges anything."""
import numpy as np

from tests import nav_model as N
from tests import objects_model as O

F = np.float32
NONE = O.NONE
DEFAULTS = dict(radius_m=0.3, min_voxels=8, use_bounds=0, bounds_min=(0, 0, 0), bounds_max=(0, 0, 0))
RECORD_DTYPE = np.dtype([("first_voxel", "<i4", (3,)), ("n_voxels", "<u4"), ("bb_min", "<i4", (3,)), ("bb_max", "<i4", (3,)),
                         ("sum", "<i8", (3,)), ("unknown_faces", "<u4"), ("nav_cost", "<u4"), ("nav_voxel", "<i4", (3,)), ("pad", "<u4")])
STAT_KEYS = ("voxels_traversable", "voxels_frontier", "components", "frontiers", "voxels_in_frontiers", "largest_frontier_voxels",
             "unknown_faces", "nav_field_used")
FACES = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))   # (dx, dy, dz)


def unpack_coord3(word):
    w = np.asarray(word, np.uint64)
    m = np.uint64(0x1fffff)
    return np.stack([(w >> np.uint64(42)) & m, (w >> np.uint64(21)) & m, w & m], axis=-1).astype(np.int64) - O.BIAS


def frontier_mask(store, c):
    """Dense [z, y, x]: (frontier voxel, its unknown_faces, traversable)."""
    observed = (store.flags & 1) != 0
    trav = N.traversable_of(store, c["radius_m"])
    nz, ny, nx = observed.shape
    pad = np.zeros((nz + 2, ny + 2, nx + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = observed
    unknown = np.zeros(observed.shape, np.int64)
    for dx, dy, dz in FACES:
        unknown += ~pad[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
    cand = trav
    if c["use_bounds"]:
        lo, hi = np.asarray(c["bounds_min"], np.int64), np.asarray(c["bounds_max"], np.int64)
        z, y, x = np.meshgrid(*(np.arange(n) + o for n, o in zip((nz, ny, nx), store.org[::-1])), indexing="ij")
        cand = trav & (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (z >= lo[2]) & (z <= hi[2])
    part = cand & (unknown > 0)
    return part, np.where(part, unknown, 0), trav


def frontiers(store, field=None, **cfg):
    c = dict(DEFAULTS, **{k: v for k, v in cfg.items() if v is not None})
    vps = cfg.get("vps", 8)
    part, unknown, trav = frontier_mask(store, c)
    comp, nc = O.components_of(part, np.zeros(part.shape, np.int64))
    z, y, x = np.nonzero(part)
    xyz = np.stack([x, y, z], axis=1).astype(np.int64) + store.org
    k = comp[part]
    word = O.pack_coord3(xyz) if len(xyz) else np.zeros(0, np.uint64)
    n = np.bincount(k, minlength=nc).astype(np.int64)
    first = np.full(nc, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(first, k, word)
    bb_min, bb_max = np.full((nc, 3), np.iinfo(np.int64).max), np.full((nc, 3), np.iinfo(np.int64).min)
    np.minimum.at(bb_min, k, xyz)
    np.maximum.at(bb_max, k, xyz)
    sums = np.zeros((nc, 3), np.int64)
    np.add.at(sums, k, xyz)
    faces = np.zeros(nc, np.int64)
    np.add.at(faces, k, unknown[part])
    # the join: first the smallest reached cost, then the smallest voxel at that cost
    nav_cost = np.full(nc, N.UNREACHED, np.int64)
    nav_word = first.copy()
    if field is not None and len(xyz):
        cost = field.at(xyz).astype(np.int64)
        ok = cost <= N.MAX_COST
        np.minimum.at(nav_cost, k[ok], cost[ok])
        best = ok & (cost == nav_cost[k])
        at = np.full(nc, np.iinfo(np.uint64).max, np.uint64)
        np.minimum.at(at, k[best], word[best])
        nav_word = np.where(nav_cost != N.UNREACHED, at, first)
    keep = np.nonzero(n >= int(c["min_voxels"]))[0]
    keep = keep[np.argsort(first[keep], kind="stable")]
    rec = np.zeros(len(keep), RECORD_DTYPE)
    if len(keep):
        rec["first_voxel"], rec["nav_voxel"] = unpack_coord3(first[keep]), unpack_coord3(nav_word[keep])
        rec["n_voxels"], rec["bb_min"], rec["bb_max"], rec["sum"] = n[keep], bb_min[keep], bb_max[keep], sums[keep]
        rec["unknown_faces"], rec["nav_cost"] = faces[keep], nav_cost[keep]
    final_of = np.full(nc + 1, NONE, np.uint32)      # (the last entry serves component -1)
    final_of[keep] = np.arange(len(keep), dtype=np.uint32)
    stats = dict(voxels_traversable=int(trav.sum()), voxels_frontier=int(part.sum()), components=nc, frontiers=len(keep),
                 voxels_in_frontiers=int(n[keep].sum()), largest_frontier_voxels=int(n[keep].max()) if len(keep) else 0,
                 unknown_faces=int(unknown.sum()), nav_field_used=int(field is not None))
    m = O.Model(store.org.copy(), final_of[comp], rec, stats, vps, components=comp)
    m.part = part
    return m


def model_of(g, field=None, **cfg):
    from tests import esdf_read_model as E
    return frontiers(E.store_of(g), field, vps=g.vps, **cfg)


def workspace_bytes(n_tiles, components):
    """DESIGN.md, "Exploration frontiers": 10 bytes per voxel and 128 per tile of the store, 96 of counters, 196 per component."""
    return 10 * 512 * n_tiles + 128 * n_tiles + 96 + 196 * components


def by_first(rec):
    return {tuple(int(v) for v in r["first_voxel"]): (int(r["n_voxels"]), int(r["unknown_faces"])) for r in rec}


def assert_same(got, model, idx, ids, what=""):
    """got = (records, stats) of HipIntegrator.frontiers(); ids = frontier_ids(idx): every record, every stat, every voxel's id."""
    rec, stats = got
    rec = np.ascontiguousarray(rec)
    assert rec.dtype.itemsize == 88 and model.records.dtype.itemsize == 88
    for key in STAT_KEYS:
        assert stats[key] == model.stats[key], (what, key, stats[key], model.stats[key], stats, model.stats)
    assert len(rec) == len(model.records), (what, len(rec), len(model.records))
    if rec.tobytes() != model.records.tobytes():
        bad = [i for i in range(len(rec)) if rec[i].tobytes() != model.records[i].tobytes()]
        raise AssertionError("%s: %d of %d records differ, first %d: %r vs %r" % (what, len(bad), len(rec), bad[0], rec[bad[0]], model.records[bad[0]]))
    want = model.blocks(idx)
    ids = np.ascontiguousarray(ids)
    assert ids.shape == want.shape and ids.dtype == np.uint32, (what, ids.shape, want.shape)
    if ids.tobytes() != want.tobytes():
        bad = np.argwhere(ids != want)
        raise AssertionError("%s: %d of %d ids differ, first at %r: %r vs %r" % (what, len(bad), ids.size, tuple(bad[0]), ids[tuple(bad[0])], want[tuple(bad[0])]))
