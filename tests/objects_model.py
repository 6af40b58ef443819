"""NumPy restatement of the object-instance contract (DESIGN.md, section "Object instances"), written from the contract and not
from the kernels: the yardstick of tests/test_objects_cpu.py and tests/test_objects_gpu.py.

A dense array over the bounding box of the downloaded blocks (an absent tile reads as weight 0: a neighbour that does not
exist), the voxels that take part, their 13 forward neighbour offsets as an edge list, a plain union-find over the edges.
tests/test_objects_cpu.py validates it against scipy.ndimage.label and on an analytic sphere before it judges anything."""
import numpy as np

F = np.float32
NONE = np.uint32(0xffffffff)
DEFAULTS = dict(min_weight=1e-4, surface_distance_m=0.0, label_mask=0x1fffff, min_voxels=8)
RECORD_DTYPE = np.dtype([("first_voxel", "<i4", (3,)), ("n_voxels", "<u4"), ("bb_min", "<i4", (3,)), ("bb_max", "<i4", (3,)),
                         ("sum", "<i8", (3,)), ("label", "<u4"), ("pad", "<u4")])
STAT_KEYS = ("voxels_surface", "components", "objects", "voxels_in_objects", "largest_object_voxels")
BIAS = 1 << 20
# the 13 offsets (dx, dy, dz) that come after (0, 0, 0): every unordered pair of 26-neighbours once
FORWARD = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) > (0, 0, 0)]


def pack_coord3(xyz):
    """(n, 3) signed voxel indices -> the 63-bit word whose order is the order of (x, y, z)."""
    v = (np.asarray(xyz, np.int64) + BIAS).astype(np.uint64)
    return (v[:, 0] << np.uint64(42)) | (v[:, 1] << np.uint64(21)) | v[:, 2]


class Model:
    """origin: voxel index of ids[0, 0, 0]; ids: object index per voxel [z, y, x] over the bounding box of the blocks (NONE elsewhere);
    records: RECORD_DTYPE, ascending by first_voxel; stats: dict; components: provisional component per voxel, -1 = takes no part."""

    def __init__(self, origin, ids, records, stats, vps, components=None):
        self.origin, self.ids, self.records, self.stats, self.vps, self.components = origin, ids, records, stats, vps, components

    def blocks(self, indices):
        """(n, vps^3) ids of host-layout blocks; NONE outside the map."""
        indices = np.asarray(indices, np.int64).reshape(-1, 3)
        v = self.vps
        out = np.full((len(indices), v ** 3), NONE, np.uint32)
        nz, ny, nx = self.ids.shape
        for j, b in enumerate(indices):
            x0, y0, z0 = (b * v - self.origin)
            if x0 < 0 or y0 < 0 or z0 < 0 or x0 + v > nx or y0 + v > ny or z0 + v > nz:
                continue
            out[j] = self.ids[z0:z0 + v, y0:y0 + v, x0:x0 + v].reshape(-1)
        return out

    def at(self, ijk):
        """Ids of the voxels with integer indices ijk (n, 3): NONE outside the box."""
        ijk = np.asarray(ijk, np.int64).reshape(-1, 3) - self.origin
        nz, ny, nx = self.ids.shape
        ok = ((ijk >= 0) & (ijk < np.array([nx, ny, nz]))).all(axis=1)
        out = np.full(len(ijk), NONE, np.uint32)
        out[ok] = self.ids[ijk[ok, 2], ijk[ok, 1], ijk[ok, 0]]
        return out

    def centroids(self, voxel_size):
        r = self.records
        return (r["sum"].astype(np.float64) / np.maximum(r["n_voxels"], 1)[:, None] + 0.5) * float(voxel_size)


def dense_from_blocks(indices, tsdf, labels, vps):
    indices = np.asarray(indices, np.int64).reshape(-1, 3)
    lo, hi = indices.min(axis=0) * vps, (indices.max(axis=0) + 1) * vps
    nx, ny, nz = (hi - lo)
    D, W, L = np.zeros((nz, ny, nx), F), np.zeros((nz, ny, nx), F), np.zeros((nz, ny, nx), np.uint8)
    for j, b in enumerate(indices):
        x0, y0, z0 = b * vps - lo
        sl = (slice(z0, z0 + vps), slice(y0, y0 + vps), slice(x0, x0 + vps))
        D[sl] = np.asarray(tsdf["distance"][j], F).reshape(vps, vps, vps)
        W[sl] = np.asarray(tsdf["weight"][j], F).reshape(vps, vps, vps)
        L[sl] = np.asarray(labels[j], np.uint8).reshape(vps, vps, vps)
    return lo, D, W, L


def taking_part(D, W, L, voxel_size, c):
    sd = F(c["surface_distance_m"]) if F(c["surface_distance_m"]) != 0 else F(voxel_size)
    with np.errstate(invalid="ignore"):
        surface = (W >= F(c["min_weight"])) & (np.abs(D) <= sd)      # (a NaN distance compares false)
    lab = np.where(L == 255, 0, L).astype(np.int64)
    in_mask = (lab < 21) & (((np.int64(c["label_mask"]) >> np.minimum(lab, 31)) & 1) == 1)
    return surface & in_mask, lab


def union_find(n, edges):
    """Plain union-find with path halving: the root of each of n nodes."""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(a) for a in range(n)], np.int64)


def components_of(part, lab):
    """Per voxel of the dense array the number of its component (0 .. n - 1), or -1; and n."""
    num = np.full(part.shape, -1, np.int64)
    n = int(part.sum())
    num[part] = np.arange(n)
    nz, ny, nx = part.shape
    edges = []
    for dx, dy, dz in FORWARD:
        a = tuple(slice(max(0, -d), s - max(0, d)) for d, s in ((dz, nz), (dy, ny), (dx, nx)))
        b = tuple(slice(max(0, d), s - max(0, -d)) for d, s in ((dz, nz), (dy, ny), (dx, nx)))
        joined = part[a] & part[b] & (lab[a] == lab[b])
        edges.append(np.stack([num[a][joined], num[b][joined]], axis=1))
    root = union_find(n, np.concatenate(edges).tolist() if edges else [])
    _, comp = np.unique(root, return_inverse=True)
    out = np.full(part.shape, -1, np.int64)
    out[part] = comp
    return out, (int(comp.max()) + 1 if n else 0)


def objects_from_blocks(indices, tsdf, labels, vps, voxel_size, **cfg):
    c = dict(DEFAULTS, **cfg)
    if len(indices) == 0:
        return Model(np.zeros(3, np.int64), np.zeros((0, 0, 0), np.uint32), np.zeros(0, RECORD_DTYPE), dict.fromkeys(STAT_KEYS, 0), vps)
    origin, D, W, L = dense_from_blocks(indices, tsdf, labels, vps)
    part, lab = taking_part(D, W, L, voxel_size, c)
    comp, nc = components_of(part, lab)
    z, y, x = np.nonzero(part)
    xyz = np.stack([x, y, z], axis=1).astype(np.int64) + origin
    k = comp[part]
    n = np.bincount(k, minlength=nc).astype(np.int64)
    first = np.full(nc, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(first, k, pack_coord3(xyz))
    bb_min, bb_max = np.full((nc, 3), np.iinfo(np.int64).max), np.full((nc, 3), np.iinfo(np.int64).min)
    np.minimum.at(bb_min, k, xyz)
    np.maximum.at(bb_max, k, xyz)
    sums = np.zeros((nc, 3), np.int64)
    np.add.at(sums, k, xyz)
    label = np.zeros(nc, np.int64)
    label[k] = lab[part]
    keep = np.nonzero(n >= int(c["min_voxels"]))[0]
    keep = keep[np.argsort(first[keep], kind="stable")]
    rec = np.zeros(len(keep), RECORD_DTYPE)
    f = first[keep]
    rec["first_voxel"] = np.stack([(f >> np.uint64(42)) & np.uint64(0x1fffff), (f >> np.uint64(21)) & np.uint64(0x1fffff), f & np.uint64(0x1fffff)],
                                  axis=1).astype(np.int64) - BIAS
    rec["n_voxels"], rec["bb_min"], rec["bb_max"], rec["sum"], rec["label"] = n[keep], bb_min[keep], bb_max[keep], sums[keep], label[keep]
    final_of = np.full(nc + 1, NONE, np.uint32)      # (the last entry serves component -1)
    final_of[keep] = np.arange(len(keep), dtype=np.uint32)
    ids = final_of[comp]
    stats = dict(voxels_surface=int(part.sum()), components=nc, objects=len(keep), voxels_in_objects=int(n[keep].sum()),
                 largest_object_voxels=int(n[keep].max()) if len(keep) else 0)
    return Model(origin, ids, rec, stats, vps, components=comp)


def model_of(g, cfg=None):
    """The model's objects of the map an integrator holds (through download())."""
    idx, t, s = g.download()
    return objects_from_blocks(idx, t, s["label"], g.vps, g.cfg.voxel_size, **dict(cfg or {}))


def workspace_bytes(n_tiles, components):
    """DESIGN.md, "Object instances": 9 bytes per voxel of the resident tiles, 32 of counters, 164 per component."""
    return 9 * 512 * n_tiles + 32 + 164 * components


def assert_same(got, model, idx, ids, what=""):
    """got = (records, stats) of HipIntegrator.objects(); ids = object_ids(idx): every record, every stat, every voxel's id."""
    rec, stats = got
    rec = np.ascontiguousarray(rec)
    assert rec.dtype.itemsize == 72 and model.records.dtype.itemsize == 72
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
