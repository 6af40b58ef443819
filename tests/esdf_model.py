"""The yardstick of the ESDF tests: a NumPy restatement of the ESDF contract (DESIGN.md, section "ESDF"), written from the
contract and not from the kernels.  Integers are np.uint64 / np.int64, floats np.float32 (IEEE single, no fused operations).

    esdf_from_blocks(indices, tsdf, labels, vps, voxel_size, form=..., **cfg) -> Model

takes host-layout blocks as HipIntegrator.download() returns them.  A voxel the download shows with weight 0 is not
observed, whether its tile is resident or not, so blocks are all the model needs.  Two forms of the windowed minimum:
"brute" takes it over the full (2R+1)^3 window by shifted arrays — the definition itself; "separable" takes three 1-D
windowed minima in a row, for larger maps (tests/test_esdf_cpu.py shows they agree before either judges anything)."""
import numpy as np

F = np.float32
U = np.uint64
RECORD_DTYPE = np.dtype([("distance", "<f4"), ("flags", "u1"), ("label", "u1"), ("pad", "u1", (2,))])
DEFAULTS = dict(min_weight=1e-6, min_distance_m=0.2, max_distance_m=2.0)
# "no site": above every key (d2 <= 3 * 255^2 < 2^18, so keys stay below 2^58) and still a uint64 after d2 << 40 is added
NONE = U(1 << 63)
LOW = U((1 << 40) - 1)


def reach(max_distance_m, voxel_size):
    return int(np.ceil(F(max_distance_m) / F(voxel_size)))


def default_records(shape):
    r = np.zeros(shape, RECORD_DTYPE)
    r["label"] = 255
    return r


class Model:
    """origin: voxel index of dense[0, 0, 0]; dense: records [z, y, x] over the bounding box of the blocks; stats: dict."""

    def __init__(self, origin, dense, stats, vps, keys=None):
        self.origin, self.dense, self.stats, self.vps, self.keys = origin, dense, stats, vps, keys

    def blocks(self, indices, region=None):
        """(n, vps^3) records of host-layout blocks; outside the map, and outside `region` (block_min, block_max, inclusive),
        default records."""
        indices = np.asarray(indices, np.int64).reshape(-1, 3)
        v = self.vps
        out = default_records((len(indices), v ** 3))
        nz, ny, nx = self.dense.shape
        for j, b in enumerate(indices):
            if region is not None and not all(region[0][a] <= b[a] <= region[1][a] for a in range(3)):
                continue
            x0, y0, z0 = (b * v - self.origin)
            if x0 < 0 or y0 < 0 or z0 < 0 or x0 + v > nx or y0 + v > ny or z0 + v > nz:
                continue
            out[j] = self.dense[z0:z0 + v, y0:y0 + v, x0:x0 + v].reshape(-1)
        return out

    def at(self, ijk):
        """Records of the voxels with integer indices ijk (n, 3): default records outside the box."""
        ijk = np.asarray(ijk, np.int64).reshape(-1, 3) - self.origin
        nz, ny, nx = self.dense.shape
        ok = ((ijk >= 0) & (ijk < np.array([nx, ny, nz]))).all(axis=1)
        out = default_records(len(ijk))
        out[ok] = self.dense[ijk[ok, 2], ijk[ok, 1], ijk[ok, 0]]
        return out


def window_min_brute(planes, R):
    """planes (p, nz, ny, nx) uint64 -> min over |dx|, |dy|, |dz| <= R of plane[v + d] + (|d|^2 << 40)."""
    p, nz, ny, nx = planes.shape
    pad = np.full((p, nz + 2 * R, ny + 2 * R, nx + 2 * R), NONE, U)
    pad[:, R:R + nz, R:R + ny, R:R + nx] = planes
    acc = np.full(planes.shape, NONE, U)
    tmp = np.empty(planes.shape, U)
    for dz in range(-R, R + 1):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                np.add(pad[:, R + dz:R + dz + nz, R + dy:R + dy + ny, R + dx:R + dx + nx], U((dx * dx + dy * dy + dz * dz) << 40), out=tmp)
                np.minimum(acc, tmp, out=acc)
    return acc


def window_min_separable(planes, R):
    """The same minimum as three 1-D windowed minima: x, then y, then z."""
    cur = planes
    for axis in (3, 2, 1):
        n = cur.shape[axis]
        shape = list(cur.shape)
        shape[axis] = n + 2 * R
        pad = np.full(shape, NONE, U)
        sl = [slice(None)] * 4
        sl[axis] = slice(R, R + n)
        pad[tuple(sl)] = cur
        acc = np.full(cur.shape, NONE, U)
        tmp = np.empty(cur.shape, U)
        for o in range(-R, R + 1):
            sl[axis] = slice(R + o, R + o + n)
            np.add(pad[tuple(sl)], U((o * o) << 40), out=tmp)
            np.minimum(acc, tmp, out=acc)
        cur = acc
    return cur


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


def esdf_from_blocks(indices, tsdf, labels, vps, voxel_size, form="separable", keep_keys=False, **cfg):
    c = dict(DEFAULTS, **cfg)
    vs, mw, dmin, dmax = F(voxel_size), F(c["min_weight"]), F(c["min_distance_m"]), F(c["max_distance_m"])
    R = reach(dmax, vs)
    assert R <= 255
    if len(indices) == 0:
        return Model(np.zeros(3, np.int64), default_records((0, 0, 0)), dict(voxels_observed=0, voxels_fixed=0, voxels_clamped=0), vps)
    origin, D, W, L = dense_from_blocks(indices, tsdf, labels, vps)
    observed = W >= mw
    neg = D < F(0)
    site = observed & (np.abs(D) < dmin)
    key = (np.abs(D).view(np.uint32).astype(U) << U(8)) | L.astype(U)
    planes = np.stack([np.where(site & ~neg, key, NONE), np.where(site & neg, key, NONE)])
    best = (window_min_brute if form == "brute" else window_min_separable)(planes, R)
    k = np.where(neg, best[1], best[0])
    found = k < NONE
    d2 = (k >> U(40)).astype(np.int64)
    w = ((k >> U(8)) & U(0xffffffff)).astype(np.uint32).view(F)
    centre = vs * np.sqrt(np.where(found, d2, 0).astype(F))
    total = centre + w
    assert centre.dtype == F and total.dtype == F
    dist = np.where(found, np.minimum(dmax, total), dmax).astype(F)
    sign = np.where(neg, F(-1), F(1))
    far = observed & ~site
    rec = default_records(D.shape)
    rec["distance"] = np.where(site, D, np.where(far, sign * dist, F(0)))
    rec["flags"] = observed.astype(np.uint8) | (site.astype(np.uint8) << 1)
    rec["label"] = np.where(site, L, np.where(far & found, (k & U(0xff)).astype(np.uint8), 255))
    clamped = far & (~found | ~(total < dmax))
    stats = dict(voxels_observed=int(observed.sum()), voxels_fixed=int(site.sum()), voxels_clamped=int(clamped.sum()))
    return Model(origin, rec, stats, vps, keys=(planes, best, far, neg) if keep_keys else None)


def tied_voxels(model, R, form="brute"):
    """Observed voxels outside the band whose minimum-d2 sites (two or more) differ in (|distance|, label): where the
    secondary keys decide.  The largest low part among the sites at the minimum d2, against the smallest: the minimum of the
    keys with their low parts flipped.  That minimum separates like the key's own: adding o^2 << 40 keeps the order of a
    flipped low part just as it keeps that of the low part, so form "separable" takes it for larger windows
    (tests/test_esdf_cpu.py shows the two forms agree)."""
    planes, best, far, neg = model.keys
    flipped = np.where(planes < NONE, (planes & ~LOW) | (~planes & LOW), NONE)
    other = (window_min_brute if form == "brute" else window_min_separable)(flipped, R)
    k = np.where(neg, best[1], best[0])
    o = np.where(neg, other[1], other[0])
    found = far & (k < NONE)
    assert ((k >> U(40)) == (o >> U(40)))[found].all()
    return int((found & ((k & LOW) != (~o & LOW))).sum())


def found_d2(model):
    """(found, d2) over the dense box: the observed voxels outside the band that have a site in their window, and the squared
    offset, in voxels, of the site that won (0 where none did)."""
    planes, best, far, neg = model.keys
    k = np.where(neg, best[1], best[0])
    found = far & (k < NONE)
    return found, np.where(found, k >> U(40), U(0)).astype(np.int64)


def model_of(g, cfg=None, form="separable", **kw):
    """The model's ESDF of the map an integrator holds (through download())."""
    idx, t, s = g.download()
    return esdf_from_blocks(idx, t, s["label"], g.vps, g.cfg.voxel_size, form=form, **dict(cfg or {}), **kw)


def assert_same(records, want, what=""):
    """The bytes of the records: every voxel of every block."""
    a, b = np.ascontiguousarray(records), np.ascontiguousarray(want)
    assert a.dtype.itemsize == 8 and b.dtype.itemsize == 8 and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
        raise AssertionError("%s: %d of %d records differ, first at %r: %r vs %r" % (what, len(bad), a.size, tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))
