"""The yardstick of the ESDF read tests: a NumPy restatement of the contract (DESIGN.md, section "ESDF reads"), written from
the contract and not from the kernels.  Operands are np.float32 throughout (IEEE single, no fused operations).

    Store(block_indices, records, vps)              the stored ESDF as HipIntegrator.block_indices() / .esdf_blocks() return it
    sample(store, xyz, voxel_size)                  -> dict(distance, gradient, status, label, flags, stats)
    slice_image(store, origin, du, dv, w, h, vs)    -> the same, (h, w[, 3])
    sweep(store, segments, voxel_size, **cfg)       -> dict(status, t_stop, min_clearance, t_min, stats)

A voxel outside the downloaded blocks reads as the default record: the download gives default records for the tiles of a block that
were not resident when the store was made, and a block that is absent holds no resident tile at all.  All segments walk together, one
sample per round for those still on their way."""
import numpy as np

F = np.float32
LIM = F((1 << 20) - 1)          # the packed range of voxel indices, as ks_esdf_query
EPS = F(1e-6)                   # grid_coord
NAN = np.array([0x7fc00000], np.uint32).view(F)[0]
INF = F(np.inf)
SWEEP_DEFAULTS = dict(radius_m=0.3, min_step_m=0.0, unknown_is_free=0, max_samples=4096)
FREE, COLLISION, UNKNOWN, INVALID = 0, 1, 2, 3


def inv_of(voxel_size):
    """The context's voxel_size_inv."""
    return F(1.0 / np.float64(F(voxel_size)))


class Store:
    """Dense [z, y, x] arrays of distance, flags and label over the bounding box of the blocks; default records elsewhere."""

    def __init__(self, indices, records, vps):
        idx = np.asarray(indices, np.int64).reshape(-1, 3)
        lo = idx.min(axis=0) if len(idx) else np.zeros(3, np.int64)
        hi = idx.max(axis=0) + 1 if len(idx) else np.ones(3, np.int64)
        self.org = lo * vps
        n = (hi - lo) * vps
        self.shape = (int(n[2]), int(n[1]), int(n[0]))
        self.dist, self.flags = np.zeros(self.shape, F), np.zeros(self.shape, np.uint8)
        self.label = np.full(self.shape, 255, np.uint8)
        for j in range(len(idx)):
            x, y, z = (idx[j] - lo) * vps
            sl = (slice(z, z + vps), slice(y, y + vps), slice(x, x + vps))
            self.dist[sl] = records["distance"][j].reshape(vps, vps, vps)
            self.flags[sl] = records["flags"][j].reshape(vps, vps, vps)
            self.label[sl] = records["label"][j].reshape(vps, vps, vps)

    def records(self, v, valid=None):
        """v (n, 3) int64 voxel coordinates -> (distance, flags, label); default records outside the box and where ~valid."""
        l = v - self.org
        ok = ((l >= 0) & (l < np.array(self.shape[::-1]))).all(axis=1)
        if valid is not None:
            ok &= valid
        l = np.clip(l, 0, np.array(self.shape[::-1]) - 1)
        z, y, x = l[:, 2], l[:, 1], l[:, 0]
        return (np.where(ok, self.dist[z, y, x], F(0)), np.where(ok, self.flags[z, y, x], 0).astype(np.uint8),
                np.where(ok, self.label[z, y, x], 255).astype(np.uint8))


def lerp(a, b, f):
    return a + f * (b - a)


def _count(status):
    return dict(points_interpolated=int((status == 2).sum()), points_nearest=int((status == 1).sum()), points_unknown=int((status == 0).sum()))


def sample(store, xyz, voxel_size):
    """E(p) for points (n, 3)."""
    p = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    inv = inv_of(voxel_size)
    with np.errstate(invalid="ignore", over="ignore"):
        g = p * inv - F(0.5)
        i = np.floor(g)
        f = g - i
        ok = np.isfinite(p).all(axis=1) & ((np.abs(i) < LIM) & (np.abs(i + F(1)) < LIM)).all(axis=1)
        nf = np.floor(p * inv + EPS)
        n_ok = ok & (np.abs(nf) < LIM).all(axis=1)
    assert g.dtype == F and f.dtype == F and nf.dtype == F
    iv = np.where(ok[:, None], i, F(0)).astype(np.int64)
    d, all_observed = [], ok.copy()
    for j in range(8):
        dist, flags, _ = store.records(iv + np.array([j & 1, (j >> 1) & 1, j >> 2]), valid=ok)
        d.append(dist)
        all_observed &= (flags & 1) != 0
    n_dist, n_flags, n_label = store.records(np.where(n_ok[:, None], nf, F(0)).astype(np.int64), valid=n_ok)
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        value = lerp(lerp(lerp(d[0], d[1], fx), lerp(d[2], d[3], fx), fy), lerp(lerp(d[4], d[5], fx), lerp(d[6], d[7], fx), fy), fz)
        gx = lerp(lerp(d[1] - d[0], d[3] - d[2], fy), lerp(d[5] - d[4], d[7] - d[6], fy), fz) * inv
        gy = lerp(lerp(d[2] - d[0], d[3] - d[1], fx), lerp(d[6] - d[4], d[7] - d[5], fx), fz) * inv
        gz = lerp(lerp(d[4] - d[0], d[5] - d[1], fx), lerp(d[6] - d[2], d[7] - d[3], fx), fy) * inv
    assert value.dtype == F and gx.dtype == F
    nearest = ok & ~all_observed & ((n_flags & 1) != 0)
    status = np.where(all_observed, 2, np.where(nearest, 1, 0)).astype(np.uint8)
    known = status != 0
    distance = np.where(all_observed, value, np.where(nearest, n_dist, NAN)).astype(F)
    gradient = np.where(all_observed[:, None], np.stack([gx, gy, gz], axis=1), F(0)).astype(F)
    return dict(distance=distance, gradient=gradient, status=status, label=np.where(known, n_label, 255).astype(np.uint8),
                flags=np.where(known, n_flags, 0).astype(np.uint8), stats=_count(status))


def slice_points(origin, du, dv, width, height):
    o, u, v = (np.asarray(a, F).reshape(3) for a in (origin, du, dv))
    fi = np.tile(np.arange(width, dtype=F), height)[:, None]
    fj = np.repeat(np.arange(height, dtype=F), width)[:, None]
    p = (o[None, :] + fi * u[None, :]) + fj * v[None, :]
    assert p.dtype == F
    return p


def slice_image(store, origin, du, dv, width, height, voxel_size):
    out = sample(store, slice_points(origin, du, dv, width, height), voxel_size)
    return {k: (a if k == "stats" else a.reshape((height, width) + a.shape[1:])) for k, a in out.items()}


def sweep(store, segments, voxel_size, **cfg):
    c = dict(SWEEP_DEFAULTS, **cfg)
    seg = np.ascontiguousarray(segments, F).reshape(-1, 6)
    n = len(seg)
    radius = F(c["radius_m"])
    min_step = F(c["min_step_m"]) if F(c["min_step_m"]) > 0 else F(0.5) * F(voxel_size)
    max_samples, unknown_is_free = int(c["max_samples"]), bool(c["unknown_is_free"])
    a, b = seg[:, :3], seg[:, 3:]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = b - a
        L = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        valid = np.isfinite(seg).all(axis=1) & np.isfinite(L) & ~(L > F(max_samples - 2) * min_step)
        u = np.where((L == 0)[:, None], F(0), d / L[:, None]).astype(F)
    assert L.dtype == F
    status = np.full(n, INVALID, np.uint8)
    t, t_stop, t_min = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
    min_c = np.full(n, INF, F)
    live = valid.copy()
    samples = 0
    for _ in range(max_samples):
        at = np.nonzero(live)[0]
        if len(at) == 0:
            break
        ta = t[at]
        E = sample(store, a[at] + ta[:, None] * u[at], voxel_size)
        samples += len(at)
        st, dist = E["status"], E["distance"]
        known = st != 0
        stop_unknown = ~known & (not unknown_is_free)
        with np.errstate(invalid="ignore"):
            cl = np.where(known, dist - radius, F(0)).astype(F)
            lower = known & ~stop_unknown & (cl < min_c[at])
            hit = known & (cl < F(0))
        min_c[at[lower]] = cl[lower]
        t_min[at[lower]] = ta[lower]
        done_free = ~stop_unknown & ~hit & (ta >= L[at])
        for mask, code, where in ((stop_unknown, UNKNOWN, ta), (hit, COLLISION, ta), (done_free, FREE, L[at])):
            status[at[mask]] = code
            t_stop[at[mask]] = where[mask]
        go = ~(stop_unknown | hit | done_free)
        with np.errstate(invalid="ignore"):
            step = np.where(known, np.fmax(cl, min_step), min_step).astype(F)   # (fmaxf: the number when the other operand is NaN)
            t_next = np.fmin(ta + step, L[at]).astype(F)
        t[at[go]] = t_next[go]
        live[at[~go]] = False
    left = live   # the bound: INVALID with the outputs of an invalid segment
    t_stop[left], t_min[left], min_c[left] = F(0), F(0), INF
    stats = dict(segments_free=int((status == FREE).sum()), segments_collision=int((status == COLLISION).sum()),
                 segments_unknown=int((status == UNKNOWN).sum()), segments_invalid=int((status == INVALID).sum()), samples=samples)
    return dict(status=status, t_stop=t_stop, min_clearance=min_c, t_min=t_min, stats=stats)


def store_of(g):
    """The model's view of the ESDF an integrator has stored (through block_indices() and esdf_blocks())."""
    idx = g.block_indices()
    return Store(idx, g.esdf_blocks(idx), g.vps)


def assert_same(got, want, what="", keys=None):
    """Every array as bit patterns (NaN equals NaN), and the statistics."""
    for k in (keys or [k for k in want if k != "stats"]):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            n = len(a.reshape(-1)) // max(1, int(np.prod(a.shape[a.ndim - (1 if k == "gradient" else 0):])))
            rows_a, rows_b = a.reshape(n, -1), b.reshape(n, -1)
            bad = np.nonzero((rows_a.view(np.uint8) != rows_b.view(np.uint8)).any(axis=1))[0]
            raise AssertionError("%s: %s differs at %d of %d elements, first %d: %r vs %r" % (what, k, len(bad), n, bad[0], rows_a[bad[0]], rows_b[bad[0]]))
    if got.get("stats") is not None:
        assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
