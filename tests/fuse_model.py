"""NumPy yardstick of submap fusion (ks_fuse_map), written from the contract: points 1-5 restated operation by
operation, a brute force over EVERY destination voxel of the bounding box, with tests/merge_ref.merge_records for the fold.

    inverse_pose(T_D_S)                      -> T_S_D, (7,) f32: formed in f64, rounded at the end
    transform(T, c)                          -> transform_point of ks_device_math.h on rows c (n, 3) f32
    sample(S, p, inv, min_weight)            -> valid, d_a, w_a, flat index of the nearest corner
    fuse(dst, src, T_D_S, voxel_size, ...)   -> Result: the destination's blocks after the call, the touched voxels and tiles

Maps are host-layout blocks (idx, tsdf, sem, vps) as HipIntegrator.download() returns them.  A voxel of a block that is absent, or of
a tile inside a downloaded block that is not resident, has weight 0 there and is never valid, since min_weight > 0: "lies in a
resident source tile" needs no tile list.  A downloaded label never reads 255 (the host layout shows 0): that is the label the
incoming record carries."""
import numpy as np

from tests import merge_ref
from tests.render_model import rotate

F = np.float32
D = np.float64
LIM = F((1 << 20) - 1)          # the packed range of voxel indices
PRIOR_INIT = F(-0.60205999132)
GRAY = np.array([127, 127, 127, 255], np.uint8)


# ---- 1. the inverse pose --------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _rotate64(w, v, p):
    """(p + (2 w) (v x p)) + 2 (v x (v x p)), f64, in this form."""
    uv = _cross(v, p)
    c2 = _cross(v, uv)
    return [(p[k] + (D(2.0) * w) * uv[k]) + D(2.0) * c2[k] for k in range(3)]


def pose64(T_D_S):
    """The pose as the call reads it: the f32 numbers widened to f64, the quaternion normalised."""
    T = np.asarray(T_D_S, F).astype(D)
    n = np.sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2] + T[3] * T[3])
    return T[0] / n, [T[1] / n, T[2] / n, T[3] / n], [T[4], T[5], T[6]]


def inverse_pose(T_D_S):
    w, v, t = pose64(T_D_S)
    vi = [-v[0], -v[1], -v[2]]
    r = _rotate64(w, vi, t)
    return np.array([w, vi[0], vi[1], vi[2], -r[0], -r[1], -r[2]], D).astype(F)


# ---- 2. the point ---------------------------------------------------------------------------------------------------------------
def transform(T, c):
    T = np.asarray(T, F)
    out = rotate(T, c) + T[4:7][None, :]
    assert out.dtype == F
    return out


def centres(v, voxel_size):
    """c_k = ((float)v_k + 0.5f) * voxel_size for rows v (n, 3) of global voxel indices."""
    c = (v.astype(F) + F(0.5)) * F(voxel_size)
    assert c.dtype == F
    return c


# ---- dense maps -----------------------------------------------------------------------------------------------------------------
class Dense:
    """Blocks as dense [z, y, x] arrays over a block-aligned box (default voxels where no block is)."""

    def __init__(self, idx, tsdf, sem, vps, lo=None, hi=None):
        idx = np.asarray(idx, np.int64).reshape(-1, 3)
        self.vps = vps
        if lo is None:
            lo = idx.min(axis=0) if len(idx) else np.zeros(3, np.int64)
            hi = idx.max(axis=0) + 1 if len(idx) else np.ones(3, np.int64)
        self.blo, self.bhi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
        self.org = self.blo * vps
        n = (self.bhi - self.blo) * vps
        self.shape = (int(n[2]), int(n[1]), int(n[0]))
        self.dist, self.wgt = np.zeros(self.shape, F), np.zeros(self.shape, F)
        self.rgba, self.label = np.zeros(self.shape, "<u4"), np.zeros(self.shape, np.uint8)
        self.ref = np.full(self.shape, -1, np.int64)      # voxel -> row of self.rows (the 21 priors), -1: initial priors
        self.rows = np.ascontiguousarray(sem["priors"], F).reshape(-1, 21).copy() if len(idx) else np.zeros((0, 21), F)
        self.sem_rgba = np.full(self.shape, GRAY.view("<u4")[0], "<u4")
        for j in range(len(idx)):
            sl = self.block_slice(idx[j])
            shp = (vps, vps, vps)
            self.dist[sl] = tsdf["distance"][j].reshape(shp)
            self.wgt[sl] = tsdf["weight"][j].reshape(shp)
            self.rgba[sl] = np.ascontiguousarray(tsdf["color"][j]).view("<u4").reshape(shp)
            self.label[sl] = sem["label"][j].reshape(shp)
            self.ref[sl] = (j * vps ** 3 + np.arange(vps ** 3, dtype=np.int64)).reshape(shp)
            self.sem_rgba[sl] = np.ascontiguousarray(sem["color"][j]).view("<u4").reshape(shp)

    def block_slice(self, b):
        x, y, z = (np.asarray(b, np.int64) - self.blo) * self.vps
        v = self.vps
        return (slice(z, z + v), slice(y, y + v), slice(x, x + v))

    def priors_at(self, flat):
        """(n, 21) f32: the priors of the voxels at the flat indices."""
        r = self.ref.reshape(-1)[flat]
        out = np.full((len(flat), 21), PRIOR_INIT, F)
        out[r >= 0] = self.rows[r[r >= 0]]
        return out

    def set_priors(self, flat, values):
        r = self.ref.reshape(-1)
        new = r[flat] < 0
        first = len(self.rows)
        self.rows = np.concatenate([self.rows, np.zeros((int(new.sum()), 21), F)])
        r[flat[new]] = first + np.arange(int(new.sum()))
        self.rows[r[flat]] = values

    def blocks(self, idx):
        """Host-layout (tsdf, sem) of the blocks idx (n, 3), which lie inside the box."""
        from kimera_semantics_amd import binding as B
        idx = np.asarray(idx, np.int64).reshape(-1, 3)
        nv = self.vps ** 3
        t, s = np.zeros((len(idx), nv), B.TSDF_DTYPE), np.zeros((len(idx), nv), B.SEM_DTYPE)
        for j in range(len(idx)):
            sl = self.block_slice(idx[j])
            t["distance"][j] = self.dist[sl].reshape(nv)
            t["weight"][j] = self.wgt[sl].reshape(nv)
            t["color"][j] = np.ascontiguousarray(self.rgba[sl]).reshape(nv, 1).view(np.uint8)
            s["label"][j] = self.label[sl].reshape(nv)
            s["priors"][j] = self.priors_at(np.ravel_multi_index(tuple(np.mgrid[sl]), self.shape).reshape(-1))
            s["color"][j] = np.ascontiguousarray(self.sem_rgba[sl]).reshape(nv, 1).view(np.uint8)
        return t, s


# ---- 3. the sample --------------------------------------------------------------------------------------------------------------
def sample(S, p, inv, min_weight):
    """S(p) on the dense source S for points p (n, 3) f32 -> (valid, d_a, w_a, flat index of the nearest corner, corners (n, 8, 3))."""
    mw = F(min_weight)
    with np.errstate(invalid="ignore", over="ignore"):
        g = p * inv - F(0.5)
        i = np.floor(g)
        f = g - i
        ok = ((np.abs(i) < LIM) & (np.abs(i + F(1)) < LIM)).all(axis=1)
    assert g.dtype == F and f.dtype == F
    iv = np.where(ok[:, None], i, F(0)).astype(np.int64)
    l = iv - S.org
    nz, ny, nx = S.shape
    ok &= ((l >= 0) & (l < np.array([nx - 1, ny - 1, nz - 1]))).all(axis=1)   # all eight lie inside when the lowest does, one short of the end
    flat = np.where(ok, (l[:, 2] * ny + l[:, 1]) * nx + l[:, 0], 0)
    dist, wgt = S.dist.reshape(-1), S.wgt.reshape(-1)
    d, w, at = [], [], []
    for k in range(8):
        a = flat + ((k & 1) + nx * (((k >> 1) & 1) + ny * (k >> 2)))
        with np.errstate(invalid="ignore"):
            ok &= (wgt[a] >= mw) & ~np.isnan(dist[a])
        d.append(dist[a])
        w.append(wgt[a])
        at.append(a)
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]

    def lerp3(c):
        with np.errstate(invalid="ignore", over="ignore"):
            a0, a1 = c[0] + fx * (c[1] - c[0]), c[2] + fx * (c[3] - c[2])
            a2, a3 = c[4] + fx * (c[5] - c[4]), c[6] + fx * (c[7] - c[6])
            b0, b1 = a0 + fy * (a1 - a0), a2 + fy * (a3 - a2)
            out = b0 + fz * (b1 - b0)
        assert out.dtype == F
        return out

    nk = (fx >= F(0.5)).astype(np.int64) + 2 * (fy >= F(0.5)).astype(np.int64) + 4 * (fz >= F(0.5)).astype(np.int64)
    near = np.stack(at, axis=1)[np.arange(len(p)), nk]
    return ok, lerp3(d), lerp3(w), near, (iv, nk)


# ---- the colour of KS_COLOR_MODE_SEMANTIC_PROBABILITY (vxb::rainbowColorMap of exp(best prior), as k_merge_tiles ends) ----------------
def rainbow(best):
    h = np.exp(best.astype(D)).astype(F).astype(D)
    h = h - np.floor(h)
    h = h * 6
    i = np.floor(h).astype(np.int64)
    f = h - i
    f = np.where(i % 2 == 0, 1 - f, f)
    n = (255 * (1 - f)).astype(np.uint8).astype(np.uint32)
    v, m = np.uint32(255), np.uint32(0)
    zero = np.zeros_like(n)
    r = np.select([(i == 0) | (i == 6) | (i == 5), (i == 1) | (i == 4)], [zero + v, n], zero + m)
    g = np.select([(i == 1) | (i == 2), (i == 0) | (i == 6) | (i == 3)], [zero + v, n], zero + m)
    b = np.select([(i == 3) | (i == 4), (i == 2) | (i == 5)], [zero + v, n], zero + m)
    return (r | (g << 8) | (b << 16) | np.uint32(255 << 24)).astype("<u4")


# ---- 4 + 5. the incoming records and the fold --------------------------------------------------------------------------------------
class Result:
    pass


def _rows(a):
    return [tuple(int(v) for v in r) for r in np.asarray(a).reshape(-1, 3)]


def fuse(dst, src, T_D_S, voxel_size, min_weight=1e-4, color_mode=1, max_weight=10000.0, label_rgba=None):
    """dst, src: (idx, tsdf, sem, vps).  Returns a Result: idx (ascending), tsdf, sem — the destination's blocks after the call —,
    touched (n, vps^3) bool, tiles_touched (set of tile triples), tiles_before-independent block set, voxels_fused, T_S_D."""
    didx, dt, dsem, dvps = dst
    sidx, st, ssem, svps = src
    didx = np.asarray(didx, np.int64).reshape(-1, 3)
    sidx = np.asarray(sidx, np.int64).reshape(-1, 3)
    vs = F(voxel_size)
    inv = F(1.0 / D(vs))                                  # the context's voxel_size_inv
    T_S_D = inverse_pose(T_D_S)
    R = Result()
    R.T_S_D = T_S_D
    lut = np.ascontiguousarray(np.asarray(label_rgba, np.uint8).reshape(256, 4)).view("<u4")[:, 0]
    # the destination voxels that can be touched: the source box through T_D_S (f64), two voxels more on every side
    boxes = []
    if len(sidx):
        w, v, t = pose64(T_D_S)
        lo_m, hi_m = sidx.min(axis=0) * svps * D(vs), (sidx.max(axis=0) + 1) * svps * D(vs)
        pts = []
        for k in range(8):
            p = [D(hi_m[a]) if (k >> a) & 1 else D(lo_m[a]) for a in range(3)]
            r = _rotate64(w, v, p)
            pts.append([r[a] + t[a] for a in range(3)])
        pts = np.array(pts, D) / D(vs)
        lo_v, hi_v = np.floor(pts.min(axis=0)).astype(np.int64) - 2, np.ceil(pts.max(axis=0)).astype(np.int64) + 2
        boxes.append((lo_v // dvps, hi_v // dvps + 1))
    if len(didx):
        boxes.append((didx.min(axis=0), didx.max(axis=0) + 1))
    if not boxes:
        boxes.append((np.zeros(3, np.int64), np.ones(3, np.int64)))
    blo = np.min([b[0] for b in boxes], axis=0)
    bhi = np.max([b[1] for b in boxes], axis=0)
    Dd = Dense(didx, dt, dsem, dvps, blo, bhi)
    nz, ny, nx = Dd.shape
    touched = np.zeros(nz * ny * nx, bool)
    if len(sidx):
        S = Dense(sidx, st, ssem, svps)
        w_plane = ny * nx
        step = max(1, (1 << 18) // w_plane)
        for z0 in range(0, nz, step):
            z1 = min(nz, z0 + step)
            zz, yy, xx = np.meshgrid(np.arange(z0, z1), np.arange(ny), np.arange(nx), indexing="ij")
            base = z0 * w_plane
            v = np.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], axis=1).astype(np.int64) + Dd.org[None, :]
            p = transform(T_S_D, centres(v, vs))
            ok, d_a, w_a, near, _ = sample(S, p, inv, min_weight)
            a = np.nonzero(ok)[0]
            if not len(a):
                continue
            at = a + base
            touched[at] = True
            n = near[a]
            inc = np.zeros((len(a), 32), np.uint32)
            inc[:, 0], inc[:, 1] = d_a[a].view(np.uint32), w_a[a].view(np.uint32)
            inc[:, 2] = S.rgba.reshape(-1)[n]
            inc[:, 3] = S.label.reshape(-1)[n]            # (a download shows 255 as 0)
            inc[:, 4:25] = S.priors_at(n).view(np.uint32)
            rec = np.zeros((len(a), 32), np.uint32)
            rec[:, 0], rec[:, 1] = Dd.dist.reshape(-1)[at].view(np.uint32), Dd.wgt.reshape(-1)[at].view(np.uint32)
            rec[:, 2] = Dd.rgba.reshape(-1)[at]
            rec[:, 3] = Dd.label.reshape(-1)[at]
            rec[:, 4:25] = Dd.priors_at(at).view(np.uint32)
            merge_ref.merge_records(rec, inc, max_weight=max_weight, color_mode=color_mode, label_rgba=label_rgba)
            if color_mode == 2:
                rec[:, 2] = rainbow(rec[:, 4:25].view(F).max(axis=1))
            Dd.dist.reshape(-1)[at] = rec[:, 0].view(F)
            Dd.wgt.reshape(-1)[at] = rec[:, 1].view(F)
            Dd.rgba.reshape(-1)[at] = rec[:, 2]
            Dd.label.reshape(-1)[at] = rec[:, 3].astype(np.uint8)
            Dd.set_priors(at, rec[:, 4:25].view(F))
            Dd.sem_rgba.reshape(-1)[at] = lut[rec[:, 3]]
    tm = touched.reshape(Dd.shape)
    tz, ty, tx = np.nonzero(tm)
    gv = np.stack([tx, ty, tz], axis=1) + Dd.org[None, :]
    R.tiles_touched = {tuple(int(c) for c in r) for r in np.unique(gv >> 3, axis=0)} if len(gv) else set()
    new_blocks = {tuple(int(c) for c in r) for r in np.unique(gv // dvps, axis=0)} if len(gv) else set()
    R.idx = np.array(sorted(set(_rows(didx)) | new_blocks), np.int32).reshape(-1, 3)
    R.tsdf, R.sem = Dd.blocks(R.idx)
    R.touched = np.stack([tm[Dd.block_slice(b)].reshape(-1) for b in R.idx.astype(np.int64)]) if len(R.idx) else np.zeros((0, dvps ** 3), bool)
    R.voxels_fused = int(touched.sum())
    R.dense = Dd
    return R
