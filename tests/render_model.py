"""The yardstick of the view-rendering tests: a NumPy restatement of the contract (DESIGN.md, section "View rendering"),
written from the contract and not from the kernel.  Operands are np.float32 throughout (IEEE single, no fused operations);
all pixels march together, one sample per round for those still on their way.

    render_from_blocks(idx, tsdf, sem, vps, voxel_size, T_G_C, K, w, h, cfg) -> dict(depth, labels, rgba, normals, stats, ...)

takes host-layout blocks as HipIntegrator.download() returns them.  A voxel of a block that is absent, or of a tile inside a
downloaded block that is not resident, has weight 0 there and is never valid, since min_weight > 0: "belongs to a resident
tile and has weight >= min_weight" needs no tile list.  Beyond the contract's outputs the dict carries r_hit, p_hit and the
hit mask, for the tests of the yardstick itself."""
import numpy as np

F = np.float32
LIM = F((1 << 20) - 1)          # the packed range of voxel indices, as ks_esdf_query
EPS = F(1e-6)                   # grid_coord
DEFAULT_CFG = dict(min_weight=1e-4, min_range_m=0.1, max_range_m=10.0)


class Dense:
    """The downloaded blocks as dense [z, y, x] arrays over their bounding box (weight 0 where no block is)."""

    def __init__(self, idx, tsdf, sem, vps):
        idx = np.asarray(idx, np.int64).reshape(-1, 3)
        self.vps = vps
        lo = idx.min(axis=0) if len(idx) else np.zeros(3, np.int64)
        hi = idx.max(axis=0) + 1 if len(idx) else np.ones(3, np.int64)
        self.org = lo * vps                                   # first voxel of the box (x, y, z)
        n = (hi - lo) * vps
        self.shape = (int(n[2]), int(n[1]), int(n[0]))
        self.dist, self.wgt = np.zeros(self.shape, F), np.zeros(self.shape, F)
        self.rgba, self.label = np.zeros(self.shape, "<u4"), np.zeros(self.shape, np.uint8)
        for j in range(len(idx)):
            x, y, z = (idx[j] - lo) * vps
            sl = (slice(z, z + vps), slice(y, y + vps), slice(x, x + vps))
            self.dist[sl] = tsdf["distance"][j].reshape(vps, vps, vps)
            self.wgt[sl] = tsdf["weight"][j].reshape(vps, vps, vps)
            self.rgba[sl] = np.ascontiguousarray(tsdf["color"][j]).view("<u4").reshape(vps, vps, vps)
            self.label[sl] = sem["label"][j].reshape(vps, vps, vps)

    def inside(self, v):
        """v: (n, 3) int64 voxel indices -> (mask, z, y, x) with clipped local coordinates."""
        l = v - self.org
        ok = ((l >= 0) & (l < np.array(self.shape[::-1]))).all(axis=1)
        l = np.clip(l, 0, np.array(self.shape[::-1]) - 1)
        return ok, l[:, 2], l[:, 1], l[:, 0]


def sample(D, p, inv, mw):
    """S(p) for points p (n, 3) f32 -> (valid (n,), value (n,) f32)."""
    with np.errstate(invalid="ignore", over="ignore"):
        g = p * inv - F(0.5)
        i = np.floor(g)
        f = g - i
        ok = ((np.abs(i) < LIM) & (np.abs(i + F(1)) < LIM)).all(axis=1)
    assert g.dtype == F and f.dtype == F
    # a corner outside the box of the blocks is in no block: all eight lie inside when the lowest one does, one short of the end
    l = np.where(ok[:, None], i, F(0)).astype(np.int64) - D.org
    nz, ny, nx = D.shape
    ok &= ((l >= 0) & (l < np.array([nx - 1, ny - 1, nz - 1]))).all(axis=1)
    flat = np.where(ok, (l[:, 2] * ny + l[:, 1]) * nx + l[:, 0], 0)
    dist, wgt = D.dist.reshape(-1), D.wgt.reshape(-1)
    d = []
    for k in range(8):
        at = flat + ((k & 1) + nx * (((k >> 1) & 1) + ny * (k >> 2)))
        with np.errstate(invalid="ignore"):
            ok &= wgt[at] >= mw
        d.append(dist[at])
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        a0, a1 = d[0] + fx * (d[1] - d[0]), d[2] + fx * (d[3] - d[2])
        a2, a3 = d[4] + fx * (d[5] - d[4]), d[6] + fx * (d[7] - d[6])
        b0, b1 = a0 + fy * (a1 - a0), a2 + fy * (a3 - a2)
        s = b0 + fz * (b1 - b0)
    assert s.dtype == F
    return ok, s


def rotate(T, p):
    """The rotation of transform_point (Eigen's quaternion _transformVector) of rows p (n, 3) f32 by T_G_C = (w, x, y, z, t)."""
    w, v = F(T[0]), [F(T[1]), F(T[2]), F(T[3])]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    pc = [p[:, 0], p[:, 1], p[:, 2]]
    uv = cross(v, pc)
    uv = [c + c for c in uv]
    c2 = cross(v, uv)
    out = np.stack([(pc[k] + w * uv[k]) + c2[k] for k in range(3)], axis=1)
    assert out.dtype == F
    return out


def render_from_blocks(idx, tsdf, sem, vps, voxel_size, T_G_C, K, w, h, cfg=None, dense=None):
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    D = dense if dense is not None else Dense(idx, tsdf, sem, vps)
    vs, mw = F(voxel_size), F(cfg["min_weight"])
    inv = F(1.0 / np.float64(vs))                              # the context's voxel_size_inv
    rmin, rmax = F(cfg["min_range_m"]), F(cfg["max_range_m"])
    T = np.asarray(T_G_C, F)
    fx, fy, cx, cy = [F(v) for v in K]
    const_x, const_y = F(np.float64(1.0) / np.float64(fx)), F(np.float64(1.0) / np.float64(fy))
    n = w * h
    u = np.tile(np.arange(w, dtype=F), h)
    v = np.repeat(np.arange(h, dtype=F), w)
    dcx, dcy = (u - cx) * const_x, (v - cy) * const_y
    ln = np.sqrt((dcx * dcx + dcy * dcy) + F(1))
    uc = np.stack([dcx / ln, dcy / ln, F(1) / ln], axis=1)
    dg = rotate(T, uc)
    o = T[4:7]
    assert uc.dtype == F and dg.dtype == F
    point = lambda r, rows: o[None, :] + r[:, None] * dg[rows]

    r = np.full(n, rmin, F)
    r_prev, s_prev, r_hit = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
    prev_pos, hit = np.zeros(n, bool), np.zeros(n, bool)
    live = np.ones(n, bool)
    samples = 0
    while True:
        live &= ~(r > rmax)
        a = np.nonzero(live)[0]
        if len(a) == 0:
            break
        samples += len(a)
        valid, s = sample(D, point(r[a], a), inv, mw)
        with np.errstate(invalid="ignore", divide="ignore"):
            now = valid & (s <= F(0)) & prev_pos[a]
            rh = r_prev[a] + (r[a] - r_prev[a]) * (s_prev[a] / (s_prev[a] - s))
            pos = valid & (s > F(0))
        r_hit[a[now]] = rh[now]
        hit[a[now]] = True
        live[a[now]] = False
        go = ~now
        ag, pg, sg = a[go], pos[go], s[go]
        prev_pos[ag] = pg
        r_prev[ag[pg]] = r[ag[pg]]
        s_prev[ag[pg]] = sg[pg]
        with np.errstate(invalid="ignore"):
            step = np.where(pg, np.fmax(sg, vs), vs).astype(F)   # (fmaxf: the number when the other operand is NaN)
        r[ag] = r[ag] + step
    assert r.dtype == F and r_hit.dtype == F

    depth = np.full(n, np.nan, F)
    labels, rgba = np.full(n, 255, np.uint8), np.zeros(n, "<u4")
    normals = np.zeros((n, 3), F)
    p_hit = np.zeros((n, 3), F)
    a = np.nonzero(hit)[0]
    if len(a):
        ph = point(r_hit[a], a)
        p_hit[a] = ph
        depth[a] = r_hit[a] * uc[a, 2]
        gc = np.floor(ph * inv + EPS)
        ok = (np.abs(gc) < LIM).all(axis=1)
        ins, z, y, x = D.inside(np.where(ok[:, None], gc, F(0)).astype(np.int64))
        ok &= ins
        labels[a] = np.where(ok, D.label[z, y, x], 0)
        rgba[a] = np.where(ok, D.rgba[z, y, x], 0)
        g, good = [], np.ones(len(a), bool)
        for k in range(3):
            e = np.zeros(3, F)
            e[k] = vs
            vp_, sp = sample(D, ph + e, inv, mw)
            vm_, sm = sample(D, ph - e, inv, mw)
            good &= vp_ & vm_
            with np.errstate(invalid="ignore"):
                g.append(sp - sm)
        with np.errstate(invalid="ignore", divide="ignore"):
            n2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
            good &= n2 > F(0)
            nn = np.sqrt(n2)
            nrm = np.stack([g[0] / nn, g[1] / nn, g[2] / nn], axis=1)
        normals[a] = np.where(good[:, None], nrm, F(0))
    n_hit = int(hit.sum())
    return dict(depth=depth.reshape(h, w), labels=labels.reshape(h, w), rgba=rgba.view(np.uint8).reshape(h, w, 4),
                normals=normals.reshape(h, w, 3), stats=dict(pixels_hit=n_hit, pixels_missed=n - n_hit, samples=samples),
                hit=hit.reshape(h, w), r_hit=r_hit.reshape(h, w), p_hit=p_hit.reshape(h, w, 3))


def model_of(g, T_G_C, K, w, h, cfg=None):
    """The model's view of the map an integrator holds (through download())."""
    idx, t, s = g.download()
    return render_from_blocks(idx, t, s, g.vps, g.cfg.voxel_size, T_G_C, K, w, h, cfg)


def assert_same(got, model, what=""):
    """got = what HipIntegrator.render() returns.  All four images as bit patterns (NaN equals NaN) and the stats."""
    depth, labels, rgba, normals, stats = got
    for name, a in (("depth", depth), ("labels", labels), ("rgba", rgba), ("normals", normals)):
        b = model[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if np.ascontiguousarray(a).tobytes() != np.ascontiguousarray(b).tobytes():
            h, w = depth.shape
            bad = np.nonzero((a.reshape(h * w, -1).view(np.uint8) != b.reshape(h * w, -1).view(np.uint8)).any(axis=1))[0]
            raise AssertionError("%s: %s differs at %d of %d pixels, first (u, v) = (%d, %d): %r vs %r" % (
                what, name, len(bad), h * w, bad[0] % w, bad[0] // w, a.reshape(h * w, -1)[bad[0]], b.reshape(h * w, -1)[bad[0]]))
    assert stats == model["stats"], (what, stats, model["stats"])
