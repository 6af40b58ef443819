"""The yardstick of the scan-alignment tests: a NumPy restatement of the contract (DESIGN.md, section "Scan alignment"),
written from the contract and not from the kernels.  Per point the operands are np.float32 (IEEE single, no fused
operations); from the products on np.float64, the sums in the contract's tree (64-lane halving fold per wavefront, the
finisher's 256 strided accumulators and their halving fold), the LDL^T solve in the contract's order of operations.

    align_from_blocks(idx, tsdf, sem, vps, voxel_size, truncation, T_G_C, xyz, cfg) -> (T_out (7,) f32, stats dict, trace)

takes host-layout blocks as HipIntegrator.download() returns them (tests/render_model.py's Dense: a voxel outside every
resident tile has weight 0 there and is never valid).  `trace` holds the step of every iteration, for the tests of the
yardstick itself."""
import numpy as np

from tests import render_model as R

F, D = np.float32, np.float64
CONVERGED, ITERATION_LIMIT, TOO_FEW_INLIERS, DEGENERATE = 0, 1, 2, 3
DEFAULT_CFG = dict(min_weight=1e-4, max_residual_m=0.0, damping=1e-6, eps_rotation_rad=1e-4, eps_translation_m=1e-4,
                   max_iterations=10, point_stride=1, min_inliers=64, dof_mask=0x3f)
PIVOT_REL = D(2.0) ** -40
N_SUMS = 30     # 21 J_a J_b | 6 J_a r | r r | inliers | used points


def corners(Dn, p, inv, mw):
    """The eight corners of S(p) for points p (n, 3) f32 -> (valid (n,), [d0 .. d7] f32, f (n, 3) f32)."""
    with np.errstate(invalid="ignore", over="ignore"):
        g = p * inv - F(0.5)
        i = np.floor(g)
        f = g - i
        ok = ((np.abs(i) < R.LIM) & (np.abs(i + F(1)) < R.LIM)).all(axis=1)
    assert g.dtype == F and f.dtype == F
    l = np.where(ok[:, None], i, F(0)).astype(np.int64) - Dn.org
    nz, ny, nx = Dn.shape
    ok &= ((l >= 0) & (l < np.array([nx - 1, ny - 1, nz - 1]))).all(axis=1)   # (else a corner lies in no block)
    flat = np.where(ok, (l[:, 2] * ny + l[:, 1]) * nx + l[:, 0], 0)
    dist, wgt = Dn.dist.reshape(-1), Dn.wgt.reshape(-1)
    d = []
    for k in range(8):
        at = flat + ((k & 1) + nx * (((k >> 1) & 1) + ny * (k >> 2)))
        with np.errstate(invalid="ignore"):
            ok &= (wgt[at] >= mw) & ~np.isnan(dist[at])
        d.append(dist[at])
    return ok, d, f


def _lerp(a, b, f):
    return a + f * (b - a)


def rows_of(Dn, T, pc, inv, mw, max_res):
    """Finite camera-frame points pc (n, 3) f32 at pose T -> (inlier (n,), J (n, 6) f32, r (n,) f32); zeros where no inlier."""
    t = T[4:7]
    p = R.rotate(T, pc) + t[None, :]
    a = p - t[None, :]
    ok, d, f = corners(Dn, p, inv, mw)
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        s = _lerp(_lerp(_lerp(d[0], d[1], fx), _lerp(d[2], d[3], fx), fy), _lerp(_lerp(d[4], d[5], fx), _lerp(d[6], d[7], fx), fy), fz)
        gx = _lerp(_lerp(d[1] - d[0], d[3] - d[2], fy), _lerp(d[5] - d[4], d[7] - d[6], fy), fz) * inv
        gy = _lerp(_lerp(d[2] - d[0], d[3] - d[1], fx), _lerp(d[6] - d[4], d[7] - d[5], fx), fz) * inv
        gz = _lerp(_lerp(d[4] - d[0], d[5] - d[1], fx), _lerp(d[6] - d[2], d[7] - d[3], fx), fy) * inv
        g2 = (gx * gx + gy * gy) + gz * gz
        inl = ok & (np.abs(s) < max_res) & (g2 > F(0))
        cx, cy, cz = a[:, 1] * gz - a[:, 2] * gy, a[:, 2] * gx - a[:, 0] * gz, a[:, 0] * gy - a[:, 1] * gx
    J = np.stack([cx, cy, cz, gx, gy, gz], axis=1)
    assert J.dtype == F and s.dtype == F and p.dtype == F and a.dtype == F
    return inl, np.where(inl[:, None], J, F(0)), np.where(inl, s, F(0))


def evaluate(Dn, T, xyz, stride, inv, mw, max_res):
    """The 30 totals at pose T, through the wavefront partials and the finisher's tree."""
    n_used = (len(xyz) + stride - 1) // stride
    W = (n_used + 63) // 64
    pts = np.full((W * 64, 3), np.nan, F)
    pts[:n_used] = xyz[::stride]
    fin = np.isfinite(pts).all(axis=1)
    rows = np.nonzero(fin)[0]
    J, r, inl = np.zeros((W * 64, 6), F), np.zeros(W * 64, F), np.zeros(W * 64, bool)
    if len(rows):
        inl[rows], J[rows], r[rows] = rows_of(Dn, T, pts[rows], inv, mw, max_res)
    Jd, rd = J.astype(D), r.astype(D)
    terms = np.zeros((W * 64, N_SUMS), D)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            terms[:, k] = Jd[:, a] * Jd[:, b]
            k += 1
    for a in range(6):
        terms[:, 21 + a] = Jd[:, a] * rd
    terms[:, 27] = rd * rd
    terms[:, 28] = inl
    terms[:, 29] = fin
    part = terms.reshape(W, 64, N_SUMS)
    for off in (32, 16, 8, 4, 2, 1):
        part = part[:, :off] + part[:, off:2 * off]
    part = part.reshape(W, N_SUMS)
    acc = np.zeros((256, N_SUMS), D)
    for base in range(0, W, 256):
        c = part[base:base + 256]
        acc[:len(c)] = acc[:len(c)] + c
    for off in (128, 64, 32, 16, 8, 4, 2, 1):
        acc = acc[:off] + acc[off:2 * off]
    return acc[0]


def solve(tot, dof_mask, damping):
    """delta = -(H + damping * count)^-1 b by LDL^T in the contract's order, or None at a pivot that is not above 2^-40 of its diagonal entry."""
    H, b = np.zeros((6, 6), D), np.zeros(6, D)
    k = 0
    for a in range(6):
        for c in range(a, 6):
            H[a, c] = H[c, a] = tot[k]
            k += 1
    b[:] = tot[21:27]
    for a in range(6):
        if not (dof_mask >> a) & 1:
            H[a, :] = 0.0
            H[:, a] = 0.0
            H[a, a] = 1.0
            b[a] = 0.0
    lam = D(damping) * tot[28]
    for a in range(6):
        H[a, a] = H[a, a] + lam
    L, Dg, y, x = np.zeros((6, 6), D), np.zeros(6, D), np.zeros(6, D), np.zeros(6, D)
    with np.errstate(all="ignore"):
        for c in range(6):
            dj = H[c, c]
            for k in range(c):
                dj = dj - (L[c, k] * Dg[k]) * L[c, k]
            if not dj > PIVOT_REL * H[c, c]:
                return None
            Dg[c] = dj
            for i in range(c + 1, 6):
                v = H[i, c]
                for k in range(c):
                    v = v - (L[i, k] * Dg[k]) * L[c, k]
                L[i, c] = v / dj
        for i in range(6):
            v = b[i]
            for k in range(i):
                v = v - L[i, k] * y[k]
            y[i] = v
        for i in range(6):
            y[i] = y[i] / Dg[i]
        for i in range(5, -1, -1):
            v = y[i]
            for k in range(i + 1, 6):
                v = v - L[k, i] * x[k]
            x[i] = v
    return -x


def update(T, delta):
    """dq = (1, omega / 2) from the left, renormalised; t + v.  f32."""
    with np.errstate(all="ignore"):
        hx, hy, hz = F(delta[0]) / F(2), F(delta[1]) / F(2), F(delta[2]) / F(2)
        qw, qx, qy, qz = T[0], T[1], T[2], T[3]
        nw = ((qw - hx * qx) - hy * qy) - hz * qz
        nx = ((qx + hx * qw) + hy * qz) - hz * qy
        ny = ((qy - hx * qz) + hy * qw) + hz * qx
        nz = ((qz + hx * qy) - hy * qx) + hz * qw
        ln = np.sqrt(((nw * nw + nx * nx) + ny * ny) + nz * nz)
        out = np.array([nw / ln, nx / ln, ny / ln, nz / ln, T[4] + F(delta[3]), T[5] + F(delta[4]), T[6] + F(delta[5])])
    assert out.dtype == F
    return out


def align_from_blocks(idx, tsdf, sem, vps, voxel_size, truncation, T_G_C, xyz, cfg=None, dense=None):
    cfg = dict(DEFAULT_CFG, **{k: v for k, v in (cfg or {}).items() if v is not None})
    Dn = dense if dense is not None else R.Dense(idx, tsdf, sem, vps)
    inv = F(1.0 / D(F(voxel_size)))
    mw = F(cfg["min_weight"])
    max_res = F(cfg["max_residual_m"]) if F(cfg["max_residual_m"]) > 0 else F(truncation)
    er, et = D(F(cfg["eps_rotation_rad"])), D(F(cfg["eps_translation_m"]))
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    T = np.array(T_G_C, F)
    stride = int(cfg["point_stride"])
    ev = lambda pose: evaluate(Dn, pose, xyz, stride, inv, mw, max_res)
    status, iterations, first, steps = ITERATION_LIMIT, 0, None, []
    for it in range(int(cfg["max_iterations"])):
        tot = ev(T)
        if it == 0:
            first = tot
        if tot[28] < D(cfg["min_inliers"]):
            status = TOO_FEW_INLIERS
            break
        delta = solve(tot, int(cfg["dof_mask"]), F(cfg["damping"]))
        if delta is None:
            status = DEGENERATE
            break
        steps.append(delta)
        T = update(T, delta)
        iterations = it + 1
        if (delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2] <= er * er and \
                (delta[3] * delta[3] + delta[4] * delta[4]) + delta[5] * delta[5] <= et * et:
            status = CONVERGED
            break
    last = ev(T)
    rmse = lambda tot: float(np.sqrt(tot[27] / tot[28])) if tot[28] > 0 else 0.0
    stats = dict(status=status, iterations=iterations, points_used=int(first[29]), inliers_first=int(first[28]), inliers_last=int(last[28]),
                 rmse_first=rmse(first), rmse_last=rmse(last))
    return T, stats, dict(steps=steps, first=first, last=last)


def model_of(g, T_G_C, xyz, cfg=None):
    """The model's alignment against the map an integrator holds (through download())."""
    idx, t, s = g.download()
    return align_from_blocks(idx, t, s, g.vps, g.cfg.voxel_size, g.cfg.truncation_distance, T_G_C, xyz, cfg)


def assert_same(got, model, what=""):
    """got = what HipIntegrator.align() returns: the pose as bit patterns and every stats field (the two rmse as bit patterns)."""
    T, st = got
    assert T.dtype == F and T.tobytes() == model[0].tobytes(), (what, T, model[0], st, model[1])
    assert set(st) == set(model[1]), (what, st, model[1])
    for k, v in model[1].items():
        same = D(st[k]).tobytes() == D(v).tobytes() if k.startswith("rmse") else st[k] == v
        assert same, (what, k, st, model[1])
