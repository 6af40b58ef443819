"""The yardstick of the view-information-gain tests: a NumPy restatement of the contract (DESIGN.md, section "View information
gain"), written from the contract and not from the kernels.  Operands are np.float32 throughout (IEEE single, no fused
operations); the rays of a view walk together, one sample per round for those still on their way, and the distinct voxels are the
unique rows of what they visited (no bitmap, no box).

    view_gain(store, poses, K, voxel_size, **cfg) -> (records (n,) RECORD_DTYPE, stats dict)

works over tests/esdf_read_model.Store and builds the rays by tests/render_model's ray rule.  The statistics that follow from the
sizing rule (workspace_bytes, views_in_lds) need what only the library knows (the store's tile count, the debug switches): they
are given by workspace_bytes() and by the `box_bits` of every view, which view_gain returns in stats["box_bits"]."""
import math

import numpy as np

from tests import esdf_read_model as E
from tests import render_model as R

F = np.float32
LIM = E.LIM
EPS = E.EPS
RECORD_DTYPE = np.dtype([(k, "<u4") for k in ("unknown_voxels", "free_voxels", "surface_voxels", "label_voxels", "rays_hit", "rays_open",
                                              "samples", "flags")])
COUNTERS = RECORD_DTYPE.names[:7]
DEFAULTS = dict(min_range_m=0.0, max_range_m=5.0, step_m=0.0, stop_distance_m=0.0, width=32, height=24, label=255)
LDS_BITS = 1 << 19          # the library's LDS budget (ks_k_view_gain.h), MAX_GROUPS its cap of workgroups in flight
MAX_GROUPS = 512
VALID = 1


def ray_directions(T, K, w, h):
    """dg (w * h, 3) f32 of the pixels (u, v), u fastest, by the renderer's rule (DESIGN.md §13.1 "Ray")."""
    fx, fy, cx, cy = [F(v) for v in K]
    const_x, const_y = F(np.float64(1.0) / np.float64(fx)), F(np.float64(1.0) / np.float64(fy))
    u = np.tile(np.arange(w, dtype=F), h)
    v = np.repeat(np.arange(h, dtype=F), w)
    with np.errstate(invalid="ignore", over="ignore"):
        dcx, dcy = (u - cx) * const_x, (v - cy) * const_y
        ln = np.sqrt((dcx * dcx + dcy * dcy) + F(1))
        uc = np.stack([dcx / ln, dcy / ln, F(1) / ln], axis=1)
        dg = R.rotate(np.asarray(T, F), uc)
    assert uc.dtype == F and dg.dtype == F
    return dg


def step_of(cfg, voxel_size):
    return F(cfg["step_m"]) if F(cfg["step_m"]) > 0 else F(voxel_size)


def n_samples(voxel_size, **cfg):
    c = dict(DEFAULTS, **cfg)
    return int(np.floor((F(c["max_range_m"]) - F(c["min_range_m"])) / step_of(c, voxel_size))) + 1


def ball_bits(max_range_m, voxel_size):
    side = 2 * math.ceil(float(F(max_range_m)) / float(F(voxel_size))) + 3
    return side ** 3


def workspace_bytes(n_tiles, n_views, max_range_m, voxel_size, groups=MAX_GROUPS, max_workspace_bytes=1 << 30):
    """The sizing rule: 256 B of bit planes per tile of the store, 96 B of counters, and per workgroup in flight
    one slab of the ball bound in bits, in steps of 256 B; the workgroups in flight are min(n, groups, what fits)."""
    slab = ((ball_bits(max_range_m, voxel_size) + 31) // 32 + 63) // 64 * 64 * 4
    fixed = n_tiles * 256 + 96
    in_flight = min(n_views, groups, (max_workspace_bytes - fixed) // slab)
    return fixed + in_flight * slab


def _coords(p, inv):
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor(p * inv + EPS)
    assert c.dtype == F
    return c


def one_view(store, T, K, voxel_size, c):
    """(record values (7,), box_bits) of a view whose pose is finite; box_bits -1: its rays leave the ball bound."""
    inv = E.inv_of(voxel_size)
    rmin, step, stop = F(c["min_range_m"]), step_of(c, voxel_size), F(c["stop_distance_m"])
    N = n_samples(voxel_size, **c)
    dg = ray_directions(T, K, c["width"], c["height"])
    o = np.asarray(T, F)[4:7]
    n = len(dg)

    def point(k, rows):
        t = rmin + F(k) * step
        with np.errstate(invalid="ignore", over="ignore"):
            p = o[None, :] + t * dg[rows]
        assert p.dtype == F
        return p

    # the box of the contract: the voxels of samples 0 and N - 1 of every ray that has a sample
    everyone = np.arange(n)
    p0, p1 = point(0, everyone), point(N - 1, everyone)
    c0, c1 = _coords(p0, inv), _coords(p1, inv)
    has = np.isfinite(p0).all(axis=1) & (np.abs(c0) < LIM).all(axis=1)
    bits = 0
    if has.any():
        last = F((1 << 20) - 2)
        c1 = np.clip(c1[has], -last, last)                       # (a coordinate beyond the packed range bounds at its last index)
        assert not np.isnan(c1).any()
        lo = np.minimum(c0[has], c1).min(axis=0).astype(np.int64)
        hi = np.maximum(c0[has], c1).max(axis=0).astype(np.int64)
        bits = int(np.prod(hi - lo + 1))
        if bits > ball_bits(c["max_range_m"], voxel_size):
            return None, -1
    # the walk
    live = np.ones(n, bool)
    hit = np.zeros(n, bool)
    samples = 0
    visited, state = [], []
    for k in range(N):
        rows = np.nonzero(live)[0]
        if len(rows) == 0:
            break
        p = point(k, rows)
        cc = _coords(p, inv)
        ok = np.isfinite(p).all(axis=1) & (np.abs(cc) < LIM).all(axis=1)
        live[rows[~ok]] = False                                  # the ray ends before this sample, OPEN
        rows, cc = rows[ok], cc[ok]
        v = cc.astype(np.int64)
        dist, flags, label = store.records(v)
        observed = (flags & 1) != 0
        with np.errstate(invalid="ignore"):
            occupied = observed & ~(dist > stop)
        samples += len(rows)
        visited.append(v)
        state.append(np.where(~observed, 0, np.where(~occupied, 1, 2 + (label == c["label"]) * (c["label"] != 255))))
        hit[rows[occupied]] = True
        live[rows[occupied]] = False
    counts = [0, 0, 0, 0]
    if visited:
        v, s = np.concatenate(visited), np.concatenate(state)
        if len(v):
            _, first = np.unique(v, axis=0, return_index=True)       # (the state belongs to the voxel: any visit gives it)
            s = s[first]
            counts = [int((s == 0).sum()), int((s == 1).sum()), int((s >= 2).sum()), int((s == 3).sum())]
            if bits:
                assert ((v >= lo) & (v <= hi)).all(), "a sample outside the box of samples 0 and N - 1"
    return counts + [int(hit.sum()), int(n - hit.sum()), samples], bits


def view_gain(store, poses, K, voxel_size, lds_bits=LDS_BITS, **cfg):
    c = dict(DEFAULTS, **cfg)
    T = np.ascontiguousarray(poses, F).reshape(-1, 7)
    rec = np.zeros(len(T), RECORD_DTYPE)
    box = []
    for j in range(len(T)):
        values, bits = one_view(store, T[j], K, voxel_size, c) if np.isfinite(T[j]).all() else (None, -1)
        box.append(bits)
        if values is not None:
            rec[j] = tuple(values) + (VALID,)
    valid = rec["flags"] == VALID
    stats = dict(views_valid=int(valid.sum()), views_invalid=int((~valid).sum()), views_in_lds=int(sum(1 for b in box if 1 <= b <= lds_bits)))
    for k in COUNTERS:
        stats[k] = int(rec[k].astype(np.int64).sum())
    stats["box_bits"] = box
    return rec, stats


def model_of(g, poses, K, lds_bits=LDS_BITS, **cfg):
    """The model on the ESDF an integrator has stored."""
    return view_gain(E.store_of(g), poses, K, g.cfg.voxel_size, lds_bits=lds_bits, **cfg)


def assert_same(got, want, what=""):
    """got: (records, stats) of the library; want: of the model.  Records byte for byte, the statistics the model can know."""
    rec, stats = got
    mrec, mstats = want
    assert rec.dtype == RECORD_DTYPE and rec.shape == mrec.shape, (what, rec.dtype, rec.shape, mrec.shape)
    if rec.tobytes() != mrec.tobytes():
        bad = [j for j in range(len(rec)) if rec[j] != mrec[j]]
        raise AssertionError("%s: %d of %d records differ, first %d: %r vs %r" % (what, len(bad), len(rec), bad[0], rec[bad[0]], mrec[bad[0]]))
    for k in mstats:
        if k != "box_bits":
            assert stats[k] == mstats[k], (what, k, stats[k], mstats[k])
