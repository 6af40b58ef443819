"""The yardstick of the path-shortening tests: a NumPy restatement of the contract (DESIGN.md, section "Path shortening"), written
from the contract and not from the kernel.  SW(a, b) is tests/esdf_read_model.py's sweep, imported and not copied; operands are
np.float32 throughout.

    shorten(store, waypoints, n_waypoints, voxel_size, **cfg) -> dict(status, n_waypoints, waypoints, length, min_clearance, stats, trace)

All paths search together: one round sweeps the current chunk of every path still on its way, in one call of the sweep.  `trace`
is per path the list of its greedy steps (a, j*, chunk, verified, nearer_blocked): what the tests assert the cases exercise."""
import numpy as np

from tests import esdf_read_model as E

F = E.F
INF = E.INF
OK, UNVERIFIED, INVALID = 0, 1, 2
DEFAULTS = dict(E.SWEEP_DEFAULTS, lookahead=64)
WAYPOINT_FILL = F(-7.0)          # what HipIntegrator.shorten_paths leaves in the rows the library does not write
STAT_KEYS = ("paths_ok", "paths_unverified", "paths_invalid", "waypoints_in", "waypoints_out", "segments_unverified", "sweeps", "samples")
CHUNK = 64


def length_of(a, b):
    """L(a, b): the length sweep rule 1 computes, f32 in the order written."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(b, F) - np.asarray(a, F)
        L = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    assert L.dtype == F
    return L


def valid_paths(wp, nw):
    mw = wp.shape[1]
    ok = (nw >= 1) & (nw <= mw)
    for i in np.nonzero(ok)[0]:
        ok[i] = np.isfinite(wp[i, :nw[i]]).all()
    return ok


def shorten(store, waypoints, n_waypoints, voxel_size, **cfg):
    c = dict(DEFAULTS, **cfg)
    look = int(c.pop("lookahead"))
    wp = np.ascontiguousarray(waypoints, F)
    nw = np.ascontiguousarray(n_waypoints, np.uint32).reshape(-1)
    n, mw = len(nw), wp.shape[1]
    assert wp.shape == (n, mw, 3) and 1 <= look <= 4096
    m = nw.astype(np.int64)
    valid = valid_paths(wp, nw)
    status = np.where(valid, OK, INVALID).astype(np.uint8)
    n_out = np.where(valid, 1, 0).astype(np.uint32)
    out = np.full((n, mw, 3), WAYPOINT_FILL, F)
    out[valid, 0] = wp[valid, 0]
    length, min_c = np.zeros(n, F), np.full(n, INF, F)
    a = np.zeros(n, np.int64)
    live = valid & (a < m - 1)
    top = np.where(live, np.minimum(a + look, m - 1), 0)
    chunk = np.zeros(n, np.int64)
    trace = [[] for _ in range(n)]
    sweeps = samples = unverified_segments = 0
    while live.any():
        at = np.nonzero(live)[0]
        lo = np.maximum(a[at] + 1, top[at] - (CHUNK - 1))
        counts = top[at] - lo + 1
        first = np.concatenate([[0], np.cumsum(counts)])
        path = np.repeat(at, counts)
        j = np.concatenate([np.arange(l, t + 1) for l, t in zip(lo, top[at])])
        seg = np.concatenate([wp[path, a[path]], wp[path, j]], axis=1)
        res = E.sweep(store, seg, voxel_size, **c)
        sweeps += len(seg)
        samples += res["stats"]["samples"]
        for k, i in enumerate(at):
            s = slice(first[k], first[k + 1])
            js, free = j[s], res["status"][s] == E.FREE
            if free.any():
                pick = int(np.nonzero(free)[0].max())
            elif js[0] == a[i] + 1:          # the last chunk: the input's own segment is kept
                pick = 0
                status[i] = UNVERIFIED
                unverified_segments += 1
            else:
                top[i] -= CHUNK
                chunk[i] += 1
                continue
            j_star = int(js[pick])
            trace[i].append((int(a[i]), j_star, int(chunk[i]), bool(free.any()), bool((~free[:pick]).any())))
            length[i] = length[i] + length_of(wp[i, a[i]], wp[i, j_star])
            mc = res["min_clearance"][s][pick]
            if mc < min_c[i]:
                min_c[i] = mc
            out[i, n_out[i]] = wp[i, j_star]
            n_out[i] += 1
            a[i] = j_star
            chunk[i] = 0
            if a[i] < m[i] - 1:
                top[i] = min(a[i] + look, m[i] - 1)
            else:
                live[i] = False
    assert length.dtype == F and min_c.dtype == F
    stats = dict(paths_ok=int((status == OK).sum()), paths_unverified=int((status == UNVERIFIED).sum()), paths_invalid=int((status == INVALID).sum()),
                 waypoints_in=int(m[valid].sum()), waypoints_out=int(n_out.sum()), segments_unverified=unverified_segments, sweeps=sweeps, samples=samples)
    return dict(status=status, n_waypoints=n_out, waypoints=out, length=length, min_clearance=min_c, stats=stats, trace=trace)


def model_of(g, waypoints, n_waypoints, **cfg):
    """The model's result on the ESDF an integrator has stored."""
    from tests import mesh_case
    return shorten(E.store_of(g), waypoints, n_waypoints, mesh_case.VOXEL, **cfg)


def assert_same(got, want, what="", in_place_of=None):
    """Every array the library returned as bit patterns, and the eight statistics.  in_place_of: the input array of an in-place call,
    whose rows from n_waypoints on the output keeps."""
    for k in ("status", "n_waypoints", "waypoints", "length", "min_clearance"):
        if k not in got:
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if k == "waypoints" and in_place_of is not None:
            rows = np.arange(b.shape[1])[None, :] < want["n_waypoints"][:, None]
            b = np.where(rows[:, :, None], b, np.ascontiguousarray(in_place_of, F))
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            ra, rb = a.reshape(len(a), -1), b.reshape(len(b), -1)
            bad = np.nonzero((ra.view(np.uint8) != rb.view(np.uint8)).any(axis=1))[0]
            raise AssertionError("%s: %s differs at %d of %d paths, first %d: %r vs %r" % (what, k, len(bad), len(a), bad[0], ra[bad[0]][:12], rb[bad[0]][:12]))
    if got.get("stats") is not None:
        assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
