"""The path-shortening cases (ks_path_shorten; DESIGN.md, section "Path shortening"), shared by both tiers like those of
tests/nav_case.py: the GPU tier (tests/test_path_shorten_gpu.py) calls run_case in-process, the CPU tier
(tests/test_path_shorten_cpu.py) runs it as a child process on the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.path_shorten_case '<json spec>'
The checker is tests/path_shorten_model.py on the stored ESDF as the library hands it out; every comparison is byte for byte, the
eight statistics included.  The stores are the analytic ones of the ESDF-read and navigation cases (the open box, `sphere`, `holes`)
and a box with a wall and a gap; paths come from tests/nav_model.py or are written by hand.  No case stores a navigation field
unless it says so: the call needs none."""
import ctypes
import json
import os
import sys

import numpy as np

from tests import esdf_case, esdf_read_case, mesh_case, nav_case, objects_case
from tests import esdf_read_model as E
from tests import nav_model as NM
from tests import path_shorten_model as M

VOXEL = mesh_case.VOXEL
F = np.float32
FILL = M.WAYPOINT_FILL
LENGTHS = (1, 2, 64, 65, 66, 130)
LOOKAHEADS = (1, 63, 64, 65, 70, 128, 4096)
BOX_RADIUS = 0.3                 # the open box stores 0.4 m everywhere: a clearance of 0.1 m
SPHERE_RADIUS = 0.1
WALL_RADIUS = 0.15
WALL_X = (3, 4)                  # the wall's voxels: these x, y in -8..7, every z; the gap is y in 8..15
refused = esdf_read_case.refused


def B():
    from kimera_semantics_amd import binding
    return binding


def centres(vox):
    return ((np.asarray(vox, np.float64).reshape(-1, 3) + 0.5) * VOXEL).astype(F)


def pack(paths, mw=None):
    """A list of (m_i, 3) polylines -> (waypoints (n, mw, 3) with FILL behind each path, n_waypoints)."""
    mw = mw or max(1, max(len(p) for p in paths))
    wp = np.full((len(paths), mw, 3), FILL, F)
    for i, p in enumerate(paths):
        wp[i, :len(p)] = np.asarray(p, F).reshape(-1, 3)[:mw]
    return wp, np.array([len(p) for p in paths], np.uint32)


def snake(x0, x1, y0, z, m):
    """m voxels in walking order: rows along x at y0, y0 + 1, ..., linked at alternating ends (a 5 cm staircase)."""
    out, y, xs = [], y0, list(range(x0, x1 + 1))
    while len(out) < m:
        out += [(x, y, z) for x in xs]
        xs.reverse()
        y += 1
    return out[:m]


def wall_voxels():
    free = {v: nav_case.FREE for v in nav_case.open_box_voxels()}
    for x in WALL_X:
        for y in range(-8, 8):
            for z in range(-8, 16):
                free[(x, y, z)] = (1, 1.0, 0.0)      # a site
    return free


def stored(kind, vps, **extra):
    if kind == "open_box":
        return nav_case._stored("open_box", vps, **extra)
    if kind == "wall":
        g = mesh_case._integrator(0, 64, 48, vps=vps, **extra)
        g.upload(*objects_case.voxel_field(wall_voxels(), vps))
        g.esdf_update(**nav_case.ECFG)
        return g
    return esdf_read_case._stored(dict(field=kind, vps=vps), **extra)


def check(g, wp, nw, what, store=None, **kw):
    """One host call against the model: (got, want)."""
    cfg = {k: v for k, v in kw.items() if k in M.DEFAULTS}
    want = M.shorten(store or E.store_of(g), wp, nw, VOXEL, **cfg)
    got = g.shorten_paths(wp, nw, **kw)
    M.assert_same(got, want, what, in_place_of=wp if kw.get("in_place") else None)
    return got, want


def summary(want):
    t = [s for tr in want["trace"] for s in tr]
    return dict(want["stats"], shortened=int((want["n_waypoints"] < want["n_in"]).sum()) if "n_in" in want else 0,
                late_chunk=sum(1 for s in t if s[2] > 0), nearer_blocked=sum(1 for s in t if s[3] and s[4]))


def merge(total, want, nw):
    want = dict(want, n_in=np.asarray(nw))
    for k, v in summary(want).items():
        total[k] = total.get(k, 0) + v
    return total


# ---- paths ---------------------------------------------------------------------------------------------------------------------
def grid_paths(kind):
    """The six lengths as prefixes of one staircase: through the open box (negative indices, the tile seams at 0 and 8), or across the
    cap of the sphere at z = 0.525 m."""
    if kind == "open_box":
        vox = snake(-7, 14, -3, 3, max(LENGTHS))
    else:
        vox = snake(-14, 14, -2, 10, max(LENGTHS))
    return pack([centres(vox[:m]) for m in LENGTHS])


def wall_paths(store):
    """Hand-written polylines on the wall store, then two paths of the navigation model round the wall's end."""
    left = lambda k, y=-4, z=3: (-6 + 0.5 * k, y, z)          # on the anchor's side, half a voxel apart
    behind = lambda k: (10, -6 + 0.1 * k, 3)                   # deep behind the wall
    paths = [
        # a far candidate is FREE and a nearer one is not: 0 -> 1 free, 2 behind the wall, 3 back on the anchor's side
        centres([(-6, -4, 3), (-5, -4, 3), (10, -4, 3), (-2, 2, 3)]),
        # j* is not in chunk 0: with lookahead 128 chunk 0 holds 17..80, all behind the wall, and chunk 1 the free 1..5
        centres([left(k) for k in range(6)] + [behind(k) for k in range(75)]),
        # repeated waypoints: L == 0, a single sample
        centres([(-6, 0, 3), (-6, 0, 3), (-5, 1, 3), (-5, 1, 3), (-5, 1, 3), (-2, 4, 5)]),
        # a staircase in the open half that collapses to its two ends
        centres(snake(-7, 0, 9, 5, 40)),
    ]
    fld = NM.field(store, centres([(-5, -4, 3)]), VOXEL, radius_m=WALL_RADIUS)
    starts = centres([(12, -4, 3), (11, 0, 8)])
    nav = NM.paths(fld, starts, 96)
    assert (nav["status"] == NM.REACHED).all(), nav["status"]
    wp, nw = pack(paths, 96)
    return np.concatenate([wp, nav["waypoints"]]), np.concatenate([nw, nav["n_waypoints"]]), fld


def many_paths():
    """300 staircases of 1..200 waypoints over the sphere store: rows of different lengths at different heights."""
    rng = np.random.default_rng(17)
    paths = []
    for i in range(300):
        m = 1 + (i * 199) // 299
        x0 = int(rng.integers(-14, -2))
        paths.append(centres(snake(x0, x0 + int(rng.integers(6, 16)), int(rng.integers(-14, 4)), int(rng.integers(-14, 15)), m)))
    assert {len(p) for p in paths} >= {1, 200}
    return pack(paths, 200)


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def case_grid(spec):
    kind, vps = spec["field"], spec["vps"]
    g = stored(kind, vps)
    store = E.store_of(g)
    wp, nw = grid_paths(kind)
    radius = BOX_RADIUS if kind == "open_box" else SPHERE_RADIUS
    total = {}
    for look in LOOKAHEADS:
        for free in ((0, 1) if kind == "holes" else (0,)):
            got, want = check(g, wp, nw, "%s lookahead %d unknown_is_free %d" % (kind, look, free), store, radius_m=radius, lookahead=look, unknown_is_free=free)
            merge(total, want, nw)
            if kind == "open_box":   # everything is free: the closed form and the identity
                assert (got["status"] == M.OK).all()
                if look == 1:
                    assert got["waypoints"].tobytes() == wp.tobytes() and (got["n_waypoints"] == nw).all()
                for i, m in enumerate(LENGTHS):
                    assert got["n_waypoints"][i] == (1 if m == 1 else 1 + -(-(m - 1) // look)), (look, m, got["n_waypoints"][i])
    g.close()
    return total


def case_wall(spec):
    g = stored("wall", spec["vps"])
    store = E.store_of(g)
    wp, nw, fld = wall_paths(store)
    total = {}
    got, want = check(g, wp, nw, "wall, lookahead 128", store, radius_m=WALL_RADIUS, lookahead=128)
    merge(total, want, nw)
    tr = want["trace"]
    assert want["status"][0] == M.OK and tr[0][0][:2] == (0, 3) and tr[0][0][4], tr[0]                 # 3 is free, 2 is not
    assert tr[1][0][:3] == (0, 5, 1) and want["status"][1] == M.UNVERIFIED, tr[1][:2]                     # found in chunk 1; the rest is behind the wall
    assert want["status"][2] == M.OK and want["n_waypoints"][2] == 2
    assert want["status"][3] == M.OK and want["n_waypoints"][3] == 2 and want["waypoints"][3, 1].tobytes() == wp[3, 39].tobytes()
    for i in (4, 5):                                                                                      # round the wall's end: a corner survives
        kept = want["waypoints"][i, :want["n_waypoints"][i]]
        assert want["status"][i] == M.OK and 3 <= want["n_waypoints"][i] < nw[i] / 3, (i, want["n_waypoints"][i], nw[i])
        assert (kept[1:-1, 1] > 7.5 * VOXEL).any(), kept
    for look in (1, 8, 64):
        merge(total, check(g, wp, nw, "wall, lookahead %d" % look, store, radius_m=WALL_RADIUS, lookahead=look)[1], nw)
    # with a navigation field stored, and the library's own paths: the same bytes
    goals, starts = centres([(-5, -4, 3)]), centres([(12, -4, 3), (11, 0, 8)])
    g.nav_update(goals, radius_m=WALL_RADIUS)
    nav = g.nav_paths(starts, 96)
    assert nav["waypoints"].tobytes() == wp[4:].tobytes() and (nav["n_waypoints"] == nw[4:]).all()
    again = g.shorten_paths(wp, nw, radius_m=WALL_RADIUS, lookahead=128)
    M.assert_same(again, want, "with a field stored")
    g.close()
    return total


def case_unknown(spec):
    """A candidate line through unobserved space: out of the open box and back in."""
    g = stored("open_box", spec["vps"])
    out = lambda k: (20 + k, 3, 3)
    paths = [centres([(0, 3, 3), (14, 3, 3)] + [out(k) for k in range(4)] + [(14, 5, 3), (0, 5, 3)]),
             centres([(0, 0, 0), (30, 0, 0), (30, 30, 0)])]
    wp, nw = pack(paths)
    _, strict = check(g, wp, nw, "unknown blocks", radius_m=BOX_RADIUS, unknown_is_free=0)
    _, loose = check(g, wp, nw, "unknown is free", radius_m=BOX_RADIUS, unknown_is_free=1)
    assert strict["status"][1] == M.UNVERIFIED and strict["stats"]["segments_unverified"] >= 2 and strict["n_waypoints"][1] == 3
    assert strict["status"][0] == M.OK and strict["n_waypoints"][0] == 2          # straight through the box from 0 to 7
    assert (loose["status"] == M.OK).all() and loose["n_waypoints"][1] == 2
    g.close()
    return dict(strict["stats"])


def case_radius(spec):
    """A radius equal to the distance the sweep reads at a waypoint, and one ulp above: the adjacent segment becomes unverified."""
    g = stored("sphere", spec["vps"])
    store = E.store_of(g)
    p = centres([(14, 5, -3)])
    e = E.sample(store, p, VOXEL)
    d0 = e["distance"][0]
    assert e["status"][0] != 0 and 0.12 < d0 < 0.38, e
    q = centres([(14, 6, -3)])
    assert E.sample(store, q, VOXEL)["distance"][0] > d0                              # the neighbour is farther from the sphere
    wp, nw = pack([np.concatenate([p, p]), np.concatenate([p, q])])
    _, equal = check(g, wp, nw, "radius equal", store, radius_m=float(d0))
    _, above = check(g, wp, nw, "radius one ulp above", store, radius_m=float(np.nextafter(d0, F(1))))
    assert (equal["status"] == M.OK).all() and equal["min_clearance"][0] == 0 and equal["length"][0] == 0
    assert (above["status"] == M.UNVERIFIED).all() and above["stats"]["segments_unverified"] == 2 and (above["min_clearance"] < 0).all()
    assert (above["n_waypoints"] == 2).all() and above["waypoints"].tobytes() == wp.tobytes()   # the input's own segments are kept
    g.close()
    return dict(above["stats"])


def case_too_long(spec):
    """Candidates longer than (max_samples - 2) * min_step: their sweeps are INVALID and count as not free."""
    g = stored("open_box", spec["vps"])
    wp, nw = pack([centres([(-7 + k, 2, 2) for k in range(20)]), centres([(-7 + 3 * k, 4, 4) for k in range(7)])])
    _, want = check(g, wp, nw, "max_samples 6", radius_m=BOX_RADIUS, max_samples=6, min_step_m=0.03)
    assert want["status"][0] == M.OK and [s[1] for s in want["trace"][0]] == list(range(2, 19, 2)) + [19]   # at most 0.12 m: two voxels at a time
    assert want["status"][1] == M.UNVERIFIED and want["n_waypoints"][1] == 7 and np.isinf(want["min_clearance"][1])   # 0.15 m apart: every sweep INVALID
    g.close()
    return dict(want["stats"])


def case_invalid(spec):
    g = stored("open_box", spec["vps"])
    line = centres([(-7 + k, 0, 0) for k in range(12)])
    paths = [line, line[:0], line, line.copy(), line.copy(), line[:5], line.copy()]
    paths[3][7, 1] = np.nan
    paths[4][11, 2] = np.inf
    paths[6][0, 0] = -np.inf
    wp, nw = pack(paths, 12)
    nw[2] = 13                                            # m > max_waypoints
    wp[5, 5:] = np.nan                                    # NaN in rows that are not used: ignored
    got, want = check(g, wp, nw, "invalid paths", radius_m=BOX_RADIUS)
    assert list(want["status"]) == [M.OK, M.INVALID, M.INVALID, M.INVALID, M.INVALID, M.OK, M.INVALID]
    bad = want["status"] == M.INVALID
    assert (got["waypoints"][bad] == FILL).all() and (got["n_waypoints"][bad] == 0).all() and (got["length"][bad] == 0).all()
    assert np.isinf(got["min_clearance"][bad]).all() and want["stats"]["waypoints_in"] == 17
    inp = g.shorten_paths(wp, nw, radius_m=BOX_RADIUS, in_place=True)
    M.assert_same(inp, want, "invalid paths in place", in_place_of=wp)   # their rows stay untouched
    g.close()
    return dict(want["stats"])


def case_many(spec):
    """300 paths of 1..200 waypoints in one call, with a grid of two workgroups (KS_SHORTEN_GRID): eight wavefronts take them in
    turn.  With `chunk` the host entry stages KS_SHORTEN_CHUNK paths at a time; the model knows neither."""
    assert os.environ.get("KS_DEBUG") == "1" and os.environ.get("KS_SHORTEN_GRID") == "2"
    chunk = spec.get("chunk")
    if chunk:
        assert int(os.environ.get("KS_SHORTEN_CHUNK", "0")) == chunk
    g = stored("sphere", spec["vps"])
    store = E.store_of(g)
    wp, nw = many_paths()
    assert not chunk or (len(nw) - 1) // chunk >= 2
    total = {}
    got, want = check(g, wp, nw, "300 paths", store, radius_m=SPHERE_RADIUS, lookahead=70)
    merge(total, want, nw)
    # each output alone, with and without statistics
    for name in ("status", "n_waypoints", "waypoints", "length", "min_clearance"):
        only = g.shorten_paths(wp, nw, outputs=(name,), stats=False, radius_m=SPHERE_RADIUS, lookahead=70)
        assert set(only) == {name, "stats"} and only["stats"] is None
        M.assert_same(only, want, "only " + name)
    for name in ("status", "n_waypoints", "waypoints", "length", "min_clearance"):
        rest = tuple(k for k in ("status", "n_waypoints", "waypoints", "length", "min_clearance") if k != name)
        M.assert_same(g.shorten_paths(wp, nw, outputs=rest, radius_m=SPHERE_RADIUS, lookahead=70), want, "all but " + name)
    # in place against out of place; a second call
    inp = g.shorten_paths(wp, nw, in_place=True, radius_m=SPHERE_RADIUS, lookahead=70)
    M.assert_same(inp, want, "in place", in_place_of=wp)
    M.assert_same(g.shorten_paths(wp, nw, radius_m=SPHERE_RADIUS, lookahead=70), got, "second call")
    one = g.shorten_paths(wp[299:], nw[299:], radius_m=SPHERE_RADIUS, lookahead=70)
    assert one["waypoints"].tobytes() == got["waypoints"][299:].tobytes() and one["length"][0] == got["length"][299]
    none = g.shorten_paths(np.zeros((0, 5, 3), F), np.zeros(0, np.uint32))
    assert none["stats"] == {k: 0 for k in M.STAT_KEYS} and none["waypoints"].shape == (0, 5, 3)
    g.close()
    return total


def case_snapshot(spec):
    """The store is read as it is: a block that joins later is unknown until a refresh, a removed block at once."""
    vps = spec["vps"]
    g = stored("sphere", vps)
    idx0 = g.block_indices()
    new = np.array([[int(idx0[:, 0].max()) + 1, 0, 0]], np.int32)               # beside the box, on its +x face
    v0 = new[0] * vps
    into = [centres([tuple(v0 + (-3, 2, 2)), tuple(v0 + (-2, 2, 2)), tuple(v0 + (2, 2, 2)), tuple(v0 + (4, 3, 2)), tuple(v0 + (5, 5, 3))])]
    into.append(centres(snake(-14, 14, -14, -12, 60)))
    wp, nw = pack(into)
    g.upload(*nav_case.field_blocks([tuple(v0 + (x, y, z)) for x in range(vps) for y in range(vps) for z in range(vps)], vps))
    _, before = check(g, wp, nw, "before the refresh", radius_m=0.05)
    assert before["status"][0] == M.UNVERIFIED                                  # the new block is not in the store yet
    g.esdf_refresh()
    _, after = check(g, wp, nw, "after the refresh", radius_m=0.05)
    assert after["status"][0] == M.OK and after["n_waypoints"][0] < 5
    gone = np.array([[-2, -2, -2]], np.int32) if vps == 8 else np.array([[-1, -1, -1]], np.int32)
    g.remove_blocks(gone)
    _, removed = check(g, wp, nw, "after the removal", radius_m=0.05)
    assert removed["stats"] != after["stats"]
    g.esdf_refresh()
    check(g, wp, nw, "refreshed after the removal", radius_m=0.05)
    g.close()
    return dict(after["stats"])


def case_reads_only(spec):
    vps = spec["vps"]
    wp, nw = grid_paths("sphere")

    def prepared():
        g = stored("sphere", vps)
        g.mesh()
        g.objects()
        g.mesh_index()
        g.nav_update(np.array([[-0.7, -0.7, -0.7]], F), radius_m=0.1)
        g.frontiers()
        g.updated_block_indices(reset=True)
        g.upload(*esdf_case.random_field([(0, 0, 0)], vps, 91))       # written voxels: `updated`, `dirty`, both stale bits
        f = mesh_case._frames(1, 64, 48)[0]
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        return g

    def snapshot(g):
        idx, t, s = g.download()
        n, nr = ctypes.c_size_t(), ctypes.c_size_t()
        assert B().lib().ks_count_updated_voxels(g._h, ctypes.byref(n), ctypes.byref(nr)) == 0
        im = g.mesh_index(build=False)
        return dict(updated=g.updated_block_indices(reset=False).tobytes(), counted=(n.value, nr.value), idx=idx.tobytes(), tsdf=t.tobytes(),
                    sem=s.tobytes(), esdf=g.esdf_blocks(idx).tobytes(), objects=g.object_records().tobytes(), ids=g.object_ids(idx).tobytes(),
                    nav=g.nav_blocks(idx).tobytes(), frontiers=g.frontier_records().tobytes(),
                    mesh=im.blocks.tobytes(), index=(im.xyz.tobytes(), im.indices.tobytes(), im.object_ids.tobytes()))

    def followers(g):
        return dict(stale=g.esdf_refresh()["tiles_stale"], meshed=g.mesh(only_stale=True).stats["blocks_meshed"])

    g = prepared()
    before = snapshot(g)
    assert len(before["updated"]) > 0 and before["counted"][0] > 0
    g.shorten_paths(wp, nw, radius_m=SPHERE_RADIUS)
    g.shorten_paths(wp, nw, radius_m=SPHERE_RADIUS, in_place=True, lookahead=4096)
    after = snapshot(g)
    assert after == before, [k for k in before if before[k] != after[k]]
    with_calls = followers(g)
    g.close()
    g = prepared()                                                    # the same history without the calls
    without = followers(g)
    g.close()
    assert with_calls == without and with_calls["stale"] > 0 and with_calls["meshed"] > 0, (with_calls, without)
    return with_calls


def case_errors(spec):
    KS, L = B(), B().lib()
    g = mesh_case._integrator(0, 64, 48, vps=8)
    g.upload(*nav_case.field_blocks(nav_case.open_box_voxels(), 8))
    wp, nw = pack([centres([(-7 + k, 0, 0) for k in range(12)])] * 3)
    P = lambda a: a.ctypes.data
    s8, n32, out, f32 = np.zeros(3, np.uint8), np.zeros(3, np.uint32), np.zeros_like(wp), np.zeros(3, F)
    st = KS.KsPathShortenStats()
    calls = [lambda: g.shorten_paths(wp, nw), lambda: g.shorten_paths_device(8, 8, 1, 12, d_status=8)]
    for call in calls:                                                          # no stored ESDF (the device addresses are never used)
        assert "no ESDF is stored" in str(refused(KS.KS_ERR_INVALID_ARG, call))
    g.esdf_update(**nav_case.ECFG)
    idx = g.block_indices()
    before = g.esdf_blocks(idx).tobytes()
    cfg = g.path_shorten_config()
    assert ctypes.sizeof(cfg) == 32 and (cfg.radius_m, cfg.min_step_m, cfg.unknown_is_free, cfg.max_samples, cfg.lookahead) == (F(0.3), 0.0, 0, 4096, 64)
    assert L.ks_path_shorten_default_config(None) == KS.KS_ERR_INVALID_ARG
    for fn in (L.ks_path_shorten, L.ks_path_shorten_device):
        a = lambda **k: fn(k.get("ctx", g._h), k.get("wp", P(wp)), k.get("nw", P(nw)), k.get("n", 3), k.get("mw", 12), k.get("cfg", ctypes.byref(cfg)),
                           k.get("status", P(s8)), None, None, None, None, ctypes.byref(st))
        assert a(ctx=None) == KS.KS_ERR_INVALID_ARG and a(cfg=None) == KS.KS_ERR_INVALID_ARG
        assert a(wp=None) == KS.KS_ERR_INVALID_ARG and a(nw=None) == KS.KS_ERR_INVALID_ARG           # NULL input with n > 0
        assert a(status=None) == KS.KS_ERR_INVALID_ARG                                               # every output NULL
        assert a(n=1 << 32) == KS.KS_ERR_INVALID_ARG and a(n=1 << 40) == KS.KS_ERR_INVALID_ARG       # (refused before anything is read)
        for bad in (0, 65537, 0xffffffff):
            assert a(mw=bad) == KS.KS_ERR_INVALID_ARG
        assert a(n=0, wp=None, nw=None, status=None) == 0                                            # n = 0 looks at no pointer
    for bad in (0, 4097, 0xffffffff):
        refused(KS.KS_ERR_INVALID_ARG, lambda: g.shorten_paths(wp, nw, lookahead=bad))
        refused(KS.KS_ERR_INVALID_ARG, lambda: g.shorten_paths_device(8, 8, 1, 12, d_status=8, lookahead=bad))
    for name in ("radius_m", "min_step_m"):                                     # the sweep's argument rules
        for bad in (-0.1, float("nan"), float("inf"), float("-inf")):
            refused(KS.KS_ERR_INVALID_ARG, lambda: g.shorten_paths(wp, nw, **{name: bad}))
            refused(KS.KS_ERR_INVALID_ARG, lambda: g.shorten_paths_device(8, 8, 1, 12, d_status=8, **{name: bad}))
    for bad in (1, 0, -5, 65537):
        refused(KS.KS_ERR_INVALID_ARG, lambda: g.shorten_paths(wp, nw, max_samples=bad))
    for look, ms in ((1, 2), (4096, 65536)):
        check(g, wp, nw, "lookahead %d max_samples %d" % (look, ms), radius_m=BOX_RADIUS, lookahead=look, max_samples=ms)
    wide, nwide = pack([centres([(0, 0, 0), (5, 0, 0)])], 65536)
    check(g, wide, nwide, "max_waypoints 65536", radius_m=BOX_RADIUS)
    assert L.ks_path_shorten(g._h, P(wp), P(nw), 3, 12, ctypes.byref(cfg), None, P(n32), None, None, None, None) == 0   # stats may be NULL
    assert g.esdf_blocks(idx).tobytes() == before
    g.clear()
    for call in calls:
        refused(KS.KS_ERR_INVALID_ARG, call)                                    # clear() drops the stored ESDF
    g.close()
    # a marcher context of the exact multi-GPU mode holds no voxel data
    marcher, owner = (mesh_case._integrator(1, 64, 48) for _ in range(2))
    f = mesh_case._frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    for call in (lambda: marcher.shorten_paths(wp, nw), lambda: marcher.shorten_paths_device(8, 8, 1, 12, d_status=8)):
        refused(KS.KS_ERR_UNSUPPORTED, call)
    owner.esdf_update(**nav_case.ECFG)
    assert owner.shorten_paths(wp, nw)["stats"]["waypoints_in"] == 36            # (the owner holds the map)
    marcher.close()
    owner.close()
    # a context in a failed state (the pool is full: sticky until a clear)
    small = mesh_case._integrator(0, 64, 48, max_tiles=8)
    try:
        small.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        raise AssertionError("a frame fitted 8 tiles")
    except KS.KsError as e:
        assert e.code == KS.KS_ERR_POOL_FULL, e
    for call in (lambda: small.shorten_paths(wp, nw), lambda: small.shorten_paths_device(8, 8, 1, 12, d_status=8)):
        assert "failed state" in str(refused(KS.KS_ERR_INVALID_ARG, call))
    small.close()
    return {}


CASES = {"grid": case_grid, "wall": case_wall, "unknown": case_unknown, "radius": case_radius, "too_long": case_too_long, "invalid": case_invalid,
         "many": case_many, "snapshot": case_snapshot, "reads_only": case_reads_only, "errors": case_errors}

# name -> (spec, extra environment): the same cases in both tiers
_GRID = {"KS_DEBUG": "1", "KS_SHORTEN_GRID": "2"}
SPECS = {
    "grid_open_box_vps8": (dict(case="grid", field="open_box", vps=8), {}),
    "grid_open_box_vps16": (dict(case="grid", field="open_box", vps=16), {}),
    "grid_sphere_vps8": (dict(case="grid", field="sphere", vps=8), {}),
    "grid_holes_vps16": (dict(case="grid", field="holes", vps=16), {}),
    "wall_vps8": (dict(case="wall", vps=8), {}),
    "wall_vps16": (dict(case="wall", vps=16), {}),
    "unknown_vps8": (dict(case="unknown", vps=8), {}),
    "radius_vps8": (dict(case="radius", vps=8), {}),
    "too_long_vps16": (dict(case="too_long", vps=16), {}),
    "invalid_vps8": (dict(case="invalid", vps=8), {}),
    "many_vps8": (dict(case="many", vps=8), dict(_GRID)),
    "many_chunked_vps16": (dict(case="many", vps=16, chunk=37), dict(_GRID, KS_SHORTEN_CHUNK="37")),
    "snapshot_vps8": (dict(case="snapshot", vps=8), {}),
    "reads_only_vps8": (dict(case="reads_only", vps=8), {}),
    "errors": (dict(case="errors"), {}),
}


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("PATH_SHORTEN_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
