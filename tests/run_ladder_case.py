"""The voxel update at every run-length hand-over between its kernels (csrc/ks_k_apply.h), stated deliberately: hand-built clouds
through the public ABI, shared by both tiers — the GPU tier (tests/test_run_ladder_gpu.py) calls run_case in-process, the CPU tier
(tests/test_run_ladder_cpu.py) runs it as a child process on the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.run_ladder_case '<json spec>'

The pairs of a frame are sorted into per-voxel runs and a run's length decides which kernel replays it: 1 .. 32 k_apply / k_apply_runs,
33 .. 1024 k_apply_long (k_apply_long_lanes up to 256, classes with edges at 48 / 64 / 96 / 128 / 192 / 256 / 384 / 512 / 768), more than
1024 k_apply_xlong / the integer sums of ks_k_apply_xl.h.  Every edge is a compare against pairs[i + N] or a clamp at the end of the list.

The geometry is that of tests/xl_case.py: the sensor at the centre of a voxel, unrotated; a tilted Fibonacci shell of n points at 0.6 m;
`fast` without early-out.  Every point is a ray, every ray ends in the sensor's voxel: ONE run of exactly n updates, the longest of the
frame.  A spec (`kind`):
  ladder        one frame per length, each at a sensor position of its own (2.4 m apart: shell + truncation = 0.8 m, no voxel shared), all
                in one oracle and one context; the ladder twice (fresh voxels, then visited ones).  `merged` (method 1): n sites with one
                point each in distinct end voxels, the sensor voxel's run is the number of bundles; `mixed`: every fourth site a bundle
                of two points with different labels (the `deltas` path)
  bundles       `merged`, the bundle merge's own hand-over (k_bundles: at most 32 points, the long-bundle workgroups: more): end voxels
                holding exactly 1, 2, 31, 32, 33, 34, 63, 64, 65, 127, 128, 129 jittered points, random labels, per-point colours, twice
  batch         `fast`, pipeline_frames 8 / 16, the default tail: the frames of a batch share the sensor position, the voxel's run is the
                concatenation over the batch — combined lengths 32, 33, 1024, 1025; against the oracle and against KS_TAIL_BATCH=0
  single_tile   frames that touch ONE tile, the sensor in its voxel (7, 7, 7) (local index 511, the last of the sorted pair list): the
                run that ends the list (k_find_long's `i + long_min < n_pairs`, k_long_measure's clamp); `head_at`: the run's head
                on the last pair of a k_apply_runs tile of 1024 pairs (its halo); `head_mod` [64, 63]: on the last lane of a k_apply
                window of 64 pairs (the run is finished from global memory, up to the end of the list)
A route is the environment the context is created under (KS_DEBUG=1): which kernel takes which lengths (ROUTES).

Every case proves ON THE CPU, with the oracle's ray caster and statistics, that the input holds the lengths it is named after, before
the library's map is looked at; the comparison is compare_maps(exact=True) plus the bytes of every block, nothing left out, and a
failure names the length (the blocks around each sensor position are compared on their own after every pass)."""
import collections
import json
import os
import sys

import numpy as np

from tests.xl_case import CENTRE, TRUNC, VOXEL, F, compare, environment, fibonacci_sphere, make_cloud, rays_through, record

LADDER = [1, 2, 16, 17, 31, 32, 33, 34, 48, 49, 63, 64, 65, 96, 97, 127, 128, 129, 192, 193, 255, 256, 257, 384, 385, 512, 513, 768, 769,
          1023, 1024, 1025, 1279, 1280, 1281, 2049]
MERGED_LADDER = [31, 32, 33, 34, 64, 65, 256, 257, 1024, 1025]
EMU_LADDER = [31, 32, 33, 34, 256, 257, 1024, 1025]
XL_RUNS = [1025, 1279, 1280, 1281, 2049]                      # what the integer sums must walk in the second pass of `lanes_xl`
BUNDLE_SIZES = [1, 2, 31, 32, 33, 34, 63, 64, 65, 127, 128, 129]
BATCH_SUMS = {4: [[8, 8, 8, 8], [8, 8, 8, 9], [256, 256, 256, 256], [256, 256, 256, 257]],
              8: [[4] * 8, [4] * 7 + [5], [128] * 8, [128] * 7 + [129]]}
BATCH_TARGETS = [32, 33, 1024, 1025]
SINGLE_TILE = [20, 32, 33, 34, 48, 49, 64, 65, 97, 129]
WINDOW_EDGE = [6, 20, 31, 32, 33, 34, 65]                     # single tile, the run's head on lane 63 of a k_apply window
STEP = 2.4                                                    # between sensor positions: 48 voxels, three blocks, six tiles
LANES = {"KS_APPLY_RUNS": "1", "KS_LONG_LANES": "2"}
# route -> environment: what takes the runs of 1..32 / 33..256 / 257..1024 / more than 1024 updates
ROUTES = {
    "default": {},                                            # k_apply / k_apply_long / k_apply_long / k_apply_xlong
    "runs": {"KS_APPLY_RUNS": "1", "KS_LONG_LANES": "0"},     # k_apply_runs / k_apply_long / k_apply_long / k_apply_xlong
    "lanes": LANES,                                           # k_apply_runs / k_apply_long_lanes / k_apply_long / k_apply_xlong
    "one_list": {"KS_XLONG": "0"},                            # k_apply / k_apply_long for everything above 32
    "lanes_xl": dict(LANES, KS_XL_PARALLEL="2"),              # as lanes, the integer sums above 1024
}
KNOBS = ("KS_DEBUG", "KS_APPLY_RUNS", "KS_LONG_LANES", "KS_XLONG", "KS_XL_PARALLEL", "KS_TAIL_BATCH")
SINGLE_TILE_CFG = dict(start_voxel_subsampling_factor=4.0, min_ray_length_m=0.02)
SINGLE_TILE_SENSOR = [0.375, 0.375, 0.375]                    # the centre of voxel (7, 7, 7)


# ---- specs -----------------------------------------------------------------------------------------------------------------------
def ladder(route="default", method=0, cm=1, cw=1, lengths=None, second=None, pipeline=0, mixed=False):
    lengths = list(lengths or (MERGED_LADDER if method else LADDER))
    return dict(kind="ladder", route=route, method=method, cm=cm, cw=cw, lengths=lengths, second=lengths if second is None else list(second),
                pipeline=pipeline, mixed=mixed)


def name_of(sp):
    parts = [sp["kind"], "merged" if sp.get("method") else "fast", sp.get("route", "default"), "cm%d" % sp.get("cm", 1), "cw%d" % sp.get("cw", 1)]
    for k in ("pipeline", "mixed", "permute", "head_at", "head_mod"):
        if sp.get(k):
            parts.append("%s%s" % (k, "" if sp[k] is True else "_".join(map(str, sp[k])) if isinstance(sp[k], list) else sp[k]))
    return "-".join(parts)


def gpu_specs():
    out = [ladder(r, cm=cm, cw=cw) for r in ROUTES for cm in (1, 0) for cw in (1, 0)]
    out += [ladder(r, pipeline=2) for r in ("default", "lanes")]                     # frames in flight, each frame's tail on its own
    out += [ladder(r, method=1, cm=cm, cw=0) for r in ("default", "lanes") for cm in (1, 0)]
    out += [ladder(r, method=1, cw=0, lengths=[32, 33, 257, 1025], mixed=True) for r in ("default", "lanes")]
    out += [dict(kind="bundles", method=1, cm=cm, cw=0, permute=p) for cm in (1, 0) for p in (False, True)]
    out += [dict(kind="batch", method=0, cm=cm, cw=1, pipeline=p) for p in (8, 16) for cm in (1, 0)]
    out += [dict(kind="single_tile", method=0, route=r, cm=1, cw=1, lengths=SINGLE_TILE) for r in ("default", "lanes")]
    out += [dict(kind="single_tile", method=0, route=r, cm=1, cw=1, head_at=1023) for r in ("default", "runs", "lanes")]
    out += [dict(kind="single_tile", method=0, route=r, cm=1, cw=1, lengths=WINDOW_EDGE, head_mod=[64, 63]) for r in ("default", "one_list")]
    return {name_of(sp): sp for sp in out}


def emu_specs():
    """The CPU tier: a sub-ladder per route, one pass plus a second pass of 32 / 33 only."""
    out = [ladder(r, lengths=EMU_LADDER, second=[32, 33]) for r in ("default", "lanes", "one_list")]
    out += [ladder("default", method=1, cw=0, lengths=EMU_LADDER, second=[32, 33])]
    # (two whole ladders, the routes, colour mode and weights the sub-ladders leave out: some ten seconds each, side by side with the rest)
    out += [ladder("lanes_xl", cm=1, cw=0), ladder("runs", cm=0, cw=1)]
    out += [dict(kind="bundles", method=1, cm=1, cw=0, permute=False)]
    out += [dict(kind="batch", method=0, cm=1, cw=1, pipeline=8)]
    out += [dict(kind="single_tile", method=0, route=r, cm=1, cw=1, lengths=[20, 32, 33, 34, 65]) for r in ("default", "lanes")]
    out += [dict(kind="single_tile", method=0, route="lanes", cm=1, cw=1, head_at=1023)]
    out += [dict(kind="single_tile", method=0, route="default", cm=1, cw=1, lengths=WINDOW_EDGE, head_mod=[64, 63])]
    return {name_of(sp): sp for sp in out}


# ---- clouds and their preconditions (the oracle's ray caster and grid rule: no library) ----------------------------------------
def position(k):
    return [CENTRE[0] + STEP * (k % 6), CENTRE[1] + STEP * (k // 6), CENTRE[2]]


def voxel_of(p):
    """The oracle's grid_coord rule, floor(p * inv + 1e-6), in f32."""
    inv = F(1) / F(VOXEL)
    return np.floor(np.asarray(p, F) * inv + F(1e-6)).astype(np.int64)


def labels_for(n, shift=0):
    return (1 + (np.arange(n) * 7 + shift) % 19).astype(np.uint8)   # (1 .. 19: the order inside a run matters; 20 is a dynamic label)


def paint(labels, cm, seed):
    from kimera_semantics_amd import synth
    rgba = synth.default_label_colors()[labels].copy()
    if cm == 0:                                                        # the blend branch of every kernel: per-point colours
        rgba[:, :3] = np.random.default_rng(seed).integers(0, 255, size=(len(labels), 3), dtype=np.uint8)
    return rgba


def shell_cloud(n, turn=0.0):
    xyz, _, _ = make_cloud(dict(kind="shell", n=n), CENTRE)
    if turn:
        c, s = np.cos(turn), np.sin(turn)
        xyz = (xyz.astype(np.float64) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]).T).astype(F)
    return np.ascontiguousarray(xyz, F), labels_for(n)


def sites_cloud(n, sensor, mixed=False):
    """`merged`: n sites on the 0.6 m shell, each in an end voxel of its own — one point per site, or (mixed) every fourth site a bundle
    of two points with different labels.  (xyz in the camera frame, labels, bundles)."""
    s = np.asarray(sensor, np.float64)
    m = n
    while True:
        vox = np.unique(np.floor((fibonacci_sphere(m) * 0.6 + s) / VOXEL).astype(np.int64), axis=0)
        if len(vox) >= n:
            break
        m += max(1, n // 16)
    vox = vox[np.sort(np.random.default_rng(n).permutation(len(vox))[:n])]
    pts, labs = [], []
    for k, v in enumerate(vox):
        centre = (v + 0.5) * VOXEL
        pts.append(centre + np.array([0.008, -0.006, 0.004]) - s)
        labs.append(1 + (k * 7) % 19)
        if mixed and k % 4 == 1:
            pts.append(centre + np.array([-0.007, 0.009, -0.005]) - s)
            labs.append(1 + (k * 7 + 3) % 19)
    xyz = np.ascontiguousarray(np.array(pts), F)
    ends = voxel_of(xyz + np.asarray(sensor, F))
    assert len(np.unique(ends, axis=0)) == n, "precondition: %d sites in %d end voxels" % (n, len(np.unique(ends, axis=0)))
    return xyz, np.array(labs, np.uint8), n


def bundle_cloud(permute):
    """End voxels holding exactly BUNDLE_SIZES points, jittered inside the voxel; random labels; (xyz in the camera frame, labels)."""
    rng = np.random.default_rng(11)
    s = np.asarray(CENTRE, np.float64)
    centres = [(0.8, 0.3, 1.5), (-0.6, 0.2, 1.2), (0.1, -0.7, 2.0), (1.1, 1.0, 0.9), (-1.0, -0.5, 1.7), (0.4, 0.9, 2.6),
               (-0.3, -1.1, 1.4), (1.3, -0.4, 1.1), (-1.2, 0.8, 2.2), (0.6, -1.3, 1.8), (-0.8, 1.2, 1.0), (0.2, 0.4, 2.4)]
    parts = []
    for c, n in zip(centres, BUNDLE_SIZES):
        mid = (np.floor((np.asarray(c) + s) / VOXEL) + 0.5) * VOXEL
        parts.append(mid + rng.uniform(-0.4, 0.4, size=(n, 3)) * VOXEL - s)
    xyz = np.ascontiguousarray(np.concatenate(parts), F)
    labels = rng.integers(1, 20, size=len(xyz), dtype=np.uint8)
    if permute:
        order = rng.permutation(len(xyz))
        xyz, labels = np.ascontiguousarray(xyz[order]), labels[order]
    _, counts = np.unique(voxel_of(xyz + np.asarray(CENTRE, F)), axis=0, return_counts=True)
    assert sorted(counts.tolist()) == BUNDLE_SIZES, "precondition: points per end voxel %s" % sorted(counts.tolist())
    return xyz, labels


_CELLS = {}


def ray_cells(sensor, xyz, from_origin, key=None):
    """The voxels every ray updates, by the oracle's ray caster, as rays_through of tests/xl_case.py calls it."""
    from oracle import oracle_py as O
    if key is not None and key in _CELLS:
        return _CELLS[key]
    o32 = np.asarray(sensor, F)
    cells = [O.cast_ray(o32, (p + o32).astype(F), voxel_size_inv=float(F(1) / F(VOXEL)), truncation=TRUNC, cast_from_origin=from_origin, cap=256)
             for p in xyz]
    if key is not None:
        _CELLS[key] = cells
    return cells


def run_lengths(sensor, cells):
    """(updates of the sensor's voxel, the longest other run, histogram of the other runs' lengths) of one frame or one batch."""
    allc = np.concatenate(cells) if len(cells) else np.zeros((0, 3), np.int64)
    vox, counts = np.unique(allc, axis=0, return_counts=True)
    mine = (vox == voxel_of(sensor)).all(axis=1)
    others = counts[~mine]
    return int(counts[mine].sum()), int(others.max()) if len(others) else 0, collections.Counter(others.tolist())


def check_run(n, sensor, cells, what, log):
    mine, longest, hist = run_lengths(sensor, cells)
    log("%s: sensor voxel %d updates, longest other run %d, other runs by length %s" % (what, mine, longest, sorted(hist.items())))
    assert mine == n, "precondition: %s: the sensor voxel holds %d updates" % (what, mine)
    assert longest < max(n, 2), "precondition: %s: another voxel holds %d updates" % (what, longest)   # (n = 1: every voxel of the ray holds one)
    return hist


def ladder_frame(sp, k, n):
    """(sensor, xyz, rgba, labels, bundles) of the ladder's frame number k, a run of n."""
    sensor = position(k)
    if sp["method"] == 1:
        xyz, labels, _ = sites_cloud(n, sensor, sp.get("mixed", False))
    else:
        xyz, labels = shell_cloud(n)
    return sensor, xyz, paint(labels, sp["cm"], n), labels


def ladder_precondition(sp, log=print):
    """The lengths of the sensor voxels' runs, frame by frame, from the oracle's ray caster alone."""
    found = []
    for k, n in enumerate(sp["lengths"]):
        sensor, xyz, _, labels = ladder_frame(sp, k, n)
        if sp["method"] == 1:                     # one ray per bundle, from the sensor: to the site's (first) point
            first = np.concatenate([[True], (voxel_of(xyz[1:] + np.asarray(sensor, F)) != voxel_of(xyz[:-1] + np.asarray(sensor, F))).any(axis=1)])
            xyz = xyz[first]
        assert len(xyz) == n
        cells = ray_cells(sensor, xyz, sp["method"] == 1, key=("ladder", sp["method"], sp.get("mixed", False), k, n))
        check_run(n, sensor, cells, "run of %d" % n, log)
        found.append(n)
    assert found == sp["lengths"] and len(set(found)) == len(found)
    return found


def single_tile_candidates():
    """Points in the negative octant of the sensor at SINGLE_TILE_SENSOR, closer than 0.15 m (with the truncation distance: inside the
    tile), in start cells (1.25 cm) of their own; with the voxels each ray updates."""
    s32 = np.asarray(SINGLE_TILE_SENSOR, F)
    pts = np.concatenate([fibonacci_sphere(1600)[i::4] * r for i, r in enumerate((0.145, 0.13, 0.115, 0.1))])
    pts = np.ascontiguousarray(pts[(pts < -0.012).all(axis=1)], F)
    cell = np.floor((pts + s32) * (F(4.0) * (F(1) / F(VOXEL))) + F(1e-6)).astype(np.int64)
    _, firsts = np.unique(cell, axis=0, return_index=True)
    pts = pts[np.sort(firsts)]
    cells = ray_cells(SINGLE_TILE_SENSOR, pts, False, key=("single_tile",))
    inside = np.array([bool(((c >= 0) & (c <= 7)).all()) for c in cells])
    return pts[inside], [c for c, ok in zip(cells, inside) if ok]


def single_tile_frames(sp, log=print):
    """[(n, xyz, cells)]: the frames of a single_tile spec.  head_at: ONE frame whose rays update head_at voxels besides the sensor's, so
    that the sensor voxel's run — the last of the sorted list — begins at pair number head_at."""
    pts, cells = single_tile_candidates()
    log("single tile: %d candidate rays" % len(pts))
    others = [len(c) - 1 for c in cells]
    if sp.get("head_at"):                        # the fewest rays that update exactly head_at voxels besides the sensor's
        target = sp["head_at"]
        for n in range(-(-target // max(others)), len(pts) + 1):
            idx = subset_with_sum(others, n, sum(others) + 1, target)
            if idx:
                return [(n, pts[idx], [cells[i] for i in idx])]
        raise AssertionError("no subset of the rays updates exactly %d other voxels" % target)
    out = []
    for n in sp["lengths"]:
        if n > len(pts):
            continue
        if sp.get("head_mod"):                   # [m, r]: n rays whose sensor-voxel run begins at a pair number = r mod m
            idx = subset_with_sum(others, n, *sp["head_mod"])
            assert idx, "no %d rays whose run begins at a pair number = %d mod %d" % (n, sp["head_mod"][1], sp["head_mod"][0])
        else:
            idx = np.sort(np.random.default_rng(n).permutation(len(pts))[:n]).tolist()
        out.append((n, pts[idx], [cells[i] for i in idx]))
    return out


def subset_with_sum(w, n, m, r):
    """Indices of n of the weights w whose sum is r modulo m (the sum nearest to n times the mean weight that can be had), or None."""
    top = n * max(w)
    layers = [np.zeros((n + 1, top + 1), bool)]
    layers[0][0, 0] = True
    for wi in w:
        new = layers[-1].copy()
        new[1:, wi:] |= layers[-1][:-1, :top + 1 - wi]
        layers.append(new)
    sums = [s for s in np.nonzero(layers[-1][n])[0].tolist() if s % m == r]
    if not sums:
        return None
    s = min(sums, key=lambda x: abs(x - n * sum(w) / len(w)))
    pick, c = [], n
    for i in range(len(w), 0, -1):
        if not layers[i - 1][c, s]:
            pick.append(i - 1)
            c, s = c - 1, s - w[i - 1]
    assert c == 0 and s == 0 and len(pick) == n
    return sorted(pick)


def single_tile_precondition(sp, log=print):
    frames = single_tile_frames(sp, log)
    for n, xyz, cells in frames:
        check_run(n, SINGLE_TILE_SENSOR, cells, "single tile, run of %d" % n, log)
        allc = np.concatenate(cells)
        assert allc.min() >= 0 and allc.max() <= 7                       # one tile, the sensor's voxel (7, 7, 7) its local index 511
        assert (voxel_of(SINGLE_TILE_SENSOR) == 7).all()
        if sp.get("head_at"):
            assert len(allc) - n == sp["head_at"] and n > 32, (len(allc), n)
        if sp.get("head_mod"):
            assert (len(allc) - n) % sp["head_mod"][0] == sp["head_mod"][1], (len(allc), n)
    if not sp.get("head_at"):
        assert [n for n, _, _ in frames] == sp["lengths"]
        assert {32, 33, 34} <= {n for n, _, _ in frames}, [n for n, _, _ in frames]
    return frames


def batch_frames(sp):
    """[(batch, sensor, xyz, labels)]: per batch of nb frames one sensor position; every frame a shell of its own (turned about z)."""
    nb = 4 if sp["pipeline"] < 16 else 8
    out = []
    for b, sizes in enumerate(BATCH_SUMS[nb]):
        for j, n in enumerate(sizes):
            xyz, labels = shell_cloud(n, turn=0.37 * j)
            out.append((b, position(b), xyz, labels_for(n, shift=3 * j)))
    return nb, out


def batch_precondition(sp, log=print):
    nb, frames = batch_frames(sp)
    for b, target in enumerate(BATCH_TARGETS):
        mine = [f for f in frames if f[0] == b]
        assert len(mine) == nb and len({f[2].tobytes() for f in mine}) == nb          # all distinct clouds
        cells = [c for f in mine for c in ray_cells(f[1], f[2], False)]
        check_run(target, mine[0][1], cells, "batch %d, combined run of %d" % (b, target), log)
    return nb, frames


# ---- running a case --------------------------------------------------------------------------------------------------------------
def contexts(sp, env, pipeline=0, oracle=True, **extra):
    from kimera_semantics_amd import binding as B
    from oracle import oracle_py as O
    from tests.util import COMMON, NO_EARLY_OUT
    cfg = dict(COMMON, method=sp["method"], use_const_weight=sp["cw"], color_mode=sp["cm"], max_consecutive_ray_collisions=NO_EARLY_OUT)
    cfg.update(extra)
    o = O.Oracle(O.default_config(integrator_threads=1, **cfg)) if oracle else None
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        with environment(**env):
            g = B.HipIntegrator(B.default_config(max_tiles=1 << 14, max_points=1 << 12, pipeline_frames=pipeline, **cfg))
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    return o, g


def pose(sensor):
    return np.array([1, 0, 0, 0] + list(sensor), F)


def exact(o, g):
    """compare_maps(exact=True) and the bytes of every block (xl_case.assert_same_bytes): nothing left out, no tolerance."""
    return compare(dict(compare="exact"), o, g)


def same_blocks(o, g, idx, what, bad):
    _, ot, osem = o.download(idx)
    _, gt, gsem = g.download(idx)
    if not (ot.tobytes() == gt.tobytes() and osem.tobytes() == gsem.tobytes()):
        bad.append(what)


def compare_per_frame(sp, o, g, lengths, pass_no):
    """The blocks around every sensor position on their own: a failure names the length."""
    oi, gi = o.block_indices(), g.block_indices()
    assert {tuple(x) for x in oi.tolist()} == {tuple(x) for x in gi.tolist()}, "pass %d: the block sets differ" % pass_no
    frame_of = np.rint(oi[:, 0] / 3.0).astype(np.int64) + 6 * np.rint(oi[:, 1] / 3.0).astype(np.int64)   # (three blocks between positions)
    bad = []
    for k, n in enumerate(sp["lengths"]):
        if n in lengths:
            idx = oi[frame_of == k]
            assert len(idx), n
            same_blocks(o, g, idx, n, bad)
    if bad:
        v = voxel_of(position(sp["lengths"].index(bad[0])))
        raise AssertionError("pass %d, route %s: the map differs from the oracle's around the runs of %s updates; the sensor voxel of the run of %d: "
                             "oracle %s, library %s" % (pass_no, sp["route"], bad, bad[0], record(o, v), record(g, v)))


def run_ladder(sp, log):
    ladder_precondition(sp, log)
    o, g = contexts(sp, dict(ROUTES[sp["route"]], KS_DEBUG="1"), pipeline=sp["pipeline"])
    stats = [g.update_stats()]
    for pass_no, lengths in enumerate((sp["lengths"], sp["second"])):
        want = got = 0
        for k, n in enumerate(sp["lengths"]):
            if n not in lengths:
                continue
            sensor, xyz, rgba, labels = ladder_frame(sp, k, n)
            so = o.integrate(pose(sensor), xyz, rgba, labels)
            assert so.n_rays_cast == n, "precondition: the frame of %d casts %d rays" % (n, so.n_rays_cast)
            sg = g.integrate(pose(sensor), xyz, rgba, labels)
            want, got = want + so.n_rays_cast, got + sg.n_rays_cast
            if not sp["pipeline"]:
                assert (so.n_rays_cast, so.n_voxel_updates) == (sg.n_rays_cast, sg.n_voxel_updates), n
        got += g.flush().n_rays_cast
        assert want == got, (want, got)
        stats.append(g.update_stats())
        compare_per_frame(sp, o, g, lengths, pass_no)
    if sp["route"] == "lanes_xl":
        walked, serial = (stats[2][k] - stats[1][k] for k in ("walked", "serial"))
        n_xl = sum(n in XL_RUNS for n in sp["second"])
        log("update_stats %s" % stats)
        # (the integer sums refuse a context that blends colours — tests/xl_case.py: refuse_colour_blend — and hand its runs to k_apply_xlong)
        assert (walked if sp["cm"] else serial) >= n_xl == len(XL_RUNS), (stats, n_xl)
    rep = exact(o, g)
    return dict(voxels=rep["oracle_touched"], frames=len(sp["lengths"]) + len(sp["second"]))


def run_bundles(sp, log):
    xyz, labels = bundle_cloud(sp["permute"])
    rgba = paint(labels, 0, 5)                    # per-point colours in either colour mode
    o, g = contexts(sp, {"KS_DEBUG": "1"})
    for rep in range(2):
        so = o.integrate(pose(CENTRE), xyz, rgba, labels)
        sg = g.integrate(pose(CENTRE), xyz, rgba, labels)
        assert so.n_rays_cast == len(BUNDLE_SIZES), so.n_rays_cast
        assert (so.n_valid_points, so.n_rays_cast, so.n_voxel_updates) == (sg.n_valid_points, sg.n_rays_cast, sg.n_voxel_updates)
    rep = exact(o, g)
    return dict(voxels=rep["oracle_touched"])


def run_batch(sp, log):
    from tests.tail_batch_case import same_maps
    nb, frames = batch_precondition(sp, log)
    o, g1 = contexts(sp, {}, pipeline=sp["pipeline"])
    _, g0 = contexts(sp, {"KS_DEBUG": "1", "KS_TAIL_BATCH": "0"}, pipeline=sp["pipeline"], oracle=False)
    sums = [0] * len(BATCH_TARGETS)
    for b, sensor, xyz, labels in frames:
        rgba = paint(labels, sp["cm"], len(labels))
        sums[b] += o.integrate(pose(sensor), xyz, rgba, labels).n_rays_cast
        for g in (g1, g0):
            g.integrate(pose(sensor), xyz, rgba, labels)
    assert sums == BATCH_TARGETS, "precondition: the rays of the batches %s" % sums
    for g in (g1, g0):
        g.flush()
    st1, st0 = g1.tail_batch_stats(), g0.tail_batch_stats()
    log("tail_batch_stats %s, with the switch %s, pipeline %s" % (st1, st0, g1.pipeline_shape()))
    assert g1.pipeline_shape()["batch"] == nb, g1.pipeline_shape()
    assert (st1["batches"], st1["frames"], st1["per_frame_batches"]) == (len(BATCH_TARGETS), len(frames), 0), st1
    assert st0["batches"] == 0 and st0["frames"] == 0 and st0["pairs"] == 0, st0
    bad = []
    oi = o.block_indices()
    for b, target in enumerate(BATCH_TARGETS):
        for g, which in ((g1, "batched"), (g0, "frame by frame")):
            same_blocks(o, g, oi[np.rint(oi[:, 0] / 3.0).astype(np.int64) == b], "%d (%s)" % (target, which), bad)
    assert not bad, "the map differs from the oracle's around the combined runs of %s updates" % bad
    for g in (g1, g0):
        rep = exact(o, g)
    same_maps(g1, g0)
    return dict(voxels=rep["oracle_touched"], frames=len(frames))


def run_single_tile(sp, log):
    frames = single_tile_precondition(sp, log)
    o, g = contexts(sp, dict(ROUTES[sp["route"]], KS_DEBUG="1"), **SINGLE_TILE_CFG)
    block = np.zeros((1, 3), np.int32)
    bad = []
    for n, xyz, cells in frames:
        labels = labels_for(n)
        rgba = paint(labels, sp["cm"], n)
        so = o.integrate(pose(SINGLE_TILE_SENSOR), xyz, rgba, labels)
        assert so.n_rays_cast == n and so.n_voxel_updates == sum(len(c) for c in cells), (n, so.n_rays_cast, so.n_voxel_updates)
        sg = g.integrate(pose(SINGLE_TILE_SENSOR), xyz, rgba, labels)
        assert (so.n_rays_cast, so.n_voxel_updates) == (sg.n_rays_cast, sg.n_voxel_updates), n
        assert len(g.tile_keys()) == 1, "precondition: %d tiles" % len(g.tile_keys())
        same_blocks(o, g, block, n, bad)
    # (one block, frame after frame: the first length named is the one that went wrong)
    assert not bad, "route %s: the map differs from the oracle's from the run of %d updates that ends the pair list on (%s)" % (sp["route"], bad[0], bad)
    rep = exact(o, g)
    return dict(voxels=rep["oracle_touched"], lengths=[n for n, _, _ in frames])


def run_case(sp, log=print):
    return {"ladder": run_ladder, "bundles": run_bundles, "batch": run_batch, "single_tile": run_single_tile}[sp["kind"]](sp, log)


def main():
    sp = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this entry drives the functional model only"
    out = run_case(sp)
    print("RUN_LADDER_OK", json.dumps(out))


if __name__ == "__main__":
    main()
