"""The edges of the integer-sum voxel update (csrc/ks_k_apply_xl.h), stated deliberately: hand-built clouds through the public ABI,
shared by both tiers — the GPU tier (tests/test_xl_gpu.py) calls run_case in-process, the CPU tier (tests/test_xl_cpu.py) runs it as
a child process on the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.xl_case '<json spec>'
Every case creates its context under KS_DEBUG=1 KS_XL_PARALLEL=2 (the library takes this path by itself only from 2^23 pairs per
frame on), runs the oracle beside the library, proves ON THE CPU with tests/xl_model.py that the input holds the edge it is named
after (`require`), pins the path of every frame through the deltas of update_stats(), and ends in compare_maps(exact=True).

The geometry: the sensor at the centre of voxel (0, 0, 0), unrotated; a Fibonacci-sphere shell of n points, one label, constant
weights, `fast` without early-out.  Every point is a ray, every ray updates the sensor's voxel: ONE run of exactly n updates that
all carry the same increments ("uniform": the result and the chunk classification do not depend on the integration order, so
walked / serial / chunks / replayed must EQUAL the model's prediction).  In the other cases (`merged`, mixed labels, 1/z^2 weights)
the order matters: the path (walked / serial) and 0 < chunks - replayed are asserted, the observed numbers printed.

Out of scope, because not reachable at small size: more than kXlMaxRuns (4096) runs in a frame, and the run that ends the sorted
pair list (the order of the voxel slots is not controllable from the ABI)."""
import contextlib
import json
import os
import sys

import numpy as np

from tests import xl_model as M

F = np.float32
VOXEL = 0.05
TRUNC = 0.2
CENTRE = [0.025, 0.025, 0.025]
LABEL = 3
STAT_KEYS = ("walked", "serial", "chunks", "replayed")
ZERO = dict.fromkeys(STAT_KEYS, 0)


# ---- clouds ---------------------------------------------------------------------------------------------------------------------
def fibonacci_sphere(n):
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    # (tilted: no direction has a component of exactly zero — an axis-parallel ray is the ray caster's own edge case, not this file's)
    a, b = 0.3, 0.2
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    return d @ (rx @ ry).T


def make_cloud(c, sensor):
    """(xyz in the camera frame [n, 3] f32, labels [n] u8, info) — the camera is unrotated: point_G = point_C + sensor."""
    kind = c["kind"]
    info = {}
    if kind == "shell":
        n = c["n"]
        xyz = fibonacci_sphere(n) * c.get("r", 0.6)
        labels = np.full(n, c.get("label", LABEL), np.uint8)
        if c.get("close_at") is not None:        # one point closer than the truncation distance: in the middle of the cloud, or its last
            xyz[n - 1 if c.get("close_last") else n // 2] *= c["close_at"] / c.get("r", 0.6)
    elif kind == "cone":
        # a lattice of 3 cm in x and y (distinct start voxels of 2.5 cm), z in [0.5, 1.5] m: per-ray weights 1 / z^2 in [0.44, 4]
        m = c["side"]
        gx, gy = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
        x, y = (gx.ravel() - (m - 1) / 2) * 0.03, (gy.ravel() - (m - 1) / 2) * 0.03
        z = 0.5 + ((gx.ravel() * 37 + gy.ravel() * 11) % 101) / 100.0
        xyz = np.stack([x, y, z], axis=1)
        labels = np.full(len(xyz), LABEL, np.uint8)
        info["uw"] = (1.0 / (xyz[:, 2].astype(F) ** 2)).astype(F)
    elif kind == "clusters":
        # `sites` directions on a shell; each site's END VOXEL gets sizes[k % len] points near its centre (one bundle of `merged`)
        s = np.asarray(sensor, np.float64)
        pg = fibonacci_sphere(c["sites"]) * c.get("r", 0.6) + s
        vox = np.unique(np.floor(pg / VOXEL).astype(np.int64), axis=0)
        sizes, pts, labs, comp = c["sizes"], [], [], []
        off = np.array([[0, 0, 0], [0.008, -0.006, 0.004], [-0.007, 0.009, -0.005], [0.006, 0.007, 0.008], [-0.009, -0.008, 0.006]])
        for k, v in enumerate(vox):
            cnt = sizes[k % len(sizes)]
            centre = (v + 0.5) * VOXEL
            lab = [c.get("label", LABEL)] * cnt
            if c.get("mixed_every") and k % c["mixed_every"] == 1 and cnt >= 2:
                lab[1] = 5
                if cnt >= 4:
                    lab[3] = 7
            if c.get("zero_every") and k % c["zero_every"] == 2:
                lab[0] = 0
            for j in range(cnt):
                pts.append(centre + off[j] - s)
                labs.append(lab[j])
            comp.append(tuple(sorted(lab)))
        xyz, labels = np.array(pts), np.array(labs, np.uint8)
        info.update(bundles=len(vox), compositions=comp)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(xyz, F), labels, info


def log_pair(p):
    """(log p, log(1 - p)) as the ORACLE computes them."""
    from oracle import oracle_py as O
    L = O.log_likelihood(float(F(p)))
    return F(L[1, 1]), F(L[1, 2])


def tie_probability(tie_in_binade, lo=0.5005):
    return M.search_probability(lambda p: log_pair(p)[1], tie_in_binade, lo=lo)[0]


# ---- specs -----------------------------------------------------------------------------------------------------------------------
def shell(n, expect="model", **kw):
    return dict(cloud=dict(kind="shell", n=n, **kw), expect=expect)


def spec(steps, method=0, require=(), env=None, tracked=None, compare="exact", sensor=None, tie_binade=None, **cfg):
    return dict(steps=steps, method=method, cfg=cfg, require=[list(r) for r in require], env=env or {}, tracked=tracked, compare=compare,
                sensor=sensor or CENTRE, tie_binade=tie_binade)


def neg(v):
    return M.bits(F(v))


def refusal(edit=None, **cfg):
    """A primer, the edit of the sensor voxel's record in BOTH maps, a run of 1100: `accepts` must say no, the stats serial."""
    steps = [shell(1100)] + ([dict(upload=edit)] if edit else []) + [shell(1100)]
    return spec(steps, require=[(len(steps) - 1, "accepts", "==", False)], max_weight=cfg.pop("max_weight", 2.0), **cfg)


B2048_BELOW = M.bits(np.nextafter(F(-2048), F(0)))      # one ulp inside [1024, 2048): the first update leaves the binade
SPECS = {
    # ---- run-length edges, each after a priming frame (its own run of 1500 starts from a fresh voxel: refused at measure) ----
    "len_1024": spec([shell(1500), shell(1024)], require=[(1, "listed", "==", False)], max_weight=2.0),
    "len_1025": spec([shell(1500), shell(1025)], require=[(1, "chunks", "==", 5), (1, "last_chunk", "==", 1)], max_weight=2.0),
    "len_1280": spec([shell(1500), shell(1280)], require=[(1, "chunks", "==", 5), (1, "last_chunk", "==", 256)], max_weight=2.0),
    "len_1500": spec([shell(1500), shell(1500), shell(1500), shell(1500)], require=[(1, "chunks", "==", 6), (1, "last_chunk", "==", 220)], max_weight=2.0),
    # ---- ties: a probability whose log(1 - p) is a tie exactly in [2048, 4096) (biased exponent 138) ----
    "tie_walked": spec([shell(1500), shell(2000)], tie_binade=138, require=[(1, "tie_chunks", ">=", 2), (1, "handed_back", "==", False)], max_weight=2.0),
    "tie_handed_back": spec([shell(2990), shell(2900)], tie_binade=138,
                            require=[(1, "tie_chunks", ">=", 10), (1, "handed_back", "==", True)], max_weight=2.0),
    "tie_merged_bundles": spec([dict(cloud=dict(kind="clusters", sites=700, sizes=[1, 2, 4]), expect=None),
                                dict(cloud=dict(kind="clusters", sites=1500, sizes=[1, 2, 4], r=0.7), expect=dict(walked=1, serial=0))],
                               method=1, tie_binade=138, require=[(1, "bundle_ties", "==", True)], max_weight=2.0),
    # ---- binades ----
    "binades_nine_handed_back": spec([shell(12), shell(4000, r=0.9)], require=[(1, "binades_spanned", ">=", 9), (1, "handed_back", "==", True)], max_weight=2.0),
    "binades_seven_walked": spec([shell(100), shell(4000, r=0.9)], require=[(1, "binades_spanned", "<=", 7), (1, "binades_spanned", ">=", 4),
                                                                          (1, "handed_back", "==", False)], max_weight=2.0),
    "binade_left_on_first_update": spec([shell(700), dict(upload=dict(prior_bits={"5": B2048_BELOW})), shell(1100)],
                                        require=[(2, "chunk0_reasons", "has", "leaves_binade")], max_weight=2.0),
    "binade_exact_power_of_two": spec([shell(700), dict(upload=dict(prior_bits={"all": neg(-4096.0)})), shell(1100)],
                                      require=[(2, "chunk0_ok", "==", True), (2, "start_mantissa_min", "==", 0x800000)], max_weight=2.0),
    # ---- weight ----
    "weight_meets_clamp": spec([shell(1500), shell(1500), shell(1500)], require=[(1, "reasons", "has", "weight_meets_clamp"), (1, "handed_back", "==", False)],
                               max_weight=2000.0),
    # (the replay of a LATER chunk would clamp an overshoot away: here every chunk after the one that meets the clamp is carried)
    "weight_meets_clamp_late": spec([shell(700), shell(1100)], require=[(1, "clean_after_weight_clamp", "==", True), (1, "handed_back", "==", False)],
                                    max_weight=1500.0),
    "weight_at_clamp_from_start": spec([shell(1100), shell(1100)], require=[(1, "weight_at_clamp", "==", True)], max_weight=1.0),
    # (a cone: the voxel above the sensor's is crossed by nearly every ray as well — two listed runs, by the oracle's ray caster)
    "weight_below_clamp_inverse_square": spec([dict(cloud=dict(kind="cone", side=36), expect=None), dict(cloud=dict(kind="cone", side=36), expect=dict(walked=2, serial=0))],
                                              tracked=[[0, 0, 0], [0, 0, 1]],
                                              require=[(1, "weights_distinct", ">=", 64), (1, "weight_stays_below", "==", True), (1, "listed_runs", "==", 2)],
                                              max_weight=10000.0, use_const_weight=0),
    # ---- distance: one update at 0.15 m, closer than the truncation distance ----
    # in the middle of a run the updates after it bring the distance back to the clamp (the oracle's record says so); as the frame's last
    # update (a frame of fewer than 2048 points is integrated in index order) it leaves the distance off the clamp for the next frame
    "distance_leaves_clamp": spec([shell(1500), shell(1500, close_at=0.15), shell(1500, close_at=0.15, close_last=True), shell(1500)],
                                  require=[(1, "accepts", "==", True), (1, "saturating", "==", False), (2, "accepts", "==", True),
                                           (2, "saturating", "==", False), (3, "accepts", "==", False), (3, "saturating", "==", True)], max_weight=2.0),
    # ---- start states the shortcut must refuse ----
    "refuse_plus_zero": refusal(dict(prior_bits={"7": 0x00000000})),
    "refuse_positive": refusal(dict(prior_bits={"7": M.bits(F(3.5))})),
    "refuse_denormal": refusal(dict(prior_bits={"7": 0x80000001})),
    "refuse_minus_inf": dict(refusal(dict(prior_bits={"7": 0xFF800000})), compare="bytes"),
    "refuse_exponent_254": refusal(dict(prior_bits={"7": 0xFF000000})),
    "refuse_weight_zero": refusal(dict(weight_bits=0)),
    "refuse_weight_above_max": refusal(dict(weight_bits=M.bits(np.nextafter(F(2.0), F(3.0))))),
    "refuse_max_weight_1e30": refusal(max_weight=1e30),
    "refuse_distance_one_ulp_below": refusal(dict(distance_bits=M.bits(np.nextafter(F(TRUNC), F(0))))),
    "refuse_colour_blend": refusal(color_mode=0),
    # ---- merged, lanes that differ: bundles of 1..5 points, mixed labels (per-bundle delta vectors), points of label 0 ----
    "merged_lanes_weight_stays_below": spec([dict(cloud=dict(kind="clusters", sites=2600, sizes=[1, 2, 3, 4, 5], r=0.7, mixed_every=3, zero_every=5), expect=None),
                                      dict(cloud=dict(kind="clusters", sites=2600, sizes=[5, 3, 1, 4, 2], r=0.7, mixed_every=4, zero_every=7), expect=dict(walked=1, serial=0))],
                                     method=1, require=[(1, "bundle_kinds", ">=", 8), (1, "weight_total_vs_max", "==", "below")], max_weight=100000.0),
    "merged_lanes_weight_meets_clamp": spec([dict(cloud=dict(kind="clusters", sites=2600, sizes=[1, 2, 3, 4, 5], r=0.7, mixed_every=3, zero_every=5), expect=None),
                                      dict(cloud=dict(kind="clusters", sites=2600, sizes=[5, 3, 1, 4, 2], r=0.7, mixed_every=4, zero_every=7), expect=dict(walked=1, serial=0))],
                                     method=1, require=[(1, "bundle_kinds", ">=", 8), (1, "weight_total_vs_max", "==", "above")], max_weight=8000.0),
    "merged_lanes_probability_colours": spec([dict(cloud=dict(kind="clusters", sites=2600, sizes=[1, 2, 3, 4, 5], r=0.7, mixed_every=3, zero_every=5), expect=None),
                                              dict(cloud=dict(kind="clusters", sites=2600, sizes=[5, 3, 1, 4, 2], r=0.7, mixed_every=4, zero_every=7), expect=dict(walked=1, serial=0))],
                                             method=1, compare="probability_colours", require=[(1, "bundle_kinds", ">=", 8)], max_weight=2.0, color_mode=2),
    # ---- two runs in one frame: the sensor 1 mm inside the face x = 0 of its voxel, the face neighbour collects half the rays ----
    "two_runs_different_fates": spec([shell(3000), dict(upload=dict(prior_bits={"7": 0x00000000})), shell(3000)], sensor=[0.001, 0.025, 0.025],
                                     tracked=[[0, 0, 0], [-1, 0, 0]], require=[(2, "listed_runs", "==", 2), (2, "fates", "==", ["serial", "walked"])], max_weight=2.0),
    "two_runs_chunk_cap": spec([shell(3000), shell(3000)], sensor=[0.001, 0.025, 0.025], tracked=[[0, 0, 0], [-1, 0, 0]], env={"KS_XL_CAP_CHUNKS": "12"},
                               require=[(1, "listed_runs", "==", 2), (1, "fates", "==", ["walked", "walked"]), (1, "chunks_of_runs", "==", [12, 6])],
                               max_weight=2.0),
}
# the run-edge clouds in a row: what the device-only tests of the GPU tier send through frames in flight
SEQUENCE = spec([shell(1500), shell(1024), shell(1025), shell(1280), shell(1500), shell(1025)], max_weight=2.0)


# ---- running a case --------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def environment(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def contexts(sp, pipeline=0, env=None):
    from kimera_semantics_amd import binding as B
    from oracle import oracle_py as O
    from tests.util import COMMON, NO_EARLY_OUT
    cfg = dict(COMMON, method=sp["method"], use_const_weight=1, max_consecutive_ray_collisions=NO_EARLY_OUT)
    cfg.update(sp["cfg"])
    if sp.get("tie_binade"):
        cfg["semantic_measurement_probability"] = float(tie_probability(sp["tie_binade"]))
    o = O.Oracle(O.default_config(integrator_threads=1, **cfg))
    with environment(KS_DEBUG="1", KS_XL_PARALLEL="2", **dict(sp["env"], **(env or {}))):
        g = B.HipIntegrator(B.default_config(max_tiles=4096, max_points=1 << 14, pipeline_frames=pipeline, **cfg))
    return o, g, cfg


def voxel_address(v, vps):
    v = np.asarray(v, np.int64)
    b, l = v // vps, v % vps
    return b.astype(np.int32), int(l[0] + vps * (l[1] + vps * l[2]))


def record(ctx, v):
    """dict(distance, weight, priors) of voxel v in the oracle's (or the library's) map; None where the block is absent."""
    b, l = voxel_address(v, ctx.vps)
    if not any((b == x).all() for x in ctx.block_indices()):
        return None
    _, t, s = ctx.download(b.reshape(1, 3))
    return dict(distance=F(t["distance"][0, l]), weight=F(t["weight"][0, l]), priors=s["priors"][0, l].copy())


def apply_edit(o, g, edit):
    """The sensor voxel's record, edited, into BOTH maps through their upload calls."""
    b, l = voxel_address([0, 0, 0], o.vps)
    _, t, s = o.download(b.reshape(1, 3))
    for k, bits_ in (edit.get("prior_bits") or {}).items():
        cols = range(M.NUM_LABELS) if k == "all" else [int(k)]
        for c in cols:
            s["priors"][0, l, c] = M.from_bits(bits_)
    if "weight_bits" in edit:
        t["weight"][0, l] = M.from_bits(edit["weight_bits"])
    if "distance_bits" in edit:
        t["distance"][0, l] = M.from_bits(edit["distance_bits"])
    o.upload(b.reshape(1, 3), t, s)
    g.upload(b.reshape(1, 3), t, s)


def rays_through(sensor, xyz, v, from_origin):
    """Which rays update voxel v, by the oracle's ray caster (independent of the library); `fast` casts from the point, `merged` from the sensor."""
    from oracle import oracle_py as O
    o32 = np.asarray(sensor, F)
    hit = np.zeros(len(xyz), bool)
    for i, p in enumerate(xyz):
        cells = O.cast_ray(o32, (p + o32).astype(F), voxel_size_inv=float(F(1) / F(VOXEL)), truncation=TRUNC, cast_from_origin=from_origin, cap=256)
        hit[i] = (cells == np.asarray(v, np.int64)).all(axis=1).any()
    return hit


def uniform_run(sp, cfg, xyz, info, v, n_rays):
    """(increments [22, n], sdfs [n]) of the run of voxel v in a uniform frame."""
    lm, ln = log_pair(cfg["semantic_measurement_probability"])
    sensor = np.asarray(sp["sensor"], np.float64)
    hit = rays_through(sp["sensor"], xyz, v, sp["method"] == 1)
    if list(v) == [0, 0, 0]:
        assert hit.all()                                                  # every ray through the sensor's voxel: a run of exactly n updates
    d = xyz[hit].astype(np.float64)
    vo = (np.asarray(v, np.float64) + 0.5) * VOXEL - sensor
    sdf = np.linalg.norm(d, axis=1) - d @ vo / np.linalg.norm(d, axis=1)
    n = int(hit.sum())
    inc = np.empty((M.CHAINS, n), F)
    inc[:M.NUM_LABELS] = ln
    inc[LABEL] = lm
    inc[M.NUM_LABELS] = F(1)
    return inc, sdf


def facts_uniform(sp, cfg, step, xyz, info, recs, n_rays):
    """What the model says about a uniform frame: the prediction (summed over the tracked voxels) and the facts `require` asks for."""
    tracked = sp["tracked"] or [[0, 0, 0]]
    total, facts, fates, chunks_of = dict(ZERO), {}, [], []
    assert n_rays == len(xyz), (n_rays, len(xyz))                         # every point a ray: the run lengths are what the case says
    for v, rec in zip(tracked, recs):
        inc, sdf = uniform_run(sp, cfg, xyz, info, v, n_rays)
        n = inc.shape[1]
        if rec is None:                                                   # a voxel no frame has touched yet: distance 0, weight 0
            rec = dict(distance=F(0), weight=F(0), priors=np.full(M.NUM_LABELS, M.PRIOR_INIT, F))
        pred, R = M.predict(rec, inc, sdf, cfg.get("color_mode", 1), TRUNC, cfg["max_weight"])
        for k in STAT_KEYS:
            total[k] += pred[k]
        fates.append("walked" if pred["walked"] else "serial" if pred["serial"] else "short")
        chunks_of.append((n + M.CHUNK - 1) // M.CHUNK)
        if v == tracked[0]:
            acc = M.accepts(rec, cfg.get("color_mode", 1), TRUNC, cfg["max_weight"])
            facts.update(listed=n > M.LONG_RUN, accepts=acc, chunks=(n + M.CHUNK - 1) // M.CHUNK, last_chunk=n - (n - 1) // M.CHUNK * M.CHUNK,
                         saturating=bool((np.asarray(sdf) >= 2 * TRUNC).all()), weight_at_clamp=bool(rec["weight"] == F(cfg["max_weight"])),
                         start_mantissa_min=min(M.mantissa(p) for p in rec["priors"]))
            if R is not None:
                met = [b for b, why in enumerate(R.reasons) if "weight_meets_clamp" in why]
                facts.update(R.summary(), chunk0_reasons=R.reasons[0], chunk0_ok=R.ok[0], model_end=R.end,
                             clean_after_weight_clamp=bool(met) and met[0] + 1 < R.n_chunks and all(R.ok[met[0] + 1:]))
    facts.update(listed_runs=sum(c > 4 for c in chunks_of), fates=fates, chunks_of_runs=chunks_of)
    return total, facts


def facts_other(sp, cfg, xyz, info, rec0, rec1):
    """Facts about a frame whose increments depend on the order: from the cloud and the ORACLE's records before and after."""
    facts = {}
    if sp["tracked"]:
        facts["listed_runs"] = sum(int(rays_through(sp["sensor"], xyz, v, sp["method"] == 1).sum()) > M.LONG_RUN for v in sp["tracked"])
    if "uw" in info:
        facts["weights_distinct"] = len(np.unique(info["uw"]))
        facts["weight_stays_below"] = bool(float(rec0["weight"]) + float(info["uw"].astype(np.float64).sum()) * 1.001 < cfg["max_weight"])
    if "compositions" in info:
        facts["bundle_kinds"] = len(set(info["compositions"]))
        total = float(rec0["weight"]) + sum(len(c) for c in info["compositions"])
        facts["weight_total_vs_max"] = "below" if total * 1.001 < cfg["max_weight"] else "above" if total > 1.001 * cfg["max_weight"] and rec0["weight"] < F(cfg["max_weight"]) else "at"
        if sp.get("tie_binade"):
            # a pure bundle of c points adds c log(1 - p) to the other classes: a tie where the sum is in binade tie_binade(c log).  The
            # frame's sums (start and end from the oracle) must visit a binade where SOME bundle sizes tie, and start in one where none does.
            ln = log_pair(cfg["semantic_measurement_probability"])[1]
            ties_at = {M.tie_binade(F(c) * ln) for c in {len(x) for x in info["compositions"]}}
            e_start, e_end = M.exponent(rec0["priors"][1]), M.exponent(rec1["priors"][1])
            facts["bundle_ties"] = e_start not in ties_at and any(e_start < e <= e_end for e in ties_at) and len(ties_at) >= 3
            facts["tie_binades"] = sorted(ties_at), e_start, e_end
    return facts


def check_requirements(sp, frame, facts):
    ops = {"==": lambda a, b: a == b, ">=": lambda a, b: a >= b, "<=": lambda a, b: a <= b, "has": lambda a, b: b in a}
    for fr, key, op, want in sp["require"]:
        if fr == frame:
            assert key in facts, "frame %d: the model has nothing to say about %r" % (frame, key)
            assert ops[op](facts[key], want), "precondition: frame %d, %s = %r, wanted %s %r" % (frame, key, facts[key], op, want)


def assert_same_bytes(o, g):
    oi, gi = o.block_indices(), g.block_indices()
    assert oi.tobytes() == gi.tobytes()
    _, ot, osem = o.download(oi)
    _, gt, gsem = g.download(oi)
    assert ot.tobytes() == gt.tobytes() and osem.tobytes() == gsem.tobytes()


def compare(sp, o, g):
    from tests.util import compare_maps
    if sp["compare"] == "probability_colours":   # (colours go through exp(): one LSB allowed on the TSDF colour only, as in tests/test_apply_runs_gpu.py)
        rep = compare_maps(o, g, exact=False)
        assert rep["label_mismatches"] == 0 and rep["max_abs_priors_err"] == 0.0 and rep["max_abs_distance_err"] == 0.0 and rep["max_rel_weight_err"] == 0.0, rep
        assert rep["tsdf_color_mismatches"] <= rep["voxels_compared"] * 1e-3 and rep["sem_color_mismatches"] == 0, rep
        assert o.block_indices().tobytes() == g.block_indices().tobytes()
        return rep
    if sp["compare"] == "bytes":                 # (a class sum of -inf: compare_maps' error figures are NaN there; the bytes say more anyway)
        assert_same_bytes(o, g)
        return {}
    rep = compare_maps(o, g, exact=True)
    assert_same_bytes(o, g)
    return rep


def run_case(sp, log=print):
    from kimera_semantics_amd import synth
    o, g, cfg = contexts(sp)
    tracked = sp["tracked"] or [[0, 0, 0]]
    T = np.array([1, 0, 0, 0] + list(sp["sensor"]), F)
    colours = synth.default_label_colors()
    before, frame, observed = dict(ZERO), 0, []
    for step in sp["steps"]:
        if "upload" in step:
            apply_edit(o, g, step["upload"])
            frame += 1
            continue
        xyz, labels, info = make_cloud(step["cloud"], sp["sensor"])
        recs = [record(o, v) for v in tracked]
        so = o.integrate(T, xyz, colours[labels], labels)
        sg = g.integrate(T, xyz, colours[labels], labels)
        sg_flush = g.flush()
        assert so.n_rays_cast == sg.n_rays_cast + sg_flush.n_rays_cast, (so.n_rays_cast, sg.n_rays_cast)
        st = g.update_stats()
        delta = {k: st[k] - before[k] for k in STAT_KEYS}
        before = st
        rec1 = record(o, tracked[0])
        if step["expect"] == "model":
            want, facts = facts_uniform(sp, cfg, step, xyz, info, recs, so.n_rays_cast)
            if "model_end" in facts:             # the model's serial chains against the oracle's record: the yardstick itself is checked
                assert facts["model_end"][:M.NUM_LABELS].tobytes() == rec1["priors"].tobytes() and facts["model_end"][M.NUM_LABELS] == rec1["weight"]
                del facts["model_end"]
            log("frame %d: rays %d, model %s, observed %s, facts %s" % (frame, so.n_rays_cast, want, delta, facts))
            check_requirements(sp, frame, facts)
            if sp["env"].get("KS_XL_CAP_CHUNKS") and facts["fates"] == ["walked", "walked"]:
                # room for one of the two runs only, whichever the device lists first: one walked, one handed to the serial kernel
                assert delta["walked"] == 1 and delta["serial"] == 1 and delta["chunks"] in facts["chunks_of_runs"], (frame, delta)
                assert facts["chunks_of_runs"][0] == int(sp["env"]["KS_XL_CAP_CHUNKS"]) < sum(facts["chunks_of_runs"])
            else:
                assert delta == want, "frame %d: update_stats moved by %s, the model says %s" % (frame, delta, want)
        else:
            facts = facts_other(sp, cfg, xyz, info, recs[0], rec1) if recs[0] is not None else {}
            log("frame %d: rays %d, observed %s, facts %s" % (frame, so.n_rays_cast, delta, facts))
            check_requirements(sp, frame, facts)
            if "bundles" in info:
                assert so.n_rays_cast == info["bundles"], (so.n_rays_cast, info["bundles"])
            if step["expect"] is not None:
                assert so.n_rays_cast > M.LONG_RUN
                assert {k: delta[k] for k in step["expect"]} == step["expect"], (frame, delta)
                assert 0 < delta["chunks"] - delta["replayed"], (frame, delta)
        observed.append(delta)
        frame += 1
    rep = compare(sp, o, g)
    log("update_stats %s" % g.update_stats())
    return dict(observed=observed, voxels=rep.get("oracle_touched"))


def run_sequence(pipeline, env=None, log=print):
    """The run-edge clouds as six frames in flight (device-only tests of the GPU tier): (oracle, library, model's total, observed total).
    update_stats() is read once, after the last frame: it completes the frames in flight."""
    from kimera_semantics_amd import synth
    sp = SEQUENCE
    o, g, cfg = contexts(sp, pipeline=pipeline, env=env)
    T = np.array([1, 0, 0, 0] + list(sp["sensor"]), F)
    colours = synth.default_label_colors()
    want = dict(ZERO)
    for step in sp["steps"]:
        xyz, labels, info = make_cloud(step["cloud"], sp["sensor"])
        rec = record(o, [0, 0, 0])
        so = o.integrate(T, xyz, colours[labels], labels)
        g.integrate(T, xyz, colours[labels], labels)
        pred, _ = facts_uniform(sp, cfg, step, xyz, info, [rec], so.n_rays_cast)
        for k in STAT_KEYS:
            want[k] += pred[k]
    g.flush()
    st = g.update_stats()
    log("pipeline_frames %d %s: model %s, observed %s" % (pipeline, env or {}, want, st))
    return o, g, want, st


def main():
    sp = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this entry drives the functional model only"
    out = run_case(sp)
    print("XL_CASE_OK", json.dumps(out))


if __name__ == "__main__":
    main()
