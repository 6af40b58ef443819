"""The view-rendering cases, shared by both tiers: run_case(spec) drives whatever library the binding has loaded — the GPU
tier (tests/test_render_gpu.py) calls it in-process, the CPU tier (tests/test_render_cpu.py) runs it as a child process on
the host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.render_case '<json spec>'
The checker is tests/render_model.py (NumPy, written from the contract): all four images as bit patterns, and the stats."""
import json
import math
import os
import sys

import numpy as np

from tests import mesh_case

VOXEL = mesh_case.VOXEL          # 5 cm
# Cameras of the analytic fields (which fill [-0.8 m, 0.8 m)^3): T_G_C = (qw, qx, qy, qz, tx, ty, tz), camera z forward.
#   front   outside the box at z = -1.1, looking +z with a small rotation
#   back    at z = +1.1, looking -z (half a turn about x, slightly perturbed): the positive side of the `plane` field
#   inside  inside the sphere: every sample until the ray leaves it is negative
#   corner  outside the box at 45 degrees about y, 1.84 m from the centre: the first 0.7 m and more of every ray are invalid
def _unit(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q)


CAMERAS = {
    "front": np.concatenate([_unit([1.0, 0.02, -0.03, 0.01]), [0.11, -0.07, -1.1]]).astype(np.float32),
    "back": np.concatenate([_unit([0.02, 1.0, 0.01, -0.03]), [0.11, -0.07, 1.1]]).astype(np.float32),
    "inside": np.concatenate([_unit([1.0, 0.02, -0.03, 0.01]), [0.05, 0.02, -0.03]]).astype(np.float32),
    "corner": np.concatenate([_unit([math.cos(math.pi / 8), 0.01, math.sin(math.pi / 8), -0.02]), [-1.3, 0.1, -1.3]]).astype(np.float32),
}
K_EVEN = (40.0, 42.0, 31.5, 23.5)       # 64 x 48
K_ODD = (40.0, 42.0, 28.3, 24.9)        # 61 x 45: cx, cy off centre, fx != fy


def _rows(a):
    return {tuple(int(v) for v in r) for r in np.asarray(a).reshape(-1, 3)}


def _bytes(got):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in got[:4]) + repr(sorted(got[4].items())).encode()


def _fraction(got):
    return got[4]["pixels_hit"] / float(got[4]["pixels_hit"] + got[4]["pixels_missed"])


def case_upload(spec):
    from tests import render_model as M
    vps = spec["vps"]
    w, h = spec.get("size", [64, 48])
    K = K_ODD if (w, h) == (61, 45) else K_EVEN
    T = CAMERAS[spec.get("camera", "front")]
    g = mesh_case._integrator(0, 64, 48, vps=vps)
    idx, t, s = mesh_case.make_field(spec["field"], vps)
    g.upload(idx, t, s)
    got = g.render(T, K, w, h, **spec.get("cfg", {}))
    model = M.model_of(g, T, K, w, h, spec.get("cfg"))
    M.assert_same(got, model, spec["field"])
    frac = _fraction(got)
    lo, hi = spec.get("hit_fraction", [0.0, 1.0])
    assert lo <= frac <= hi, (frac, lo, hi)
    assert got[4]["pixels_hit"] + got[4]["pixels_missed"] == w * h and got[4]["samples"] >= w * h
    if spec["field"] == "two_label" and lo > 0:
        assert {3, 7} <= set(np.unique(got[1])), np.unique(got[1])
    again = g.render(T, K, w, h, **spec.get("cfg", {}))   # two calls give the same bytes
    assert _bytes(again) == _bytes(got)
    no_normals = g.render(T, K, w, h, normals=False, **spec.get("cfg", {}))
    assert no_normals[3] is None and _bytes(no_normals[:3] + (got[3], no_normals[4])) == _bytes(got)
    g.close()
    return dict(hit_fraction=round(frac, 4), samples_per_pixel=round(got[4]["samples"] / float(w * h), 2))


def _integrated(spec, pipeline=0, n_frames=2, max_tiles=4096):
    w, h = spec.get("size", [64, 48])
    g = mesh_case._integrator(spec.get("method", 0), w, h, pipeline=pipeline, max_tiles=max_tiles)
    frames = mesh_case._frames(n_frames, w, h)
    for f in frames:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    return g, frames


def other_pose():
    """A pose neither frame of mesh_case._frames (trajectory poses 0 and 5) had: on the circle between them, 5 cm lower."""
    from kimera_semantics_amd import synth
    return synth.trajectory_pose(3, height=1.45)


def case_integrated(spec):
    from tests import render_model as M
    w, h = spec.get("size", [64, 48])
    g, frames = _integrated(spec)
    idx, t, s = g.download()
    dense = M.Dense(idx, t, s, g.vps)
    out = {}
    for name, T in (("second_frame", frames[1].T_G_C), ("other", other_pose())):
        got = g.render(T, frames[1].K, w, h)
        model = M.render_from_blocks(idx, t, s, g.vps, VOXEL, T, frames[1].K, w, h, dense=dense)
        M.assert_same(got, model, name)
        frac = _fraction(got)
        assert frac >= 0.30, (name, frac)
        seen = np.unique(got[1][got[1] != 255])
        assert len(seen) >= 2, (name, seen)
        out[name] = round(frac, 4)
    g.close()
    return out


def case_side_effects(spec):
    """Rendering reads the map and writes nothing in it: the host-sync flags, both stale bits, the stored mesh and ESDF and
    the voxels are what they were; two renders give the same bytes."""
    from tests import render_model as M
    w, h = 64, 48
    g, frames = _integrated(spec)
    g.mesh()
    g.esdf_update(min_distance_m=0.1, max_distance_m=0.4)
    T, K = frames[1].T_G_C, frames[1].K

    def state():
        idx, t, s = g.download()
        m = g.mesh(only_stale=True)
        e = g.esdf_refresh()
        return dict(updated=_rows(g.updated_block_indices(reset=False)), meshed=m.stats["blocks_meshed"], stale=e["tiles_stale"],
                    map=idx.tobytes() + t.tobytes() + s.tobytes(),
                    mesh=b"".join(np.ascontiguousarray(getattr(m, k)).tobytes() for k in ("blocks", "xyz", "normals", "rgba", "labels")),
                    esdf=g.esdf_blocks(idx).tobytes())

    before = state()
    assert before["meshed"] == 0 and before["stale"] == 0 and len(before["updated"]) > 0
    first = g.render(T, K, w, h)
    second = g.render(T, K, w, h)
    assert _bytes(first) == _bytes(second)
    after = state()
    for k in before:
        assert before[k] == after[k], k
    M.assert_same(first, M.model_of(g, T, K, w, h), "side_effects")
    assert first[4]["pixels_hit"] > 0
    g.close()
    return {}


def case_errors(spec):
    import ctypes as C
    from kimera_semantics_amd import binding as B
    from tests import render_model as M
    w, h = 24, 16
    K = (20.0, 21.0, 11.5, 7.5)
    T = CAMERAS["front"]
    g = mesh_case._integrator(0, 64, 48, vps=8)

    def refused(code, call, what):
        try:
            call()
        except B.KsError as e:
            assert e.code == code, (what, e)
            return
        raise AssertionError("%s accepted" % (what,))

    # an empty map is not an error: every pixel misses
    got = g.render(T, K, w, h)
    M.assert_same(got, M.model_of(g, T, K, w, h), "empty map")
    assert got[4]["pixels_hit"] == 0 and got[4]["pixels_missed"] == w * h and np.isnan(got[0]).all() and (got[1] == 255).all()
    idx, t, s = mesh_case.make_field("sphere", 8)
    g.upload(idx, t, s)
    full = g.render(T, K, w, h)
    assert full[4]["pixels_hit"] > 0
    for bad in (0, -1, 8193):
        refused(B.KS_ERR_INVALID_ARG, lambda: g.render(T, K, bad, h), ("width", bad))
        refused(B.KS_ERR_INVALID_ARG, lambda: g.render(T, K, w, bad), ("height", bad))
    for ww, hh in ((8192, 1), (1, 8192)):   # (the limits themselves pass)
        st = g.render(T, K, ww, hh)[4]
        assert st["pixels_hit"] + st["pixels_missed"] == 8192, st
    for k in range(4):
        for bad in (float("nan"), float("inf"), -float("inf")):
            Kb = list(K)
            Kb[k] = bad
            refused(B.KS_ERR_INVALID_ARG, lambda: g.render(T, Kb, w, h), ("K", k, bad))
    for k in range(2):
        for bad in (0.0, -40.0):
            Kb = list(K)
            Kb[k] = bad
            refused(B.KS_ERR_INVALID_ARG, lambda: g.render(T, Kb, w, h), ("K", k, bad))
    for name in ("min_weight", "min_range_m", "max_range_m"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused(B.KS_ERR_INVALID_ARG, lambda: g.render(T, K, w, h, **{name: bad}), (name, bad))
    refused(B.KS_ERR_INVALID_ARG, lambda: g.render(T, K, w, h, min_range_m=2.0, max_range_m=2.0), "min_range_m == max_range_m")
    refused(B.KS_ERR_INVALID_ARG, lambda: g.render(T, K, w, h, min_range_m=3.0, max_range_m=2.0), "min_range_m > max_range_m")
    refused(B.KS_ERR_INVALID_ARG, lambda: g.render(T, K, w, h, max_range_m=205.0), "more than 4096 voxels")   # 205 / 0.05 = 4100
    # the NULL-output combinations: none -> refused; any one alone -> that image of the full call
    L = B.lib()
    rc, st = g.render_config(), B.KsRenderStats()
    Tc, Kc = np.ascontiguousarray(T, np.float32), np.ascontiguousarray(K, np.float32)
    raw = lambda d, l, c, n, stats: L.ks_render_view(g._h, Tc.ctypes.data, Kc.ctypes.data, w, h, C.byref(rc), d, l, c, n, stats)
    assert raw(None, None, None, None, C.byref(st)) == B.KS_ERR_INVALID_ARG
    assert L.ks_render_view_device(g._h, Tc.ctypes.data, Kc.ctypes.data, w, h, C.byref(rc), None, None, None, None, None) == B.KS_ERR_INVALID_ARG
    for k in range(4):
        out = [np.zeros_like(full[j]) if j == k else None for j in range(4)]
        assert raw(*[None if a is None else a.ctypes.data for a in out], None if k % 2 else C.byref(st)) == 0
        assert out[k].tobytes() == full[k].tobytes(), k
        if not k % 2:
            assert {f: int(getattr(st, f)) for f, _ in B.KsRenderStats._fields_} == full[4]
    both = [np.zeros_like(full[0]), np.zeros_like(full[1])]
    assert raw(both[0].ctypes.data, both[1].ctypes.data, None, None, None) == 0
    assert both[0].tobytes() == full[0].tobytes() and both[1].tobytes() == full[1].tobytes()
    g.clear()
    cleared = g.render(T, K, w, h)
    assert cleared[4]["pixels_hit"] == 0 and _bytes(cleared) == _bytes(got)
    g.close()
    # a marcher context of the exact multi-GPU mode holds no voxel data
    marcher, owner = (mesh_case._integrator(1, 64, 48) for _ in range(2))
    f = mesh_case._frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    refused(B.KS_ERR_UNSUPPORTED, lambda: marcher.render(f.T_G_C, f.K, 64, 48), "a marcher context")
    assert owner.render(f.T_G_C, f.K, 64, 48)[4]["pixels_hit"] > 0   # (the owner holds the map)
    marcher.close()
    owner.close()
    return {}


# median |rendered depth - input depth| of the second frame, in metres, measured with the model (fast, merged): about a tenth
# of a voxel — the TSDF averages two frames' noisy projective distances and the surface is read off by interpolation
ROUND_TRIP_MEASURED_M = {0: 0.00455, 1: 0.00225}


def case_round_trip(spec):
    """Model level: the device code is not judged here, it only integrates the frames."""
    from tests import render_model as M
    out = {}
    for method in (0, 1):
        g, frames = _integrated(dict(method=method))
        f = frames[1]
        m = M.model_of(g, f.T_G_C, f.K, 64, 48)
        g.close()
        both = m["hit"] & np.isfinite(f.depth)
        assert both.sum() >= 0.3 * both.size, both.sum()
        med = float(np.median(np.abs(m["depth"][both].astype(np.float64) - f.depth[both].astype(np.float64))))
        print("round trip, method %d: median |rendered - input| = %.5f m (%.3f voxel) over %d pixels" % (method, med, med / VOXEL, both.sum()))
        assert med < min(2 * ROUND_TRIP_MEASURED_M[method], 2 * VOXEL), (method, med)
        out[str(method)] = round(med, 6)
    return out


CASES = {"round_trip": case_round_trip, "upload": case_upload, "integrated": case_integrated, "side_effects": case_side_effects, "errors": case_errors}

# name -> spec: the same cases in both tiers.  The hit fractions are conditions that keep a case from being empty; they were
# checked with the model alone (tests/test_render_cpu.py does so again).
SPECS = {
    "sphere_vps8": dict(case="upload", field="sphere", vps=8, hit_fraction=[0.5, 0.9]),
    "sphere_vps16": dict(case="upload", field="sphere", vps=16, hit_fraction=[0.5, 0.9]),
    "plane_vps8": dict(case="upload", field="plane", vps=8, camera="back", hit_fraction=[0.5, 1.0]),
    "plane_vps16": dict(case="upload", field="plane", vps=16, camera="back", hit_fraction=[0.5, 1.0]),
    "two_label_vps8": dict(case="upload", field="two_label", vps=8, hit_fraction=[0.5, 0.9]),
    "two_label_vps16": dict(case="upload", field="two_label", vps=16, hit_fraction=[0.5, 0.9]),
    "holes_vps8": dict(case="upload", field="holes", vps=8, hit_fraction=[0.05, 0.9]),
    "holes_vps16": dict(case="upload", field="holes", vps=16, hit_fraction=[0.05, 0.9]),
    "odd_size_61x45": dict(case="upload", field="sphere", vps=8, size=[61, 45], hit_fraction=[0.5, 0.9]),
    "camera_outside_box": dict(case="upload", field="sphere", vps=8, camera="corner", cfg=dict(min_range_m=0.02), hit_fraction=[0.1, 0.9]),
    "camera_inside_sphere": dict(case="upload", field="sphere", vps=8, camera="inside", hit_fraction=[0.0, 0.0]),
    "plane_from_negative_side": dict(case="upload", field="plane", vps=8, camera="front", hit_fraction=[0.0, 0.0]),
    "integrated_fast": dict(case="integrated", method=0),
    "integrated_merged": dict(case="integrated", method=1),
    "side_effects": dict(case="side_effects"),
    "errors": dict(case="errors"),
}


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    print("RENDER_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
