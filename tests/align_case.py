"""The scan-alignment cases, shared by both tiers: run_case(spec) drives whatever library the binding has loaded — the GPU
tier (tests/test_align_gpu.py) calls it in-process, the CPU tier (tests/test_align_cpu.py) runs it as a child process on the
host functional model of the device code:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.align_case '<json spec>'
The checker is tests/align_model.py (NumPy, written from the contract): the refined pose as bit patterns, every stats field."""
import json
import math
import os
import sys

import numpy as np

from tests import mesh_case, render_case

VOXEL = mesh_case.VOXEL
PERTURB_T = (0.03, -0.02, 0.025)                  # metres, world frame
PERTURB_DEG, PERTURB_AXIS = 1.5, (1.0, 2.0, -1.0)  # about (1, 2, -1) / sqrt(6), world frame, about the sensor origin
PLANE_N, PLANE_C = np.array([0.31, -0.52, 0.79]) / np.linalg.norm([0.31, -0.52, 0.79]), 0.0613   # mesh_case.make_field("plane")


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def quat_R(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def perturbed(T, dt=PERTURB_T, deg=PERTURB_DEG, axis=PERTURB_AXIS):
    """T moved by dt and turned by deg about axis, both in the world frame (the rotation about the sensor origin)."""
    T = np.asarray(T, np.float64)
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    h = math.radians(deg) / 2
    q = quat_mul(np.concatenate([[math.cos(h)], math.sin(h) * ax]), T[:4])
    return np.concatenate([q / np.linalg.norm(q), T[4:] + np.asarray(dt)]).astype(np.float32)


def pose_error(T, T_true):
    """(translation error in metres, rotation error in degrees) of T against T_true."""
    T, T_true = np.asarray(T, np.float64), np.asarray(T_true, np.float64)
    Rd = quat_R(T[:4]) @ quat_R(T_true[:4]).T
    return float(np.linalg.norm(T[4:] - T_true[4:])), float(np.degrees(np.arccos(np.clip((np.trace(Rd) - 1) / 2, -1, 1))))


def surface_cloud(field, n, T, seed=7, shift=0.0):
    """n points of the field's zero level set (moved by `shift` along its normal), in the camera frame of pose T."""
    rng = np.random.default_rng(seed)
    if field == "plane":
        x = rng.uniform(-0.45, 0.45, (n, 3))
        pw = x - (x @ PLANE_N - PLANE_C)[:, None] * PLANE_N + shift * PLANE_N
    else:
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        pw = np.array(mesh_case.SPHERE_CENTRE) + (mesh_case.SPHERE_RADIUS + shift) * d
    T = np.asarray(T, np.float64)
    return ((pw - T[4:]) @ quat_R(T[:4])).astype(np.float32)


def _bytes(got):
    return got[0].tobytes() + repr(sorted(got[1].items())).encode()


def case_cloud(spec, T_true):
    xyz = surface_cloud(spec["field"], spec["n"], T_true)
    if spec.get("non_finite"):          # NaN and Inf points interleaved
        xyz[1::5, 0] = np.nan
        xyz[2::7, 2] = np.inf
        xyz[3::11] = -np.inf
    if spec.get("outside"):             # every third point outside every resident tile
        xyz[::3] += np.float32(7.0)
    if spec.get("all_invalid"):
        xyz += np.float32(7.0)
    return xyz


def case_upload(spec):
    from tests import align_model as M
    vps, field, n = spec["vps"], spec["field"], spec["n"]
    cfg = dict(spec.get("cfg", {}))
    T_true = render_case.CAMERAS["front"]
    xyz = case_cloud(spec, T_true)
    T0 = T_true if spec.get("start_at_truth") else perturbed(T_true)
    g = mesh_case._integrator(0, 64, 48, vps=vps)
    g.upload(*mesh_case.make_field(field, vps))
    got = g.align(T0, xyz, **cfg)
    model = M.model_of(g, T0, xyz, cfg)
    M.assert_same(got, model, field)
    again = g.align(T0, xyz, **cfg)    # two calls give the same bytes
    assert _bytes(again) == _bytes(got)
    st = got[1]
    if "status" in spec:
        assert st["status"] == spec["status"], st
    if spec.get("pose_kept"):
        assert got[0].tobytes() == np.asarray(T0, np.float32).tobytes() and st["iterations"] == 0, (got, T0)
    if spec.get("start_at_truth"):
        assert st["iterations"] < dict(M.DEFAULT_CFG, **cfg)["max_iterations"], st
    stride = cfg.get("point_stride", 1)
    assert st["points_used"] <= (n + stride - 1) // stride and st["inliers_first"] >= spec.get("inliers_at_least", 0), st
    g.close()
    return dict(st, error=[round(v, 5) for v in pose_error(got[0], T_true)])


def integrated(method, n_frames, w=64, h=48, pipeline=0):
    g = mesh_case._integrator(method, w, h, pipeline=pipeline)
    for f in mesh_case._frames(n_frames, w, h):
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    return g


def other_cloud(w=64, h=48):
    """The cloud a camera at render_case.other_pose() sees: (true pose, xyz in the camera frame)."""
    from kimera_semantics_amd import synth
    T = render_case.other_pose()
    f = synth.render_frame(synth.make_scene("room"), T, w, h, hfov_deg=90.0, seed=77)
    return f.T_G_C, f.xyz


RECOVERY_FRAMES = 2
# what the model's refinement leaves of the perturbation on the integrated map (fast, merged): (metres, degrees), as the test prints
RECOVERY_MEASURED = {0: (0.01612, 0.3278), 1: (0.01290, 0.0656)}


def case_integrated(spec):
    from tests import align_model as M
    g = integrated(spec["method"], RECOVERY_FRAMES)
    T_true, xyz = other_cloud()
    T0 = perturbed(T_true)
    cfg = dict(spec.get("cfg", {}))
    got = g.align(T0, xyz, **cfg)
    M.assert_same(got, M.model_of(g, T0, xyz, cfg), "integrated")
    assert got[1]["inliers_first"] >= 0.3 * got[1]["points_used"] > 0, got[1]
    g.close()
    return dict(got[1], error=[round(v, 5) for v in pose_error(got[0], T_true)])


def case_recovery(spec):
    """Model level: the device code is not judged here, it only integrates the frames."""
    from tests import align_model as M
    out = {}
    T_true, xyz = other_cloud()
    T0 = perturbed(T_true)
    e0 = pose_error(T0, T_true)
    for method in (0, 1):
        g = integrated(method, RECOVERY_FRAMES)
        T, st, _ = M.model_of(g, T0, xyz, dict(max_iterations=20))
        g.close()
        e = pose_error(T, T_true)
        print("recovery, method %d: %.5f m, %.4f deg -> %.5f m, %.4f deg; %r" % (method, e0[0], e0[1], e[0], e[1], st))
        assert st["inliers_first"] >= 0.3 * st["points_used"] > 0, st
        assert e[0] < 0.5 * e0[0] and e[1] < 0.5 * e0[1], (e0, e)
        assert e[0] < 2 * RECOVERY_MEASURED[method][0] and e[1] < 2 * RECOVERY_MEASURED[method][1], (e, RECOVERY_MEASURED[method])
        out[str(method)] = [round(e[0], 6), round(e[1], 5)]
    return out


def case_side_effects(spec):
    """Aligning reads the map and writes nothing in it (render_case.case_side_effects' state() around two align calls)."""
    from tests import align_model as M
    g, frames = render_case._integrated(spec)
    g.mesh()
    g.esdf_update(min_distance_m=0.1, max_distance_m=0.4)
    _rows = render_case._rows

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
    T0, xyz = perturbed(frames[1].T_G_C), frames[1].xyz
    first = g.align(T0, xyz)
    second = g.align(T0, xyz)
    assert _bytes(first) == _bytes(second)
    after = state()
    for k in before:
        assert before[k] == after[k], k
    M.assert_same(first, M.model_of(g, T0, xyz), "side_effects")
    assert first[1]["inliers_first"] > 0 and first[1]["iterations"] > 0
    g.close()
    return {}


def case_errors(spec):
    import ctypes as C
    from kimera_semantics_amd import binding as B
    from tests import align_model as M
    T = render_case.CAMERAS["front"]
    xyz = surface_cloud("sphere", 200, T)
    g = mesh_case._integrator(0, 64, 48, vps=8)

    def refused(code, call, what):
        try:
            call()
        except B.KsError as e:
            assert e.code == code, (what, e)
            return
        raise AssertionError("%s accepted" % (what,))

    def kept(got, what):
        assert got[0].tobytes() == T.tobytes() and got[1]["status"] == B.KS_ALIGN_TOO_FEW_INLIERS and got[1]["iterations"] == 0, (what, got)
        assert got[1]["inliers_first"] == 0 and got[1]["inliers_last"] == 0 and got[1]["rmse_first"] == 0.0 and got[1]["rmse_last"] == 0.0, (what, got)

    # an empty map and an empty cloud are no errors
    empty = g.align(T, xyz)
    kept(empty, "empty map")
    M.assert_same(empty, M.model_of(g, T, xyz), "empty map")
    assert empty[1]["points_used"] == 200
    g.upload(*mesh_case.make_field("sphere", 8))
    none = g.align(T, np.zeros((0, 3), np.float32))
    kept(none, "n = 0")
    M.assert_same(none, M.model_of(g, T, np.zeros((0, 3), np.float32)), "n = 0")
    full = g.align(T, xyz)
    assert full[1]["inliers_first"] > 100
    for k in range(7):
        for bad in (float("nan"), float("inf"), -float("inf")):
            Tb = T.copy()
            Tb[k] = bad
            refused(B.KS_ERR_INVALID_ARG, lambda: g.align(Tb, xyz), ("T", k, bad))
    refused(B.KS_ERR_INVALID_ARG, lambda: g.align(np.array([0, 0, 0, 0, 1, 2, 3], np.float32), xyz), "a zero quaternion")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(B.KS_ERR_INVALID_ARG, lambda: g.align(T, xyz, min_weight=bad), ("min_weight", bad))
    for name in ("max_residual_m", "damping", "eps_rotation_rad", "eps_translation_m"):
        for bad in (-1.0, float("nan"), float("inf")):
            refused(B.KS_ERR_INVALID_ARG, lambda: g.align(T, xyz, **{name: bad}), (name, bad))
    for name, values in (("max_iterations", (0, -1, 65)), ("point_stride", (0, -3)), ("min_inliers", (0, -1)), ("dof_mask", (0, 0x40, 0xffffffff))):
        for bad in values:
            refused(B.KS_ERR_INVALID_ARG, lambda: g.align(T, xyz, **{name: bad}), (name, bad))
    for ok in (dict(max_iterations=64), dict(max_iterations=1), dict(dof_mask=1), dict(max_residual_m=0.0), dict(eps_rotation_rad=0.0)):   # (the limits pass)
        g.align(T, xyz, **ok)
    # the NULL arguments, n >= 2^31 (refused before the cloud is touched), stats may be NULL
    L = B.lib()
    ac, st, out = g.align_config(), B.KsAlignStats(), np.zeros(7, np.float32)
    raw = lambda fn, Tp, cfg, outp, n=len(xyz), stats=None: fn(g._h, Tp, xyz.ctypes.data, n, cfg, outp, stats)
    for fn in (L.ks_align_points, L.ks_align_points_device):
        assert raw(fn, None, C.byref(ac), out.ctypes.data) == B.KS_ERR_INVALID_ARG
        assert raw(fn, T.ctypes.data, None, out.ctypes.data) == B.KS_ERR_INVALID_ARG
        assert raw(fn, T.ctypes.data, C.byref(ac), None) == B.KS_ERR_INVALID_ARG
        assert raw(fn, T.ctypes.data, C.byref(ac), out.ctypes.data, n=1 << 31) == B.KS_ERR_INVALID_ARG
    assert raw(L.ks_align_points, T.ctypes.data, C.byref(ac), out.ctypes.data) == 0 and out.tobytes() == full[0].tobytes()
    assert raw(L.ks_align_points, T.ctypes.data, C.byref(ac), out.ctypes.data, stats=C.byref(st)) == 0 and st.inliers_first == full[1]["inliers_first"]
    g.clear()
    kept(g.align(T, xyz), "after ks_clear")
    g.close()
    # a marcher context of the exact multi-GPU mode holds no voxel data
    marcher, owner = (mesh_case._integrator(1, 64, 48) for _ in range(2))
    f = mesh_case._frames(1, 64, 48)[0]
    owner.integrate_round_exact(marcher, None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)
    refused(B.KS_ERR_UNSUPPORTED, lambda: marcher.align(f.T_G_C, f.xyz), "a marcher context")
    assert owner.align(f.T_G_C, f.xyz)[1]["inliers_first"] > 0   # (the owner holds the map)
    marcher.close()
    owner.close()
    return {}


CASES = {"upload": case_upload, "integrated": case_integrated, "recovery": case_recovery, "side_effects": case_side_effects, "errors": case_errors}

_SMALL = dict(min_inliers=1)
# name -> spec: the same cases in both tiers.  Statuses: 0 CONVERGED, 1 ITERATION_LIMIT, 2 TOO_FEW_INLIERS, 3 DEGENERATE.
SPECS = {
    "sphere_1_point": dict(case="upload", field="sphere", vps=8, n=1, cfg=_SMALL, inliers_at_least=1),
    "sphere_63_points": dict(case="upload", field="sphere", vps=8, n=63, cfg=_SMALL, inliers_at_least=32),
    "sphere_64_points": dict(case="upload", field="sphere", vps=8, n=64, cfg=_SMALL, inliers_at_least=32),
    "sphere_65_points": dict(case="upload", field="sphere", vps=8, n=65, cfg=_SMALL, inliers_at_least=32),
    # 258 wavefronts: the finisher's strided loop runs twice for two work-items (one iteration keeps the functional model quick)
    "sphere_16453_points": dict(case="upload", field="sphere", vps=8, n=16453, cfg=dict(max_iterations=1), status=1, inliers_at_least=8000),
    "sphere_vps16_stride_3": dict(case="upload", field="sphere", vps=16, n=1000, cfg=dict(point_stride=3), inliers_at_least=200),
    "plane_vps16": dict(case="upload", field="plane", vps=16, n=700, inliers_at_least=350),
    "plane_stride_3_non_finite": dict(case="upload", field="plane", vps=8, n=900, non_finite=True, cfg=dict(point_stride=3), inliers_at_least=100),
    "sphere_non_finite": dict(case="upload", field="sphere", vps=8, n=500, non_finite=True, inliers_at_least=150),
    "sphere_points_outside_the_map": dict(case="upload", field="sphere", vps=8, n=600, outside=True, inliers_at_least=200),
    "holes_vps8": dict(case="upload", field="holes", vps=8, n=1500, inliers_at_least=100),
    "holes_vps16": dict(case="upload", field="holes", vps=16, n=1500, inliers_at_least=100),
    "all_points_invalid": dict(case="upload", field="sphere", vps=8, n=300, all_invalid=True, status=2, pose_kept=True),
    "yaw_and_translation_0x3c": dict(case="upload", field="sphere", vps=8, n=500, cfg=dict(dof_mask=0x3c), inliers_at_least=250),
    "translation_only_0x38": dict(case="upload", field="plane", vps=8, n=500, cfg=dict(dof_mask=0x38), inliers_at_least=250),
    # (translation only: the sphere leaves a rotation about its own centre free, and the damped steps along it do not die out)
    "start_at_the_true_pose": dict(case="upload", field="sphere", vps=8, n=500, start_at_truth=True, cfg=dict(dof_mask=0x38), status=0, inliers_at_least=400),
    "plane_without_damping_is_degenerate": dict(case="upload", field="plane", vps=8, n=500, cfg=dict(damping=0.0), status=3, pose_kept=True,
                                                inliers_at_least=250),
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
    print("ALIGN_CASE_OK", json.dumps(run_case(spec)))


if __name__ == "__main__":
    main()
