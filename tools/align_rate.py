#!/usr/bin/env python3
"""Rate of the on-device scan alignment (ks_align_points) beside what a host ICP needs first, the layer download.
On the map the headline of bench.py builds (the C2 ring), with the 640 x 480 clouds of the ring's own frames, each from its
pose moved by (0.03, -0.02, 0.025) m and turned by 1.5 degrees, in ONE process, candidates alternating, the median of --reps
repetitions after warm-up, the context synchronised before every timed call:
  (i)   ks_align_points_device, the cloud already on the device, default configuration (the whole loop and its one read-back)
  (ii)  ks_align_points, the cloud in page-locked host memory (the upload of the cloud plus (i))
  (iii) one (evaluate, finish) kernel pair: device events around a call of 20 iterations minus those around one of 4, over 16
        (eps = 0, so no call ends early)
  (iv)  ks_download_blocks of every block (TSDF + semantic layer) into page-locked memory: what a host ICP waits for
and the iterations, inlier fraction and pose error of every call.  There is no pass mark.  Writes profiles/align_rate.json (or --out)."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workloads and the integrator configuration of the headline)
from kimera_semantics_amd import binding as B  # noqa: E402


def med(xs):
    return round(statistics.median(xs) * 1e3, 4)


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def perturbed(T):
    T = np.asarray(T, np.float64)
    h = math.radians(1.5) / 2
    q = quat_mul(np.concatenate([[math.cos(h)], math.sin(h) * np.array([1.0, 2.0, -1.0]) / math.sqrt(6.0)]), T[:4])
    return np.concatenate([q / np.linalg.norm(q), T[4:] + np.array([0.03, -0.02, 0.025])]).astype(np.float32)


def pose_error(T, T_true):
    T, T_true = np.asarray(T, np.float64), np.asarray(T_true, np.float64)
    conj = T_true[:4] * np.array([1.0, -1.0, -1.0, -1.0])
    d = quat_mul(T[:4] / np.linalg.norm(T[:4]), conj / np.linalg.norm(conj))
    return float(np.linalg.norm(T[4:] - T_true[4:])), float(math.degrees(2 * math.atan2(np.linalg.norm(d[1:]), abs(d[0]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40, help="frames of the ring integrated before anything is measured")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_rate.json"))
    a = ap.parse_args()
    import torch
    wl = bench.WORKLOADS["C2"]
    w, h = wl["w"], wl["h"]
    ring = bench.make_frames(wl, range(a.frames))
    L = B.lib()
    g = B.HipIntegrator(B.default_config(max_tiles=1 << 13, max_points=w * h, pipeline_frames=0, **bench.integ_cfg(wl)))
    for f in ring:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.synchronize()
    blocks = g.block_indices()
    tiles = len(g.tile_keys())
    nv = g.vps ** 3
    chk = g._chk

    def pinned(nbytes):
        p = L.ks_host_alloc(max(int(nbytes), 1))
        assert p, "ks_host_alloc failed"
        return p

    p_xyz = pinned(12 * w * h)
    p_tsdf, p_sem = pinned(len(blocks) * nv * 12), pinned(len(blocks) * nv * 92)
    d_xyz = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(g.stream)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ac, st, out7 = g.align_config(), B.KsAlignStats(), np.zeros(7, np.float32)

    def stage(f):
        xyz = np.ascontiguousarray(f.xyz, np.float32)
        C.memmove(p_xyz, xyz.ctypes.data, xyz.nbytes)
        d_xyz[:len(xyz)].copy_(torch.from_numpy(xyz))
        torch.cuda.synchronize()
        return len(xyz), perturbed(f.T_G_C)

    def t_device(n, T0, cfg=ac):
        g.synchronize()
        t0 = time.perf_counter()
        chk(L.ks_align_points_device(g._h, T0.ctypes.data, d_xyz.data_ptr(), n, C.byref(cfg), out7.ctypes.data, C.byref(st)))
        return time.perf_counter() - t0

    def t_host(n, T0):
        g.synchronize()
        t0 = time.perf_counter()
        chk(L.ks_align_points(g._h, T0.ctypes.data, p_xyz, n, C.byref(ac), out7.ctypes.data, C.byref(st)))
        return time.perf_counter() - t0

    def t_events(n, T0, iterations):
        cfg = g.align_config(max_iterations=iterations, eps_rotation_rad=0.0, eps_translation_m=0.0)
        g.synchronize()
        ev0.record(stream)
        chk(L.ks_align_points_device(g._h, T0.ctypes.data, d_xyz.data_ptr(), n, C.byref(cfg), out7.ctypes.data, C.byref(st)))
        ev1.record(stream)
        ev1.synchronize()
        assert st.iterations == iterations, (st.status, st.iterations)
        return ev0.elapsed_time(ev1) * 1e-3

    def t_layers():
        g.synchronize()
        t0 = time.perf_counter()
        chk(L.ks_download_blocks(g._h, blocks.ctypes.data, len(blocks), p_tsdf, p_sem))
        return time.perf_counter() - t0

    got = dict(device=[], host=[], pair=[], layers=[], iterations=[], inlier_fraction=[], err_t0=[], err_r0=[], err_t=[], err_r=[], points=[], status=[])
    for r in range(a.warmup + a.reps):
        f = ring[(r * 7) % len(ring)]
        n, T0 = stage(f)
        one = {}
        for what in (("device", "pair", "host", "layers") if r % 2 == 0 else ("layers", "host", "pair", "device")):
            if what == "device":
                one["device"] = t_device(n, T0)
                one["iterations"], one["status"], one["points"] = int(st.iterations), int(st.status), int(st.points_used)
                one["inlier_fraction"] = st.inliers_first / float(max(st.points_used, 1))
                (one["err_t0"], one["err_r0"]), (one["err_t"], one["err_r"]) = pose_error(T0, f.T_G_C), pose_error(out7, f.T_G_C)
            elif what == "pair":
                one["pair"] = (t_events(n, T0, 20) - t_events(n, T0, 4)) / 16.0
            elif what == "host":
                one["host"] = t_host(n, T0)
            else:
                one["layers"] = t_layers()
        if r >= a.warmup:
            for k, v in one.items():
                got[k].append(v)
    m = statistics.median
    out = {
        "workload": "C2", "frames_integrated": len(ring), "reps": a.reps, "warmup": a.warmup, "width": w, "height": h,
        "map": {"tiles": tiles, "blocks": int(len(blocks)), "voxels_per_side": g.vps, "layer_bytes": int(len(blocks)) * nv * 104},
        "config": {k: getattr(ac, k) for k, _ in B.KsAlignConfig._fields_},
        "points_used_median": int(m(got["points"])),
        "i_align_device_cloud_ms": med(got["device"]),
        "ii_align_host_cloud_ms": med(got["host"]),
        "iii_kernel_pair_ms_device_events": med(got["pair"]),
        "iv_ks_download_blocks_ms": med(got["layers"]),
        "layer_download_over_align_device": round(m(got["layers"]) / (m(got["device"]) or 1.0), 2),
        "iterations": {"median": m(got["iterations"]), "min": min(got["iterations"]), "max": max(got["iterations"])},
        "status_counts": {str(s): got["status"].count(s) for s in sorted(set(got["status"]))},
        "inlier_fraction_median": round(m(got["inlier_fraction"]), 4),
        "pose_error_m_deg": {"start": [round(m(got["err_t0"]), 5), round(m(got["err_r0"]), 4)], "end_median": [round(m(got["err_t"]), 5), round(m(got["err_r"]), 4)]},
        "points_per_second_of_pair": round(m(got["points"]) / (m(got["pair"]) or 1.0), 0),
        "note": "wall-clock around synchronous calls except the kernel pair (device events on the context's stream), candidates alternating in "
                "one process; (iv) is existing code, unchanged by the alignment",
    }
    for p in (p_xyz, p_tsdf, p_sem):
        L.ks_host_free(p)
    g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
