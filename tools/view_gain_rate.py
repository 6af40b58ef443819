#!/usr/bin/env python3
"""Rates of the view information gain (ks_view_gain, ks_view_gain_device) beside the download a host ray caster waits for before it
can cast a ray.  On the map the headline of bench.py builds (the C2 ring: the map of tools/frontier_rate.py) after ks_esdf_update,
ks_nav_update and ks_frontiers_update with their defaults, in ONE process, the candidates alternating, the median of --reps
repetitions after warm-up.  The views are the centres of the frontiers' nav_voxel and the ring's camera positions, each at 8 yaws,
repeated to --views (1024); 32 x 24 rays of a 90-degree image each, 5 m range, the other options default:
  (i)   ks_view_gain_device: the kernel pair from device events on ks_stream(ctx) around the enqueue (stats = NULL: no host wait
        inside the call), and the call with stats (wall clock: it waits)
  (ii)  ks_view_gain end to end: poses from the host, records on the host
  (iii) ks_esdf_download_blocks of every block into page-locked memory: the transfer a host ray caster needs first, and the
        yardstick (its ray casting is not counted at all)
  (iv)  the same views in a second context made under KS_DEBUG=1 KS_VG_LDS_BITS=0: every bitmap in global memory; and, because a
        90-degree view of 5 m is a box of some millions of voxels that no LDS budget holds, both contexts again on the same poses with
        a 60-degree image and --short-range (3 m), where most boxes fit
No ratio is set in advance and nothing is gated on these numbers.  Not measured: other maps, the C4 workload, a wavefront per ray,
more than one GPU.  Without a GPU there is no rate to report: the tool says so, writes nothing and exits with status 1.
Writes profiles/view_gain_rate.json (or --out)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(xs):
    return round(statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40, help="frames of the C2 ring integrated before anything is measured")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", type=int, default=1024)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--height", type=int, default=24)
    ap.add_argument("--max-range", type=float, default=5.0)
    ap.add_argument("--short-range", type=float, default=3.0, help="the range of the 60-degree views of (iv)")
    ap.add_argument("--model-views", type=int, default=16, help="views checked against the NumPy model, once (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_gain_rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("view_gain_rate: no GPU here, so there is no rate to report; nothing written", file=sys.stderr)
        return 1
    import bench  # (the workloads and the integrator configuration of the headline)
    from kimera_semantics_amd import binding as B
    wl = bench.WORKLOADS["C2"]
    frames = bench.make_frames(wl, range(a.frames))

    def mapped(**env):
        before = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            g = B.HipIntegrator(B.default_config(max_tiles=1 << 13, max_points=wl["w"] * wl["h"], pipeline_frames=0, **bench.integ_cfg(wl)))
        finally:
            for k, v in before.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        for f in frames:
            g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        g.synchronize()
        return g, g.esdf_update()

    g, esdf = mapped()
    idx = g.block_indices()
    goal = np.asarray(frames[-1].T_G_C[4:7], np.float32).reshape(1, 3)
    g.nav_update(goal)
    rec_fr, st_fr = g.frontiers()
    at = np.concatenate([B.frontier_targets(rec_fr, g.cfg.voxel_size), np.array([f.T_G_C[4:7] for f in frames], np.float32)])
    poses = B.view_gain_yaw_poses(at, 8)
    distinct = len(poses)
    poses = np.ascontiguousarray(np.resize(poses, (a.views, 7)))
    w, h = a.width, a.height
    K = (0.5 * w, 0.5 * w, (w - 1) / 2, (h - 1) / 2)             # 90 degrees across the image
    cfg = dict(max_range_m=a.max_range)
    rec, stats = g.view_gain(poses, K, w, h, **cfg)
    g0, _ = mapped(KS_DEBUG="1", KS_VG_LDS_BITS="0")
    rec0, stats0 = g0.view_gain(poses, K, w, h, **cfg)
    assert rec0.tobytes() == rec.tobytes() and stats0["views_in_lds"] == 0, "the two paths disagree"
    L = B.lib()
    esdf_bytes = len(idx) * g.vps ** 3 * 8
    pinned = L.ks_host_alloc(esdf_bytes)
    assert pinned, "ks_host_alloc failed"
    d_poses = torch.from_numpy(poses).to("cuda")
    d_out = torch.zeros((a.views, 8), dtype=torch.int32, device="cuda")
    out = np.zeros(a.views, B.VIEW_GAIN_DTYPE)
    vc, st = g.view_gain_config(K, w, h, **cfg), B.KsViewGainStats()
    K60 = (0.5 * w / np.tan(np.radians(30.0)), 0.5 * w / np.tan(np.radians(30.0)), (w - 1) / 2, (h - 1) / 2)
    short = dict(max_range_m=a.short_range)
    vc60 = g.view_gain_config(K60, w, h, **short)
    rec60, stats60 = g.view_gain(poses, K60, w, h, **short)
    rec60_0, stats60_0 = g0.view_gain(poses, K60, w, h, **short)
    assert rec60.tobytes() == rec60_0.tobytes() and stats60_0["views_in_lds"] == 0, "the two paths disagree on the short views"
    torch.cuda.synchronize()

    def device_events(ctx, vc=vc):
        stream = torch.cuda.ExternalStream(ctx.stream)

        def run():
            ctx.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx._chk(L.ks_view_gain_device(ctx._h, d_poses.data_ptr(), a.views, ctypes.byref(vc), d_out.data_ptr(), None))
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run

    def wall(call):
        def run():
            g.synchronize()
            t0 = time.perf_counter()
            call()
            return (time.perf_counter() - t0) * 1e3
        return run

    candidates = {
        "kernels_device_events": device_events(g),
        "kernels_device_events_global_bitmaps": device_events(g0),
        "short_views_kernels_device_events": device_events(g, vc60),
        "short_views_kernels_device_events_global_bitmaps": device_events(g0, vc60),
        "device_call_with_stats": wall(lambda: g._chk(L.ks_view_gain_device(g._h, d_poses.data_ptr(), a.views, ctypes.byref(vc), d_out.data_ptr(), ctypes.byref(st)))),
        "host_call_end_to_end": wall(lambda: g._chk(L.ks_view_gain(g._h, poses.ctypes.data, a.views, ctypes.byref(vc), out.ctypes.data, ctypes.byref(st)))),
        "esdf_download_blocks": wall(lambda: g._chk(L.ks_esdf_download_blocks(g._h, idx.ctypes.data, len(idx), pinned))),
    }
    names = list(candidates)
    got = {k: [] for k in names}
    for r in range(a.warmup + a.reps):
        for k in (names if r % 2 == 0 else names[::-1]):
            ms = candidates[k]()
            if r >= a.warmup:
                got[k].append(ms)
    torch.cuda.synchronize()
    assert out.tobytes() == rec.tobytes(), "the records changed between two calls on the same store"
    if a.model_views:
        from tests import view_gain_model
        pick = np.linspace(0, distinct - 1, min(a.model_views, distinct)).astype(int)
        want, _ = view_gain_model.model_of(g, poses[pick], K, width=w, height=h, **cfg)
        assert rec[pick].tobytes() == want.tobytes(), "the records differ from the model"
    ms = {k: med(v) for k, v in got.items()}
    valid = max(stats["views_valid"], 1)
    out_json = {
        "workload": "C2", "frames_integrated": a.frames, "reps": a.reps, "warmup": a.warmup,
        "map": {"tiles": len(g.tile_keys()), "blocks": int(len(idx)), "esdf": esdf, "esdf_bytes_all_blocks": esdf_bytes, "frontiers": st_fr["frontiers"]},
        "inputs": {"views": a.views, "distinct_views": min(distinct, a.views), "width": w, "height": h, "max_range_m": a.max_range,
                   "samples_per_ray_at_most": int(np.floor(np.float32(a.max_range) / np.float32(g.cfg.voxel_size))) + 1, "record_bytes": a.views * 32},
        "view_gain": stats, "samples_per_view": round(stats["samples"] / valid, 1), "unknown_voxels_per_view": round(stats["unknown_voxels"] / valid, 1),
        "views_in_lds": stats["views_in_lds"],
        "short_views": {"fov_deg": 60.0, "max_range_m": a.short_range, "view_gain": stats60, "views_in_lds": stats60["views_in_lds"],
                        "samples_per_view": round(stats60["samples"] / max(stats60["views_valid"], 1), 1)},
        "ms": ms,
        "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in got.items()},
        "rates": {"views_per_s_kernels": round(a.views / ms["kernels_device_events"] * 1e3),
                  "Msamples_per_s_kernels": round(stats["samples"] / ms["kernels_device_events"] * 1e-3, 1),
                  "esdf_download_GB_per_s": round(esdf_bytes / ms["esdf_download_blocks"] * 1e-6, 2)},
        "views_checked_against_the_model": int(min(a.model_views, distinct)),
        "not_measured": ["other maps", "the C4 workload", "a wavefront per ray (the kernel takes a lane per ray)", "more than one GPU",
                         "the host ray caster that would follow the download"],
        "note": "kernels_*: events on ks_stream around the enqueue of ks_view_gain_device with stats = NULL (counter memset + k_vg_planes + k_vg_walk); the "
                "others wall clock around synchronous calls, the block download into page-locked memory; candidates alternating in one process; "
                "*_global_bitmaps: a second context over the same frames made under KS_DEBUG=1 KS_VG_LDS_BITS=0",
    }
    L.ks_host_free(pinned)
    g.close()
    g0.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out_json, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out_json))
    return 0


if __name__ == "__main__":
    sys.exit(main())
