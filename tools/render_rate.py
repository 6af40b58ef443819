#!/usr/bin/env python3
"""Rate of the on-device view renderer (ks_render_view) beside what a host renderer needs first, the layer download.
On the map the headline of bench.py builds (the C2 ring), 640 x 480, from the ring's own poses and intrinsics, in ONE process,
candidates alternating, the median of --reps repetitions after warm-up, the context synchronised before every timed call:
  (i)   ks_render_view_device, all four images into device buffers, stats read back (one kernel + an 24-byte copy) — and the
        kernel alone from device events around the enqueue with stats = NULL
  (ii)  ks_render_view of depth and labels into page-locked memory (the call plus the download of the two images)
  (iii) ks_download_blocks of every block (TSDF + semantic layer) into page-locked memory: what a host ray-caster waits for
and samples per pixel of every view.  There is no pass mark.  Writes profiles/render_rate.json (or --out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workloads and the integrator configuration of the headline)
from kimera_semantics_amd import binding as B  # noqa: E402


def med(xs):
    return round(statistics.median(xs) * 1e3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40, help="frames of the ring integrated before anything is measured")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_rate.json"))
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
    n = w * h

    def pinned(nbytes):
        p = L.ks_host_alloc(max(int(nbytes), 1))
        assert p, "ks_host_alloc failed"
        return p

    p_depth, p_labels = pinned(4 * n), pinned(n)
    p_tsdf, p_sem = pinned(len(blocks) * nv * 12), pinned(len(blocks) * nv * 92)
    d_depth = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    d_labels = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    d_rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    d_normals = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc, st = g.render_config(), B.KsRenderStats()
    stream = torch.cuda.ExternalStream(g.stream)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def args_of(f):
        import numpy as np
        return np.ascontiguousarray(f.T_G_C, np.float32), np.ascontiguousarray(f.K, np.float32)

    def t_device(f):
        T, K = args_of(f)
        g.synchronize()
        t0 = time.perf_counter()
        chk(L.ks_render_view_device(g._h, T.ctypes.data, K.ctypes.data, w, h, C.byref(rc), d_depth.data_ptr(), d_labels.data_ptr(),
                                    d_rgba.data_ptr(), d_normals.data_ptr(), C.byref(st)))
        dt = time.perf_counter() - t0
        return dt, int(st.samples), int(st.pixels_hit)

    def t_kernel(f):
        T, K = args_of(f)
        g.synchronize()
        ev0.record(stream)
        chk(L.ks_render_view_device(g._h, T.ctypes.data, K.ctypes.data, w, h, C.byref(rc), d_depth.data_ptr(), d_labels.data_ptr(),
                                    d_rgba.data_ptr(), d_normals.data_ptr(), None))
        ev1.record(stream)
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e-3

    def t_host(f):
        T, K = args_of(f)
        g.synchronize()
        t0 = time.perf_counter()
        chk(L.ks_render_view(g._h, T.ctypes.data, K.ctypes.data, w, h, C.byref(rc), p_depth, p_labels, None, None, None))
        return time.perf_counter() - t0

    def t_layers():
        g.synchronize()
        t0 = time.perf_counter()
        chk(L.ks_download_blocks(g._h, blocks.ctypes.data, len(blocks), p_tsdf, p_sem))
        return time.perf_counter() - t0

    got = dict(device=[], kernel=[], host=[], layers=[], samples_per_pixel=[], hit_fraction=[])
    for r in range(a.warmup + a.reps):
        f = ring[(r * 7) % len(ring)]
        one = {}
        for what in (("device", "kernel", "host", "layers") if r % 2 == 0 else ("layers", "host", "kernel", "device")):
            if what == "device":
                one["device"], s, hit = t_device(f)
                one["samples_per_pixel"], one["hit_fraction"] = s / float(n), hit / float(n)
            elif what == "kernel":
                one["kernel"] = t_kernel(f)
            elif what == "host":
                one["host"] = t_host(f)
            else:
                one["layers"] = t_layers()
        if r >= a.warmup:
            for k, v in one.items():
                got[k].append(v)
    out = {
        "workload": "C2", "frames_integrated": len(ring), "reps": a.reps, "warmup": a.warmup, "width": w, "height": h,
        "map": {"tiles": tiles, "blocks": int(len(blocks)), "voxels_per_side": g.vps, "layer_bytes": int(len(blocks)) * nv * 104},
        "config": {"min_weight": rc.min_weight, "min_range_m": rc.min_range_m, "max_range_m": rc.max_range_m},
        "i_render_device_four_images_with_stats_ms": med(got["device"]),
        "i_kernel_ms_device_events": med(got["kernel"]),
        "ii_render_host_depth_and_labels_ms": med(got["host"]),
        "iii_ks_download_blocks_ms": med(got["layers"]),
        "samples_per_pixel": {"median": round(statistics.median(got["samples_per_pixel"]), 2), "min": round(min(got["samples_per_pixel"]), 2),
                              "max": round(max(got["samples_per_pixel"]), 2)},
        "hit_fraction_median": round(statistics.median(got["hit_fraction"]), 4),
        "samples_per_second_of_kernel": round(statistics.median(got["samples_per_pixel"]) * n / (statistics.median(got["kernel"]) or 1.0), 0),
        "note": "wall-clock around synchronous calls except the kernel (device events on the context's stream), candidates alternating in one "
                "process; (iii) is existing code, unchanged by the renderer",
    }
    for p in (p_depth, p_labels, p_tsdf, p_sem):
        L.ks_host_free(p)
    g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
