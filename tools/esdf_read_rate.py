#!/usr/bin/env python3
"""Rates of the planner reads of the stored ESDF (ks_esdf_sample, ks_esdf_slice, ks_esdf_sweep) beside the download a host planner
needs before its first lookup.  On the map the headline of bench.py builds (the C2 ring: the map of tools/mesh_rate.py) after one
ks_esdf_update with the default configuration, in ONE process, the candidates alternating, the median of --reps repetitions after
warm-up:
  (1) the device entries, timed with events on ks_stream(ctx) around the enqueue (stats = NULL: no host wait inside the call):
      10^6 random points in the map's bounding box, 10^5 segments of 1 - 3 m that start in it, a 640 x 480 horizontal slice
  (2) the host entries end to end (wall clock: staging in, kernel, every output copied out)
  (3) ks_esdf_download_blocks of every block of the map (wall clock, into page-locked memory)
Nothing is gated on these numbers.  Writes profiles/esdf_read_rate.json (or --out)."""
import argparse
import json
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
    return round(statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40, help="frames of the C2 ring integrated before anything is measured")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=10 ** 6)
    ap.add_argument("--segments", type=int, default=10 ** 5)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esdf_read_rate.json"))
    a = ap.parse_args()
    import torch
    wl = bench.WORKLOADS["C2"]
    g = B.HipIntegrator(B.default_config(max_tiles=1 << 13, max_points=wl["w"] * wl["h"], pipeline_frames=0, **bench.integ_cfg(wl)))
    for f in bench.make_frames(wl, range(a.frames)):
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.synchronize()
    esdf = g.esdf_update()
    idx = g.block_indices()
    vs, vps = float(g.cfg.voxel_size), g.vps
    lo, hi = idx.min(axis=0) * vps * vs, (idx.max(axis=0) + 1) * vps * vs
    rng = np.random.default_rng(1)
    xyz = rng.uniform(lo, hi, (a.points, 3)).astype(np.float32)
    s0 = rng.uniform(lo, hi, (a.segments, 3))
    d = rng.normal(size=(a.segments, 3))
    seg = np.concatenate([s0, s0 + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(1.0, 3.0, (a.segments, 1))], axis=1).astype(np.float32)
    w, h = 640, 480
    z = float(0.5 * (lo[2] + hi[2]))
    o, du, dv = np.array([lo[0], lo[1], z], np.float32), np.array([(hi[0] - lo[0]) / w, 0, 0], np.float32), np.array([0, (hi[1] - lo[1]) / h, 0], np.float32)

    dev = lambda arr: torch.from_numpy(arr).to("cuda")
    empty = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
    d_xyz, d_seg = dev(xyz), dev(seg)
    n, m, px = a.points, a.segments, w * h
    pt = [empty((n,), torch.float32), empty((n, 3), torch.float32), empty((n,), torch.uint8), empty((n,), torch.uint8), empty((n,), torch.uint8)]
    im = [empty((px,), torch.float32), empty((px, 3), torch.float32), empty((px,), torch.uint8), empty((px,), torch.uint8), empty((px,), torch.uint8)]
    sw = [empty((m,), torch.uint8), empty((m,), torch.float32), empty((m,), torch.float32), empty((m,), torch.float32)]
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(g.stream)
    nbytes = len(idx) * vps ** 3 * 8
    pinned = B.lib().ks_host_alloc(nbytes)
    assert pinned, "ks_host_alloc failed"

    def timed_device(call):
        g.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed_host(call):
        g.synchronize()
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e3

    def download():
        g._chk(B.lib().ks_esdf_download_blocks(g._h, idx.ctypes.data, len(idx), pinned))

    candidates = {
        "sample_device": lambda: timed_device(lambda: g.esdf_sample_device(d_xyz.data_ptr(), n, *[t.data_ptr() for t in pt], stats=False)),
        "sweep_device": lambda: timed_device(lambda: g.esdf_sweep_device(d_seg.data_ptr(), m, *[t.data_ptr() for t in sw], stats=False, radius_m=a.radius)),
        "slice_device": lambda: timed_device(lambda: g.esdf_slice_device(o, du, dv, w, h, *[t.data_ptr() for t in im], stats=False)),
        "sample_host": lambda: timed_host(lambda: g.esdf_sample(xyz, stats=False)),
        "sweep_host": lambda: timed_host(lambda: g.esdf_sweep(seg, stats=False, radius_m=a.radius)),
        "slice_host": lambda: timed_host(lambda: g.esdf_slice(o, du, dv, w, h, stats=False)),
        "download_blocks": lambda: timed_host(download),
    }
    names = list(candidates)
    got = {k: [] for k in names}
    for r in range(a.warmup + a.reps):
        for k in (names if r % 2 == 0 else names[::-1]):
            ms = candidates[k]()
            if r >= a.warmup:
                got[k].append(ms)
    st_p = g.esdf_sample_device(d_xyz.data_ptr(), n, pt[0].data_ptr())
    st_s = g.esdf_sweep_device(d_seg.data_ptr(), m, sw[0].data_ptr(), radius_m=a.radius)
    st_i = g.esdf_slice_device(o, du, dv, w, h, im[0].data_ptr())
    ms = {k: med(v) for k, v in got.items()}
    out = {
        "workload": "C2", "frames_integrated": a.frames, "reps": a.reps, "warmup": a.warmup,
        "map": {"tiles": len(g.tile_keys()), "blocks": int(len(idx)), "esdf": esdf, "esdf_bytes_all_blocks": nbytes},
        "inputs": {"points": n, "segments": m, "segment_length_m": [1.0, 3.0], "radius_m": a.radius, "slice": [w, h]},
        "stats": {"sample": st_p, "sweep": st_s, "slice": st_i},
        "ms": ms,
        "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in got.items()},
        "rates": {"sample_device_Mpoints_per_s": round(n / ms["sample_device"] * 1e-3, 1), "sample_host_Mpoints_per_s": round(n / ms["sample_host"] * 1e-3, 2),
                  "sweep_device_Msegments_per_s": round(m / ms["sweep_device"] * 1e-3, 2), "sweep_device_Msamples_per_s": round(st_s["samples"] / ms["sweep_device"] * 1e-3, 1),
                  "sweep_host_Msegments_per_s": round(m / ms["sweep_host"] * 1e-3, 2), "slice_device_Mpixels_per_s": round(px / ms["slice_device"] * 1e-3, 1),
                  "download_GB_per_s": round(nbytes / ms["download_blocks"] * 1e-6, 2)},
        "note": "device entries: events on ks_stream around the enqueue (counter memset + kernel); host entries and the download: wall clock around "
                "synchronous calls (the host entries into pageable NumPy arrays, the download into page-locked memory); candidates alternating in one process",
    }
    B.lib().ks_host_free(pinned)
    g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
