#!/usr/bin/env python3
"""Rates of the navigation field (ks_nav_update, ks_nav_paths, ks_nav_download_blocks) beside the download a host planner needs
before it can start.  On the map the headline of bench.py builds (the C2 ring: the map of tools/mesh_rate.py) after one
ks_esdf_update with the default configuration (2 m reach), radius 0.3 m, one goal at the last camera position, in ONE process, the
candidates alternating, the median of --reps repetitions after warm-up:
  (1) ks_nav_update end to end (wall clock: the goals in, every round, the host's reads of the list count, the closing pass), with
      its rounds and tile relaxations; the host reads follow from the rounds (one before the first group of 16 and one after each)
  (2) ks_nav_paths for 10^4 starts drawn from the traversable voxels: the device entry timed with events on ks_stream(ctx) around
      the enqueue (stats = NULL: no host wait inside the call), and the host entry end to end
  (3) ks_nav_download_blocks of every block of the map (wall clock, into page-locked memory)
  (4) ks_esdf_download_blocks of every block, the same way: the transfer a host planner needs first, and the yardstick
The NumPy model's own time for the same field is noted once (--no-model skips it); it is not a yardstick.  Nothing is gated on these
numbers.  Writes profiles/nav_rate.json (or --out)."""
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

ROUNDS_PER_READ = 16   # kNavRoundsPerRead of ks_hip.hip


def med(xs):
    return round(statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40, help="frames of the C2 ring integrated before anything is measured")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--starts", type=int, default=10 ** 4)
    ap.add_argument("--max-waypoints", type=int, default=1024)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nav_rate.json"))
    a = ap.parse_args()
    import torch
    wl = bench.WORKLOADS["C2"]
    g = B.HipIntegrator(B.default_config(max_tiles=1 << 13, max_points=wl["w"] * wl["h"], pipeline_frames=0, **bench.integ_cfg(wl)))
    last = None
    for f in bench.make_frames(wl, range(a.frames)):
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        last = f
    g.synchronize()
    esdf = g.esdf_update()
    idx = g.block_indices()
    vs, vps = float(g.cfg.voxel_size), g.vps
    goal = np.asarray(last.T_G_C[4:7], np.float32).reshape(1, 3)
    field_stats = g.nav_update(goal, radius_m=a.radius)
    blocks = g.nav_blocks(idx)
    rng = np.random.default_rng(1)
    free = np.argwhere(blocks != B.KS_NAV_BLOCKED)
    pick = free[rng.choice(len(free), a.starts, replace=len(free) < a.starts)]
    local = np.stack([pick[:, 1] % vps, (pick[:, 1] // vps) % vps, pick[:, 1] // (vps * vps)], axis=1)
    starts = ((idx[pick[:, 0]].astype(np.int64) * vps + local + 0.5) * vs).astype(np.float32)
    n, mw = a.starts, a.max_waypoints

    d_starts = torch.from_numpy(starts).to("cuda")
    d_out = [torch.empty((n,), dtype=torch.uint8, device="cuda"), torch.empty((n,), dtype=torch.int32, device="cuda"),
             torch.empty((n,), dtype=torch.int32, device="cuda"), torch.empty((n, mw, 3), dtype=torch.float32, device="cuda")]
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(g.stream)
    nv = vps ** 3
    esdf_bytes, nav_bytes = len(idx) * nv * 8, len(idx) * nv * 4
    pinned = B.lib().ks_host_alloc(esdf_bytes)
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

    schedule = []

    def update():
        st = g.nav_update(goal, radius_m=a.radius)
        schedule.append((st["rounds"], st["tile_relaxations"]))

    candidates = {
        "nav_update": lambda: timed_host(update),
        "paths_device": lambda: timed_device(lambda: g.nav_paths_device(d_starts.data_ptr(), n, mw, *[t.data_ptr() for t in d_out], stats=False)),
        "paths_host": lambda: timed_host(lambda: g.nav_paths(starts, mw, stats=False)),
        "nav_download_blocks": lambda: timed_host(lambda: g._chk(B.lib().ks_nav_download_blocks(g._h, idx.ctypes.data, len(idx), pinned))),
        "esdf_download_blocks": lambda: timed_host(lambda: g._chk(B.lib().ks_esdf_download_blocks(g._h, idx.ctypes.data, len(idx), pinned))),
    }
    names = list(candidates)
    got = {k: [] for k in names}
    for r in range(a.warmup + a.reps):
        for k in (names if r % 2 == 0 else names[::-1]):
            ms = candidates[k]()
            if r >= a.warmup:
                got[k].append(ms)
    path_stats = g.nav_paths_device(d_starts.data_ptr(), n, mw, d_out[0].data_ptr())
    rounds = [s[0] for s in schedule[a.warmup:]]
    model_ms = None
    if not a.no_model:
        from tests import nav_model
        from tests import esdf_read_model
        store = esdf_read_model.store_of(g)            # (the download and the dense arrays are not timed)
        t0 = time.perf_counter()
        model = nav_model.field(store, goal, vs, radius_m=a.radius)
        model_ms = round((time.perf_counter() - t0) * 1e3, 1)
        assert model.blocks(idx, vps).tobytes() == g.nav_blocks(idx).tobytes(), "the field differs from the model"
    ms = {k: med(v) for k, v in got.items()}
    out = {
        "workload": "C2", "frames_integrated": a.frames, "reps": a.reps, "warmup": a.warmup,
        "map": {"tiles": len(g.tile_keys()), "blocks": int(len(idx)), "esdf": esdf, "esdf_bytes_all_blocks": esdf_bytes, "nav_bytes_all_blocks": nav_bytes},
        "inputs": {"radius_m": a.radius, "goals": 1, "starts": n, "max_waypoints": mw},
        "field": field_stats, "paths": path_stats,
        "schedule": {"rounds_median": statistics.median(rounds), "rounds_min_max": [min(rounds), max(rounds)],
                     "tile_relaxations_median": statistics.median(s[1] for s in schedule[a.warmup:]),
                     "host_reads_median": 1 + -(-int(statistics.median(rounds)) // ROUNDS_PER_READ), "rounds_per_host_read": ROUNDS_PER_READ},
        "ms": ms,
        "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in got.items()},
        "rates": {"nav_update_Mvoxels_traversable_per_s": round(field_stats["voxels_traversable"] / ms["nav_update"] * 1e-3, 1),
                  "paths_device_Mwaypoints_per_s": round(path_stats["waypoints"] / ms["paths_device"] * 1e-3, 2),
                  "nav_download_GB_per_s": round(nav_bytes / ms["nav_download_blocks"] * 1e-6, 2),
                  "esdf_download_GB_per_s": round(esdf_bytes / ms["esdf_download_blocks"] * 1e-6, 2)},
        "host_model_ms_once": model_ms,
        "note": "nav_update, the host path entry and both downloads: wall clock around synchronous calls (the downloads into page-locked memory, the host "
                "paths into pageable NumPy arrays); paths_device: events on ks_stream around the enqueue (counter memset + kernel); candidates "
                "alternating in one process; host_model_ms_once is the NumPy model of tests/nav_model.py on the same store, run once, not a yardstick",
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
