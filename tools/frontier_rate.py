#!/usr/bin/env python3
"""Rates of the exploration frontiers (ks_frontiers_update, ks_frontiers_download, ks_frontiers_download_blocks) beside the downloads
a host pass needs before it can look at a voxel.  On the map the headline of bench.py builds (the C2 ring: the map of
tools/nav_rate.py) after one ks_esdf_update with the default configuration and one ks_nav_update (radius 0.3 m, one goal at the last
camera position), in ONE process, the candidates alternating, the median of --reps repetitions after warm-up, wall clock around
synchronous calls:
  (1) ks_frontiers_update (statistics included: the call waits for them)
  (2) update + ks_frontiers_download: what an explorer that ranks records needs
  (3) update + records + ks_frontiers_download_blocks of every block of the map into page-locked memory
  (4) ks_esdf_download_blocks + ks_nav_download_blocks of every block, the same way: the transfers a host pass needs first, and the
      yardstick (its neighbourhood test, clustering and join are not counted at all)
No ratio is set in advance and nothing is gated on these numbers.  Not measured: other maps, the C4 workload, more than one GPU.
Without a GPU there is no rate to report: the tool says so, writes nothing and exits with status 1.  Writes profiles/frontier_rate.json (or --out)."""
import argparse
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
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--min-voxels", type=int, default=8)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("frontier_rate: no GPU here, so there is no rate to report; nothing written", file=sys.stderr)
        return 1
    import bench  # (the workloads and the integrator configuration of the headline)
    from kimera_semantics_amd import binding as B
    wl = bench.WORKLOADS["C2"]
    g = B.HipIntegrator(B.default_config(max_tiles=1 << 13, max_points=wl["w"] * wl["h"], pipeline_frames=0, **bench.integ_cfg(wl)))
    last = None
    for f in bench.make_frames(wl, range(a.frames)):
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        last = f
    g.synchronize()
    esdf = g.esdf_update()
    idx = g.block_indices()
    vps = g.vps
    goal = np.asarray(last.T_G_C[4:7], np.float32).reshape(1, 3)
    nav = g.nav_update(goal, radius_m=a.radius)
    rec, stats = g.frontiers(radius_m=a.radius, min_voxels=a.min_voxels)
    nv = vps ** 3
    esdf_bytes, word_bytes = len(idx) * nv * 8, len(idx) * nv * 4
    L = B.lib()
    pinned = L.ks_host_alloc(esdf_bytes)
    assert pinned, "ks_host_alloc failed"
    cfg, st = g.frontier_config(radius_m=a.radius, min_voxels=a.min_voxels), B.KsFrontierStats()
    out_rec = np.zeros(len(rec), B.FRONTIER_DTYPE)
    import ctypes
    n = ctypes.c_size_t()

    def timed(call):
        g.synchronize()
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e3

    def update():
        g._chk(L.ks_frontiers_update(g._h, ctypes.byref(cfg), ctypes.byref(st)))

    def records():
        update()
        g._chk(L.ks_frontiers_download(g._h, out_rec.ctypes.data, len(out_rec), ctypes.byref(n)))

    def everything():
        records()
        g._chk(L.ks_frontiers_download_blocks(g._h, idx.ctypes.data, len(idx), pinned))

    def host_inputs():
        g._chk(L.ks_esdf_download_blocks(g._h, idx.ctypes.data, len(idx), pinned))
        g._chk(L.ks_nav_download_blocks(g._h, idx.ctypes.data, len(idx), pinned))

    candidates = {"frontiers_update": update, "update_and_records": records, "update_records_and_ids": everything, "esdf_and_nav_download_blocks": host_inputs}
    names = list(candidates)
    got = {k: [] for k in names}
    for r in range(a.warmup + a.reps):
        for k in (names if r % 2 == 0 else names[::-1]):
            ms = timed(candidates[k])
            if r >= a.warmup:
                got[k].append(ms)
    assert out_rec.tobytes() == rec.tobytes(), "the records changed between two updates of the same store"
    model_ms = None
    if not a.no_model:
        from tests import esdf_read_model, frontier_model, nav_model
        store = esdf_read_model.store_of(g)            # (the download and the dense arrays are not timed)
        field = nav_model.field(store, goal, float(g.cfg.voxel_size), radius_m=a.radius)
        t0 = time.perf_counter()
        model = frontier_model.frontiers(store, field, radius_m=a.radius, min_voxels=a.min_voxels, vps=vps)
        model_ms = round((time.perf_counter() - t0) * 1e3, 1)
        frontier_model.assert_same((rec, stats), model, idx, g.frontier_ids(idx), "frontier_rate")
    ms = {k: med(v) for k, v in got.items()}
    out = {
        "workload": "C2", "frames_integrated": a.frames, "reps": a.reps, "warmup": a.warmup,
        "map": {"tiles": len(g.tile_keys()), "blocks": int(len(idx)), "esdf": esdf, "esdf_bytes_all_blocks": esdf_bytes, "nav_bytes_all_blocks": word_bytes,
                "id_bytes_all_blocks": word_bytes, "record_bytes": int(len(rec)) * 88},
        "inputs": {"radius_m": a.radius, "min_voxels": a.min_voxels, "goals": 1},
        "nav": nav, "frontiers": stats, "reached_by_the_field": int((rec["nav_cost"] <= B.KS_NAV_MAX_COST).sum()),
        "ms": ms,
        "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in got.items()},
        "rates": {"frontiers_update_Mvoxels_of_the_store_per_s": round(len(g.tile_keys()) * 512 / ms["frontiers_update"] * 1e-3, 1),
                  "esdf_and_nav_download_GB_per_s": round((esdf_bytes + word_bytes) / ms["esdf_and_nav_download_blocks"] * 1e-6, 2)},
        "host_model_ms_once": model_ms,
        "not_measured": ["other maps", "the C4 workload", "more than one GPU", "the host pass itself (neighbour test, clustering, join) that would follow the downloads"],
        "note": "wall clock around synchronous calls, the block downloads into page-locked memory, the records into a pageable NumPy array; candidates "
                "alternating in one process; host_model_ms_once is the NumPy model of tests/frontier_model.py on the same store, run once, not a yardstick",
    }
    L.ks_host_free(pinned)
    g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
