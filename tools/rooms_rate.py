#!/usr/bin/env python3
"""Rates of the rooms (ks_rooms_update, ks_rooms_download, ks_rooms_links_download, ks_rooms_download_blocks) beside the download a
host pass needs before it can look at a voxel.  On the map the headline of bench.py builds (the C2 ring: the map of the other rate
tools) after one ks_esdf_update with the default configuration (2 m reach) and one ks_objects_update, in ONE process, the candidates
alternating, the median of --reps repetitions after warm-up, wall clock around synchronous calls:
  (1) ks_rooms_update (statistics included: the call waits for them)
  (2) update + ks_rooms_download + ks_rooms_links_download: what a task planner that reads the graph needs
  (3) update + records + links + both planes of every block of the map into page-locked memory
  (4) ks_esdf_download_blocks of every block, the same way: the transfer a host pass needs first, and the yardstick (its connected
      components, its Dijkstra and its join are not counted at all)
No ratio is set in advance and nothing is gated on these numbers.  Not measured: other maps, the C4 workload, more than one GPU.
Without a GPU there is no rate to report: the tool says so, writes nothing and exits with status 1.  Writes profiles/rooms_rate.json (or --out)."""
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
    ap.add_argument("--free-distance", type=float, default=0.0)
    ap.add_argument("--core-distance", type=float, default=0.5)
    ap.add_argument("--min-core-voxels", type=int, default=64)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rooms_rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("rooms_rate: no GPU here, so there is no rate to report; nothing written", file=sys.stderr)
        return 1
    import bench  # (the workloads and the integrator configuration of the headline)
    from kimera_semantics_amd import binding as B
    wl = bench.WORKLOADS["C2"]
    g = B.HipIntegrator(B.default_config(max_tiles=1 << 13, max_points=wl["w"] * wl["h"], pipeline_frames=0, **bench.integ_cfg(wl)))
    for f in bench.make_frames(wl, range(a.frames)):
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.synchronize()
    esdf = g.esdf_update()
    _, objects = g.objects()
    idx = g.block_indices()
    vps = g.vps
    rc = dict(free_distance_m=a.free_distance, core_distance_m=a.core_distance, min_core_voxels=a.min_core_voxels)
    rec, links, stats = g.rooms(**rc)
    nv = vps ** 3
    esdf_bytes, word_bytes = len(idx) * nv * 8, len(idx) * nv * 4
    L = B.lib()
    pinned = L.ks_host_alloc(esdf_bytes)
    assert pinned, "ks_host_alloc failed"
    cfg, st = g.rooms_config(**rc), B.KsRoomsStats()
    out_rec, out_links = np.zeros(len(rec), B.ROOM_DTYPE), np.zeros(len(links), B.ROOM_LINK_DTYPE)
    n = ctypes.c_size_t()
    rounds, relaxations = [], []

    def timed(call):
        g.synchronize()
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e3

    def update():
        g._chk(L.ks_rooms_update(g._h, ctypes.byref(cfg), ctypes.byref(st)))
        rounds.append(int(st.rounds))
        relaxations.append(int(st.tile_relaxations))

    def graph():
        update()
        g._chk(L.ks_rooms_download(g._h, out_rec.ctypes.data, len(out_rec), ctypes.byref(n)))
        g._chk(L.ks_rooms_links_download(g._h, out_links.ctypes.data if len(out_links) else None, len(out_links), ctypes.byref(n)))

    def everything():
        graph()
        g._chk(L.ks_rooms_download_blocks(g._h, idx.ctypes.data, len(idx), pinned, pinned + word_bytes))

    def host_inputs():
        g._chk(L.ks_esdf_download_blocks(g._h, idx.ctypes.data, len(idx), pinned))

    candidates = {"rooms_update": update, "update_records_and_links": graph, "update_graph_and_both_planes": everything, "esdf_download_blocks": host_inputs}
    names = list(candidates)
    got = {k: [] for k in names}
    for r in range(a.warmup + a.reps):
        for k in (names if r % 2 == 0 else names[::-1]):
            ms = timed(candidates[k])
            if r >= a.warmup:
                got[k].append(ms)
    assert out_rec.tobytes() == rec.tobytes() and out_links.tobytes() == links.tobytes(), "the result changed between two updates of the same store"
    model_ms = None
    if not a.no_model:
        from tests import rooms_model
        t0 = time.perf_counter()
        model = rooms_model.model_of(g, **rc)              # (the downloads and the dense arrays are timed with it: run once, not a yardstick)
        model_ms = round((time.perf_counter() - t0) * 1e3, 1)
        rooms_model.assert_same((rec, links, stats), model, idx, g.room_ids(idx), g.room_costs(idx), "rooms_rate")
    ms = {k: med(v) for k, v in got.items()}
    out = {
        "workload": "C2", "frames_integrated": a.frames, "reps": a.reps, "warmup": a.warmup,
        "map": {"tiles": len(g.tile_keys()), "blocks": int(len(idx)), "esdf": esdf, "objects": objects, "esdf_bytes_all_blocks": esdf_bytes,
                "plane_bytes_all_blocks": 2 * word_bytes, "record_bytes": int(len(rec)) * 96, "link_bytes": int(len(links)) * 32},
        "inputs": rc,
        "rooms": stats, "rounds_min_max": [min(rounds), max(rounds)], "tile_relaxations_min_max": [min(relaxations), max(relaxations)],
        "ms": ms,
        "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in got.items()},
        "rates": {"rooms_update_Mvoxels_of_the_store_per_s": round(len(g.tile_keys()) * 512 / ms["rooms_update"] * 1e-3, 1),
                  "esdf_download_GB_per_s": round(esdf_bytes / ms["esdf_download_blocks"] * 1e-6, 2)},
        "host_model_ms_once": model_ms,
        "not_measured": ["other maps", "the C4 workload", "more than one GPU", "the host pass itself (components, Dijkstra, join) that would follow the download"],
        "note": "wall clock around synchronous calls, the block downloads into page-locked memory, records and links into pageable NumPy arrays; candidates "
                "alternating in one process; host_model_ms_once is the NumPy model of tests/rooms_model.py on the same store, run once, not a yardstick",
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
