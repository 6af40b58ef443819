#!/usr/bin/env python3
"""Rate of the on-device batch ESDF (ks_esdf_update) against what a host ESDF needs before it can start, the layer download.
On the map the headline of bench.py builds (the C2 ring), max_distance_m = 2.0, in ONE process, candidates alternating, the
median of --reps repetitions after warm-up, the context synchronised before every timed call (every timed call ends with a
stream synchronisation of its own):
  (1) ks_esdf_update alone
  (2) ... + ks_esdf_download_blocks of every block into page-locked memory
  (3) ks_download_blocks of every block (TSDF + semantic layer) into page-locked memory, as before this feature
  (4) the three passes' kernel times, from a kernel trace made in a run of its own:
        rocprofv3 --kernel-trace --stats -d DIR -- python tools/esdf_rate.py --trace-child
        python tools/esdf_rate.py --merge-kernel-stats DIR/**/*kernel_stats.csv
      with the box size and the fraction of the 8 TB/s roofline the box traffic of each pass amounts to.
  (5) the incremental refresh: one more frame of the ring is integrated (not timed), then ks_esdf_refresh is timed and after it
      a full ks_esdf_update of the same map, --reps times with a new frame each; the share of the tiles the refresh recomputed
      and its work space beside the medians.  (The order is fixed: an update before the refresh would leave it nothing to do.)
Nothing is gated on these numbers.  Writes profiles/esdf_rate.json (or --out)."""
import argparse
import csv
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

HBM_PEAK = 8e12
PASSES = {"k_esdf_x": "pass_x", "k_esdf_axis<0>": "pass_y", "k_esdf_axis<1>": "pass_z"}


def med(xs):
    return round(statistics.median(xs) * 1e3, 4)


def build_map(frames):
    wl = bench.WORKLOADS["C2"]
    ring = bench.make_frames(wl, range(frames))
    g = B.HipIntegrator(B.default_config(max_tiles=1 << 13, max_points=wl["w"] * wl["h"], pipeline_frames=0, **bench.integ_cfg(wl)))
    for f in ring:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.synchronize()
    return g


def esdf_config(a):
    ec = B.KsEsdfConfig()
    B.lib().ks_esdf_default_config(C.byref(ec))
    ec.max_distance_m, ec.min_distance_m = a.max_distance, a.min_distance
    return ec


def pass_traffic(box, tiles):
    """Bytes each pass moves at least: 16 bytes of keys per box voxel and direction; passes x and z also fetch the 128-byte
    line of every resident voxel's record, pass z writes its 8-byte result."""
    v = box[0] * box[1] * box[2]
    rec = tiles * 512 * 128
    return {"pass_x": rec + 16 * v, "pass_y": 32 * v, "pass_z": 16 * v + rec + tiles * 512 * 8}


def merge_kernel_stats(a):
    out = json.load(open(a.out))
    rows = {}
    for path in a.merge_kernel_stats:
        for row in csv.DictReader(open(path)):
            name = row.get("Name") or row.get("KernelName") or ""
            for k, p in PASSES.items():
                if k in name:
                    calls = int(row.get("Calls") or row.get("Count") or 0)
                    total = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0.0)
                    if calls:
                        rows[p] = {"calls": calls, "mean_ms": round(total / calls * 1e-6, 4)}
    traffic = pass_traffic(out["map"]["box_voxels"], out["map"]["tiles"])
    for p, r in rows.items():
        r["bytes"] = traffic[p]
        r["fraction_of_8TBs"] = round(traffic[p] / (r["mean_ms"] * 1e-3) / HBM_PEAK, 4)
    out["iv_kernel_trace"] = dict(rows, source="rocprofv3 --kernel-trace --stats, a run of its own (--trace-child)",
                                  dominant=max(rows, key=lambda p: rows[p]["mean_ms"]) if rows else None)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out["iv_kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40, help="frames of the C2 ring integrated before anything is measured")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-distance", type=float, default=2.0)
    ap.add_argument("--min-distance", type=float, default=0.2)
    ap.add_argument("--trace-child", action="store_true", help="build the map and run ks_esdf_update five times (for a kernel trace)")
    ap.add_argument("--merge-kernel-stats", nargs="+", metavar="CSV", help="fold the passes' times of a kernel trace into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esdf_rate.json"))
    a = ap.parse_args()
    if a.merge_kernel_stats:
        return merge_kernel_stats(a)
    L = B.lib()
    g = build_map(a.frames)
    chk = g._chk
    ec, st = esdf_config(a), B.KsEsdfStats()
    if a.trace_child:
        for _ in range(5):
            chk(L.ks_esdf_update(g._h, C.byref(ec), C.byref(st)))
        g.close()
        return
    blocks = g.block_indices()
    tiles = len(g.tile_keys())
    nv = g.vps ** 3

    def pinned(n):
        p = L.ks_host_alloc(max(int(n), 1))
        assert p, "ks_host_alloc failed"
        return p

    p_esdf, p_tsdf, p_sem = pinned(len(blocks) * nv * 8), pinned(len(blocks) * nv * 12), pinned(len(blocks) * nv * 92)

    def timed(call):
        g.synchronize()
        t0 = time.perf_counter()
        chk(call())
        return time.perf_counter() - t0

    t = dict(update=[], download=[], layers=[])
    for r in range(a.warmup + a.reps):
        got = {}
        for what in (("esdf", "layers") if r % 2 == 0 else ("layers", "esdf")):
            if what == "esdf":
                got["update"] = timed(lambda: L.ks_esdf_update(g._h, C.byref(ec), C.byref(st)))
                got["download"] = timed(lambda: L.ks_esdf_download_blocks(g._h, blocks.ctypes.data, len(blocks), p_esdf))
            else:
                got["layers"] = timed(lambda: L.ks_download_blocks(g._h, blocks.ctypes.data, len(blocks), p_tsdf, p_sem))
        if r >= a.warmup:
            for k, v in got.items():
                t[k].append(v)
    stats = {k: ([int(v) for v in getattr(st, k)] if k == "box_voxels" else int(getattr(st, k))) for k, _ in B.KsEsdfStats._fields_}
    # (5): the store is current after the loop above; every repetition integrates the next frame of the ring
    more = bench.make_frames(bench.WORKLOADS["C2"], range(a.frames, a.frames + a.warmup + a.reps))
    rs = B.KsEsdfRefreshStats()
    t5 = dict(refresh=[], update=[])
    shares, rooms, stale = [], [], []
    for r, f in enumerate(more):
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        got = dict(refresh=timed(lambda: L.ks_esdf_refresh(g._h, 0, C.byref(rs))))
        got["update"] = timed(lambda: L.ks_esdf_update(g._h, C.byref(ec), C.byref(st)))
        assert all(getattr(rs, k) == getattr(st, k) for k in ("voxels_observed", "voxels_fixed", "voxels_clamped")), "refresh and update disagree"
        if r >= a.warmup:
            for k, v in got.items():
                t5[k].append(v)
            shares.append(rs.tiles_recomputed / max(rs.tiles_total, 1))
            stale.append(rs.tiles_stale / max(rs.tiles_total, 1))
            rooms.append(int(rs.workspace_bytes))
    v = {"refresh_ms": med(t5["refresh"]), "update_ms": med(t5["update"]),
         "refresh_over_update": round(statistics.median(t5["refresh"]) / statistics.median(t5["update"]), 4),
         "tiles_stale_over_total": round(statistics.median(stale), 4), "tiles_recomputed_over_total": round(statistics.median(shares), 4),
         "workspace_bytes": int(statistics.median(rooms)), "update_workspace_bytes": int(st.workspace_bytes), "tiles_total": int(rs.tiles_total),
         "note": "one more ring frame integrated before every refresh; the update after it recomputes the same map from scratch"}
    ii = med([u + d for u, d in zip(t["update"], t["download"])])
    out = {
        "workload": "C2", "frames_integrated": a.frames, "reps": a.reps, "warmup": a.warmup,
        "max_distance_m": a.max_distance, "min_distance_m": a.min_distance,
        "map": {"tiles": tiles, "blocks": int(len(blocks)), "voxels_per_side": g.vps, "box_voxels": stats["box_voxels"],
                "workspace_bytes": stats["workspace_bytes"], "esdf_bytes": int(len(blocks)) * nv * 8, "layer_bytes": int(len(blocks)) * nv * 104},
        "stats": stats,
        "i_esdf_update_ms": med(t["update"]), "esdf_download_ms": med(t["download"]), "ii_update_plus_download_ms": ii,
        "iii_ks_download_blocks_ms": med(t["layers"]), "ii_below_iii": ii < med(t["layers"]),
        "v_refresh_after_one_frame": v,
        "note": "wall-clock around synchronous calls, candidates alternating in one process; (iii) is existing code, unchanged by the ESDF",
    }
    for p in (p_esdf, p_tsdf, p_sem):
        L.ks_host_free(p)
    g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
