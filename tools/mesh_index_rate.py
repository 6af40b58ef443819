#!/usr/bin/env python3
"""Rate of the indexed view of the stored mesh (ks_mesh_index) beside the unshared mesh it is made from.
On the map the headline of bench.py builds (the C2 ring: the map of tools/mesh_rate.py), the mesh extracted once, then in ONE
process, candidates alternating, the median of --reps repetitions after warm-up, the context synchronised before every timed
call (every timed call ends with a stream synchronisation of its own):
  (1) ks_mesh_index alone
  (2) ... + ks_mesh_index_download of every array into page-locked memory
  (3) ks_mesh_download of the unshared mesh (directory and four arrays) into page-locked memory
  (4) the bytes of both forms, V / C, the most corners on one vertex, the work space
  (5) the kernels' times, from a kernel trace made in a run of its own:
        rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_index_rate.py --trace-child
        python tools/mesh_index_rate.py --merge-kernel-stats DIR/**/*kernel_stats.csv
Nothing is gated on these numbers.  Writes profiles/mesh_index_rate.json (or --out)."""
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

KERNELS = ("k_mi_keys_z", "k_mi_keys_xy", "k_mi_heads", "k_mi_scan_partial", "k_mi_scan_top", "k_mi_scan_apply", "k_mi_first", "k_mi_emit",
           "k_mi_finish", "k_rs_hist", "k_rs_pass", "k_obj_query")


def med(xs):
    return round(statistics.median(xs) * 1e3, 4)


def build_map(frames):
    wl = bench.WORKLOADS["C2"]
    ring = bench.make_frames(wl, range(frames))
    g = B.HipIntegrator(B.default_config(max_tiles=1 << 13, max_points=wl["w"] * wl["h"], pipeline_frames=0, **bench.integ_cfg(wl)))
    for f in ring:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.synchronize()
    mc, st = B.KsMeshConfig(1e-4, 0), B.KsMeshStats()
    g._chk(B.lib().ks_mesh_update(g._h, C.byref(mc), C.byref(st)))
    return g, int(st.triangles_total)


def merge_kernel_stats(a):
    out = json.load(open(a.out))
    rows = {}
    for path in a.merge_kernel_stats:
        for row in csv.DictReader(open(path)):
            name = row.get("Name") or row.get("KernelName") or ""
            for k in KERNELS:
                if k in name:
                    calls = int(row.get("Calls") or row.get("Count") or 0)
                    total = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0.0)
                    if calls:
                        r = rows.setdefault(k, {"calls": 0, "total_ms": 0.0})
                        r["calls"] += calls
                        r["total_ms"] = round(r["total_ms"] + total * 1e-6, 4)
    for r in rows.values():
        r["mean_ms"] = round(r["total_ms"] / r["calls"], 5)
    out["kernel_trace"] = dict(rows, source="rocprofv3 --kernel-trace --stats, a run of its own (--trace-child: the map, the mesh, five ks_mesh_index); "
                                            "k_rs_* also count the sorts of the frames that built the map")
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40, help="frames of the C2 ring integrated before anything is measured")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-child", action="store_true", help="build the map and the mesh and run ks_mesh_index five times (for a kernel trace)")
    ap.add_argument("--merge-kernel-stats", nargs="+", metavar="CSV", help="fold the kernels' times of a kernel trace into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_index_rate.json"))
    a = ap.parse_args()
    if a.merge_kernel_stats:
        return merge_kernel_stats(a)
    L = B.lib()
    g, triangles = build_map(a.frames)
    chk = g._chk
    st = B.KsMeshIndexStats()
    if a.trace_child:
        for _ in range(5):
            chk(L.ks_mesh_index(g._h, C.byref(st)))
        g.close()
        return
    chk(L.ks_mesh_index(g._h, C.byref(st)))
    n_c, n_v = int(st.corners), int(st.vertices)
    nb, nvv = C.c_size_t(), C.c_size_t()
    chk(L.ks_mesh_size(g._h, C.byref(nb), C.byref(nvv)))
    assert nvv.value == n_c == 3 * triangles

    def pinned(n):
        p = L.ks_host_alloc(max(int(n), 1))
        assert p, "ks_host_alloc failed"
        return p

    u_blocks, u_xyz, u_nrm, u_rgba, u_lab = pinned(nb.value * 20), pinned(n_c * 12), pinned(n_c * 12), pinned(n_c * 4), pinned(n_c)
    i_xyz, i_nrm, i_rgba, i_lab, i_obj, i_idx = pinned(n_v * 12), pinned(n_v * 12), pinned(n_v * 4), pinned(n_v), pinned(n_v * 4), pinned(n_c * 4)

    def t_index():
        g.synchronize()
        t0 = time.perf_counter()
        chk(L.ks_mesh_index(g._h, C.byref(st)))
        return time.perf_counter() - t0

    def t_index_download():
        g.synchronize()
        t0 = time.perf_counter()
        chk(L.ks_mesh_index_download(g._h, i_xyz, i_nrm, i_rgba, i_lab, i_obj, n_v, i_idx, n_c))
        return time.perf_counter() - t0

    def t_mesh_download():
        g.synchronize()
        t0 = time.perf_counter()
        chk(L.ks_mesh_download(g._h, u_blocks, nb.value, u_xyz, u_nrm, u_rgba, u_lab, n_c))
        return time.perf_counter() - t0

    got = dict(index=[], index_download=[], mesh_download=[])
    for r in range(a.warmup + a.reps):
        one = {}
        for what in (("indexed", "unshared") if r % 2 == 0 else ("unshared", "indexed")):
            if what == "indexed":
                one["index"] = t_index()
                one["index_download"] = t_index_download()
            else:
                one["mesh_download"] = t_mesh_download()
        if r >= a.warmup:
            for k, v in one.items():
                got[k].append(v)
    out = {
        "workload": "C2", "frames_integrated": a.frames, "reps": a.reps, "warmup": a.warmup,
        "map": {"tiles": len(g.tile_keys()), "blocks": int(len(g.block_indices())), "triangles": triangles},
        "index": {"corners": n_c, "vertices": n_v, "vertices_per_corner": round(n_v / max(n_c, 1), 4),
                  "max_corners_per_vertex": int(st.max_corners_per_vertex), "workspace_bytes": int(st.workspace_bytes)},
        "bytes": {"unshared_29_per_corner": n_c * 29, "indexed_33_per_vertex_plus_4_per_corner": n_v * 33 + n_c * 4},
        "ms": {"1_ks_mesh_index": med(got["index"]), "ks_mesh_index_download": med(got["index_download"]),
               "2_index_plus_download": med([x + y for x, y in zip(got["index"], got["index_download"])]),
               "3_ks_mesh_download_unshared": med(got["mesh_download"])},
        "note": "wall-clock around synchronous calls, candidates alternating in one process, downloads into page-locked memory",
    }
    for p in (u_blocks, u_xyz, u_nrm, u_rgba, u_lab, i_xyz, i_nrm, i_rgba, i_lab, i_obj, i_idx):
        L.ks_host_free(p)
    g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
