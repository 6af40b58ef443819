#!/usr/bin/env python3
"""Rate of the on-device mesher (ks_mesh_update) against what it replaces, the layer download a host mesher needs first.
On the map the headline of bench.py builds (the C2 ring; --workload C4-merged for the other), in ONE process, candidates
alternating, the median of --reps repetitions after warm-up, the context synchronised before every timed call (every timed
call ends with a stream synchronisation of its own):
  full         (i)   ks_mesh_update, only_stale = 0
               (iii) ... + ks_mesh_download into page-locked memory
               (iv)  ks_download_blocks of every block (TSDF + semantic layer) into page-locked memory
  incremental  one more frame of the ring integrated before every repetition, then — on the same frame, the flags of the two
               consumers are independent —
               (ii)  ks_mesh_update, only_stale = 1
               (iii) ... + ks_mesh_download (the whole mesh: the ABI has no partial download) into page-locked memory
               (iv)  ks_download_updated_voxels into page-locked memory (buffer sized beforehand, not timed)
Acceptance: (iii) <= (iv) in both cases.  Writes profiles/mesh_rate.json (or --out)."""
import argparse
import ctypes as C
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

HBM_PEAK = 8e12


def med(xs):
    return round(statistics.median(xs) * 1e3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--frames", type=int, default=40, help="frames of the ring integrated before anything is measured")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_rate.json"))
    a = ap.parse_args()
    wl = bench.WORKLOADS[a.workload]
    n_ring = a.frames if a.workload == "C2" else min(a.frames, bench.C4_STEPS)
    ring = bench.make_frames(wl, range(n_ring))
    L = B.lib()
    g = B.HipIntegrator(B.default_config(max_tiles=(1 << 13) if a.workload.startswith("C2") or a.workload == "C3" else (1 << 18),
                                         max_points=wl["w"] * wl["h"], pipeline_frames=0, **bench.integ_cfg(wl)))
    for f in ring:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.synchronize()
    blocks = g.block_indices()
    tiles = len(g.tile_keys())
    nv = g.vps ** 3
    chk = g._chk

    def pinned(n):
        p = L.ks_host_alloc(max(int(n), 1))
        assert p, "ks_host_alloc failed"
        return p

    mc, st = B.KsMeshConfig(1e-4, 0), B.KsMeshStats()
    chk(L.ks_mesh_update(g._h, C.byref(mc), C.byref(st)))
    cap_v = int(st.triangles_total) * 3 * 2 + 4096
    cap_b = len(blocks) * 2 + 64
    p_blocks, p_xyz, p_nrm, p_rgba, p_lab = pinned(cap_b * 20), pinned(cap_v * 12), pinned(cap_v * 12), pinned(cap_v * 4), pinned(cap_v)
    p_tsdf, p_sem = pinned(len(blocks) * nv * 12), pinned(len(blocks) * nv * 92)
    n_rec = C.c_size_t()
    chk(L.ks_count_updated_voxels(g._h, C.byref(n_rec), None))     # (every voxel written so far: the first download consumes them)
    cap_rec = n_rec.value + 4096
    p_rec, p_runs = pinned(cap_rec * 120), pinned(tiles * 20)

    def t_update(only_stale):
        mc.only_stale = only_stale
        g.synchronize()
        t0 = time.perf_counter()
        chk(L.ks_mesh_update(g._h, C.byref(mc), C.byref(st)))
        return time.perf_counter() - t0

    def t_mesh_download():
        g.synchronize()
        t0 = time.perf_counter()
        chk(L.ks_mesh_download(g._h, p_blocks, cap_b, p_xyz, p_nrm, p_rgba, p_lab, cap_v))
        return time.perf_counter() - t0

    def t_layer_download():
        g.synchronize()
        t0 = time.perf_counter()
        chk(L.ks_download_blocks(g._h, blocks.ctypes.data, len(blocks), p_tsdf, p_sem))
        return time.perf_counter() - t0

    def t_voxel_download():
        n, nr = C.c_size_t(), C.c_size_t()
        g.synchronize()
        t0 = time.perf_counter()
        chk(L.ks_download_updated_voxels(g._h, p_rec, cap_rec, C.byref(n), p_runs, tiles, C.byref(nr)))
        return time.perf_counter() - t0, n.value

    full = dict(update=[], download=[], layers=[])
    for r in range(a.warmup + a.reps):
        order = ("mesh", "layers") if r % 2 == 0 else ("layers", "mesh")
        got = {}
        for what in order:
            if what == "mesh":
                got["update"] = t_update(0)
                got["download"] = t_mesh_download()
            else:
                got["layers"] = t_layer_download()
        if r >= a.warmup:
            for k, v in got.items():
                full[k].append(v)
    full_stats = {k: int(getattr(st, k)) for k, _ in B.KsMeshStats._fields_}
    # incremental: consume both consumers' flags of the map so far, then one more frame per repetition
    t_update(1)
    t_voxel_download()
    inc = dict(update=[], download=[], voxels=[], meshed=[], records=[], triangles_changed=[])
    for r in range(a.warmup + a.reps):
        f = ring[r % len(ring)]
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        got = {}
        for what in (("mesh", "voxels") if r % 2 == 0 else ("voxels", "mesh")):
            if what == "mesh":
                got["update"] = t_update(1)
                got["download"] = t_mesh_download()
                got["meshed"] = int(st.blocks_meshed)
                got["triangles_changed"] = int(st.triangles_changed)
            else:
                got["voxels"], got["records"] = t_voxel_download()
        if r >= a.warmup:
            for k, v in got.items():
                inc[k].append(v)
    nb_v, nv_v = C.c_size_t(), C.c_size_t()
    chk(L.ks_mesh_size(g._h, C.byref(nb_v), C.byref(nv_v)))
    line_bytes_per_pass = tiles * 729 * 128          # every record is one 128-byte line; a pass fetches the tile and its halo
    i_ms = med(full["update"])
    iii_full = med([u + d for u, d in zip(full["update"], full["download"])])
    iii_inc = med([u + d for u, d in zip(inc["update"], inc["download"])])
    out = {
        "workload": a.workload, "frames_integrated": len(ring), "reps": a.reps, "warmup": a.warmup,
        "map": {"tiles": tiles, "blocks": int(len(blocks)), "voxels_per_side": g.vps, "triangles": full_stats["triangles_total"],
                "mesh_bytes": int(nv_v.value) * 29, "layer_bytes": int(len(blocks)) * nv * 104},
        "full": {"i_mesh_update_ms": i_ms, "mesh_download_ms": med(full["download"]), "iii_update_plus_download_ms": iii_full,
                 "iv_ks_download_blocks_ms": med(full["layers"]), "stats": full_stats,
                 "tiles_read": tiles, "bytes_read_per_pass_tiles_x_64KiB": tiles * 65536, "bytes_read_per_pass_with_halo": line_bytes_per_pass,
                 "passes": 2, "fraction_of_8TBs": round(2 * line_bytes_per_pass / (i_ms * 1e-3) / HBM_PEAK, 4),
                 "accepted": iii_full <= med(full["layers"])},
        "incremental": {"ii_mesh_update_only_stale_ms": med(inc["update"]), "mesh_download_whole_mesh_ms": med(inc["download"]),
                        "iii_update_plus_download_ms": iii_inc, "iv_ks_download_updated_voxels_ms": med(inc["voxels"]),
                        "blocks_meshed_median": int(statistics.median(inc["meshed"])), "triangles_changed_median": int(statistics.median(inc["triangles_changed"])),
                        "voxel_records_median": int(statistics.median(inc["records"])), "accepted": iii_inc <= med(inc["voxels"])},
        "note": "wall-clock around synchronous calls, candidates alternating in one process; (iv) is existing code, unchanged by the mesher",
    }
    for p in (p_blocks, p_xyz, p_nrm, p_rgba, p_lab, p_tsdf, p_sem, p_rec, p_runs):
        L.ks_host_free(p)
    g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
