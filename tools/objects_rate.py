#!/usr/bin/env python3
"""Rate of the on-device object instances (ks_objects_update) against what a host connected-components pass needs before it can
start, the layer download.  On the map the headline of bench.py builds (the C2 ring), in ONE process, candidates alternating,
the median of --reps repetitions after warm-up, the context synchronised before every timed call (every timed call ends with a
stream synchronisation of its own):
  (1) ks_objects_update alone
  (2) ... + ks_objects_download of the records
  (3) ... + ks_objects_download_blocks of every block's ids into page-locked memory (a consumer that wants the ids as well)
  (4) ks_download_blocks of every block (TSDF + semantic layer) into page-locked memory: what the host pass needs first
Nothing is gated on these numbers.  Writes profiles/objects_rate.json (or --out)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40, help="frames of the C2 ring integrated before anything is measured")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-voxels", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_rate.json"))
    a = ap.parse_args()
    L = B.lib()
    g = build_map(a.frames)
    chk = g._chk
    oc, st = g.objects_config(min_voxels=a.min_voxels), B.KsObjectsStats()
    blocks = g.block_indices()
    tiles = len(g.tile_keys())
    nv = g.vps ** 3

    def pinned(n):
        p = L.ks_host_alloc(max(int(n), 1))
        assert p, "ks_host_alloc failed"
        return p

    p_ids, p_tsdf, p_sem = pinned(len(blocks) * nv * 4), pinned(len(blocks) * nv * 12), pinned(len(blocks) * nv * 92)
    chk(L.ks_objects_update(g._h, C.byref(oc), C.byref(st)))
    rec = np.zeros(max(int(st.components), 1), B.OBJECT_DTYPE)   # (room for any later count)
    n = C.c_size_t()

    def timed(call):
        g.synchronize()
        t0 = time.perf_counter()
        chk(call())
        return time.perf_counter() - t0

    t = dict(update=[], records=[], ids=[], layers=[])
    for r in range(a.warmup + a.reps):
        got = {}
        for what in (("objects", "layers") if r % 2 == 0 else ("layers", "objects")):
            if what == "objects":
                got["update"] = timed(lambda: L.ks_objects_update(g._h, C.byref(oc), C.byref(st)))
                got["records"] = timed(lambda: L.ks_objects_download(g._h, rec.ctypes.data, len(rec), C.byref(n)))
                got["ids"] = timed(lambda: L.ks_objects_download_blocks(g._h, blocks.ctypes.data, len(blocks), p_ids))
            else:
                got["layers"] = timed(lambda: L.ks_download_blocks(g._h, blocks.ctypes.data, len(blocks), p_tsdf, p_sem))
        if r >= a.warmup:
            for k, v in got.items():
                t[k].append(v)
    stats = {k: int(getattr(st, k)) for k, _ in B.KsObjectsStats._fields_}
    ii = med([u + d for u, d in zip(t["update"], t["records"])])
    iii = med([u + d + i for u, d, i in zip(t["update"], t["records"], t["ids"])])
    out = {
        "workload": "C2", "frames_integrated": a.frames, "reps": a.reps, "warmup": a.warmup, "min_voxels": a.min_voxels,
        "map": {"tiles": tiles, "blocks": int(len(blocks)), "voxels_per_side": g.vps, "record_bytes": int(n.value) * 72,
                "id_bytes": int(len(blocks)) * nv * 4, "layer_bytes": int(len(blocks)) * nv * 104},
        "stats": stats,
        "i_objects_update_ms": med(t["update"]), "records_download_ms": med(t["records"]), "ii_update_plus_records_ms": ii,
        "ids_download_ms": med(t["ids"]), "iii_update_plus_records_plus_ids_ms": iii,
        "iv_ks_download_blocks_ms": med(t["layers"]), "ii_below_iv": ii < med(t["layers"]),
        "note": "wall-clock around synchronous calls, candidates alternating in one process; (iv) is existing code, unchanged by the objects",
    }
    for p in (p_ids, p_tsdf, p_sem):
        L.ks_host_free(p)
    g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
