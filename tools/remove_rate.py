#!/usr/bin/env python3
"""Cost of pruning the resident map (ks_remove_distant_blocks) against what a caller had to do for the same result before the
call existed: download every block, ks_clear_voxels, upload the kept ones.  On the map the headline of bench.py builds (the C2
ring), in ONE process; every repetition starts from the same map (emptied and uploaded again from page-locked copies of all its
blocks: every block then holds all of its tiles), the candidates alternate, the context is synchronised before every timed call:
  (a) the call when it removes the farthest ~10 % of the blocks (a radius between two neighbouring block-origin distances from
      the centre of the ring, next to their 90th percentile), with tiles_moved
  (b) the call when it removes half of them (next to the median distance)
  (c), (d) for the same two sets: ks_download_blocks of every block into page-locked memory + ks_clear_voxels + a host gather of
      the kept blocks + ks_upload_blocks of them
Nothing is gated on these numbers.  Writes profiles/remove_rate.json (or --out)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40, help="frames of the C2 ring integrated before anything is measured")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remove_rate.json"))
    a = ap.parse_args()
    L = B.lib()
    wl = bench.WORKLOADS["C2"]
    ring = bench.make_frames(wl, range(a.frames))
    g = B.HipIntegrator(B.default_config(max_tiles=1 << 13, max_points=wl["w"] * wl["h"], pipeline_frames=0, **bench.integ_cfg(wl)))
    for f in ring:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.synchronize()
    chk = g._chk
    blocks = g.block_indices()
    nb, nv, tiles = len(blocks), g.vps ** 3, len(g.tile_keys())
    centre = np.mean([f.T_G_C[4:7] for f in ring], axis=0).astype(np.float32)
    dist = np.linalg.norm(blocks.astype(np.float64) * (float(g.cfg.voxel_size) * g.vps) - centre.astype(np.float64), axis=1)
    order = np.sort(dist)

    def radius_at(fraction):   # between two neighbouring distances (the widest gap within five ranks): no block sits on the threshold
        k0 = int(round(fraction * nb))
        k = max(range(max(k0 - 5, 1), min(k0 + 6, nb)), key=lambda i: order[i] - order[i - 1])
        return float(0.5 * (order[k - 1] + order[k]))

    radii = {"tenth": radius_at(0.9), "half": radius_at(0.5)}

    def pinned(n):
        p = L.ks_host_alloc(max(int(n), 1))
        assert p, "ks_host_alloc failed"
        return p

    p_tsdf, p_sem, q_tsdf, q_sem = pinned(nb * nv * 12), pinned(nb * nv * 92), pinned(nb * nv * 12), pinned(nb * nv * 92)
    chk(L.ks_download_blocks(g._h, blocks.ctypes.data, nb, p_tsdf, p_sem))   # the map every repetition starts from
    st = B.KsRemoveStats()

    def restore():
        chk(L.ks_clear_voxels(g._h))
        chk(L.ks_upload_blocks(g._h, blocks.ctypes.data, nb, p_tsdf, p_sem))
        g.synchronize()

    def timed(call):
        g.synchronize()
        t0 = time.perf_counter()
        call()
        return time.perf_counter() - t0

    def by_call(radius):
        chk(L.ks_remove_distant_blocks(g._h, centre.ctypes.data, radius, C.byref(st)))

    def by_hand(radius):
        # what a caller does today: everything comes down, the map is emptied, the kept blocks go back up
        chk(L.ks_download_blocks(g._h, blocks.ctypes.data, nb, q_tsdf, q_sem))
        keep = np.flatnonzero(dist <= radius)
        kept = np.ascontiguousarray(blocks[keep])
        t = np.frombuffer((C.c_uint8 * (nb * nv * 12)).from_address(q_tsdf), np.uint8).reshape(nb, nv * 12)
        s = np.frombuffer((C.c_uint8 * (nb * nv * 92)).from_address(q_sem), np.uint8).reshape(nb, nv * 92)
        kt, ks = np.ascontiguousarray(t[keep]), np.ascontiguousarray(s[keep])
        chk(L.ks_clear_voxels(g._h))
        if len(kept):
            chk(L.ks_upload_blocks(g._h, kept.ctypes.data, len(kept), kt.ctypes.data, ks.ctypes.data))

    t = {k: dict(call=[], hand=[]) for k in radii}
    stats, left = {}, {}
    restore()
    tiles_restored = len(g.tile_keys())
    for r in range(a.warmup + a.reps):
        for name, radius in radii.items():
            for what in (("call", "hand") if r % 2 == 0 else ("hand", "call")):
                restore()
                dt = timed((lambda: by_call(radius)) if what == "call" else (lambda: by_hand(radius)))
                if what == "call":
                    stats[name] = {k: int(getattr(st, k)) for k, _ in B.KsRemoveStats._fields_}
                left.setdefault(name, {})[what] = len(g.block_indices())
                if r >= a.warmup:
                    t[name][what].append(dt)
    for name in radii:
        assert left[name]["call"] == left[name]["hand"], left   # both leave the same blocks
    out = {
        "workload": "C2", "frames_integrated": a.frames, "reps": a.reps, "warmup": a.warmup,
        "map": {"tiles_integrated": tiles, "tiles": tiles_restored, "blocks": int(nb), "voxels_per_side": g.vps, "layer_bytes": int(nb) * nv * 104},
        "centre": [float(v) for v in centre], "radius_m": radii,
        "a_remove_tenth_ms": med(t["tenth"]["call"]), "a_stats": stats["tenth"],
        "b_remove_half_ms": med(t["half"]["call"]), "b_stats": stats["half"],
        "c_download_clear_upload_tenth_ms": med(t["tenth"]["hand"]), "d_download_clear_upload_half_ms": med(t["half"]["hand"]),
        "blocks_left": left,
        "note": "wall-clock around synchronous calls, candidates alternating in one process, every repetition from the same restored map; "
                "(c) and (d) are existing code with page-locked staging for the download, unchanged by the removal",
    }
    for p in (p_tsdf, p_sem, q_tsdf, q_sem):
        L.ks_host_free(p)
    g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
