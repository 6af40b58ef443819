#!/usr/bin/env python3
"""Cost of fusing a submap into the resident map at a rigid pose (ks_fuse_map) against what a caller pays today BEFORE a host-side
resampling can even start: ks_download_blocks of the source plus ks_upload_blocks of as many blocks into the destination.  On the
map the headline of bench.py builds (the C2 ring) as the source, in ONE process; the destination is emptied before every
repetition (ks_clear_voxels), the candidates alternate, both contexts are synchronised before every timed call:
  (a) the call at the identity pose into an empty destination
  (b) the call at a generic pose (33 degrees about (1, 2, 3), a translation of (0.31, -0.17, 0.23) m) into an empty destination
  (c) the same pose into a destination that already holds a copy of the source map (every touched tile exists: no allocation)
  (d) the lower bound of the host route: ks_download_blocks of every source block into page-locked memory + ks_upload_blocks of the
      same bytes into the empty destination — no resampling, no merge arithmetic (12 + 92 bytes per voxel twice over the link)
This script times calls; the resample and merge kernels' own times are read from a `rocprofv3 --kernel-trace --stats` run of it
(profiles/fuse_rate_kernel_stats.txt).  Nothing is gated on these numbers.  Writes profiles/fuse_rate.json (or --out)."""
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


def pose(axis, deg, t):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = np.deg2rad(deg) / 2
    return np.concatenate([[np.cos(h)], np.sin(h) * a, np.asarray(t, np.float64)]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40, help="frames of the C2 ring integrated before anything is measured")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_rate.json"))
    a = ap.parse_args()
    L = B.lib()
    wl = bench.WORKLOADS["C2"]
    ring = bench.make_frames(wl, range(a.frames))
    make = lambda: B.HipIntegrator(B.default_config(max_tiles=1 << 14, max_points=wl["w"] * wl["h"], pipeline_frames=0, **bench.integ_cfg(wl)))
    src, dst = make(), make()
    for f in ring:
        src.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    src.synchronize()
    blocks = src.block_indices()
    nb, nv, tiles = len(blocks), src.vps ** 3, len(src.tile_keys())
    poses = {"identity": pose((0, 0, 1), 0.0, (0, 0, 0)), "generic": pose((1, 2, 3), 33.0, (0.31, -0.17, 0.23))}

    def pinned(n):
        p = L.ks_host_alloc(max(int(n), 1))
        assert p, "ks_host_alloc failed"
        return p

    p_tsdf, p_sem = pinned(nb * nv * 12), pinned(nb * nv * 92)
    dst._chk(L.ks_download_blocks(src._h, blocks.ctypes.data, nb, p_tsdf, p_sem))   # (also: the copy of the source that (c) starts from)

    def empty():
        dst.clear_voxels()
        dst.synchronize()

    def copy_of_source():
        empty()
        dst._chk(L.ks_upload_blocks(dst._h, blocks.ctypes.data, nb, p_tsdf, p_sem))
        dst.synchronize()

    def timed(call):
        src.synchronize()
        dst.synchronize()
        t0 = time.perf_counter()
        out = call()
        return time.perf_counter() - t0, out

    def host_route():
        dst._chk(L.ks_download_blocks(src._h, blocks.ctypes.data, nb, p_tsdf, p_sem))
        dst._chk(L.ks_upload_blocks(dst._h, blocks.ctypes.data, nb, p_tsdf, p_sem))

    cands = {
        "a_fuse_identity_empty": (empty, lambda: dst.fuse(src, poses["identity"])),
        "b_fuse_generic_empty": (empty, lambda: dst.fuse(src, poses["generic"])),
        "c_fuse_generic_into_copy": (copy_of_source, lambda: dst.fuse(src, poses["generic"])),
        "d_download_plus_upload": (empty, host_route),
    }
    t = {k: [] for k in cands}
    stats = {}
    names = list(cands)
    for r in range(a.warmup + a.reps):
        for name in (names if r % 2 == 0 else names[::-1]):
            prepare, call = cands[name]
            prepare()
            dt, out = timed(call)
            if isinstance(out, dict):
                stats[name] = out
            if r >= a.warmup:
                t[name].append(dt)
    out = {
        "workload": "C2", "frames_integrated": a.frames, "reps": a.reps, "warmup": a.warmup,
        "source_map": {"tiles": tiles, "blocks": int(nb), "voxels_per_side": src.vps, "layer_bytes": int(nb) * nv * 104},
        "poses": {k: [float(v) for v in p] for k, p in poses.items()},
    }
    for name in names:
        out[name + "_ms"] = med(t[name])
        out[name + "_min_max_ms"] = [round(min(t[name]) * 1e3, 4), round(max(t[name]) * 1e3, 4)]
        if name in stats:
            out[name + "_stats"] = stats[name]
    out["note"] = ("wall-clock around synchronous calls, candidates alternating in one process, the destination prepared before every repetition; "
                   "(d) is existing code with page-locked staging and is only the transfer a host-side resampling starts from — the resampling of "
                   "12 + 92 bytes per voxel on the host and the merge are not in it; the kernels' own times: profiles/fuse_rate_kernel_stats.txt")
    L.ks_host_free(p_tsdf)
    L.ks_host_free(p_sem)
    src.close()
    dst.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
