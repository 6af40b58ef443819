#!/usr/bin/env python3
"""Rates of path shortening (ks_path_shorten) beside what a caller could do before it existed.  On the map the headline of bench.py
builds (the C2 ring: the map of tools/nav_rate.py) after one ks_esdf_update with the default configuration, radius 0.3 m, one goal at
the last camera position and the 10^4 starts of tools/nav_rate.py put through ks_nav_paths_device (max_waypoints 1024), in ONE
process, the candidates alternating, the median of --reps repetitions after warm-up:
  (1) ks_path_shorten_device at lookahead 64 and at lookahead 1024: events on ks_stream(ctx) around the enqueue (stats = NULL: no
      host wait inside the call)
  (2) ks_path_shorten, the host entry, end to end (wall clock: the rows in, the kernel, the rows out), lookahead 64
  (3) the yardstick: THE SAME GREEDY RULE DRIVEN FROM THE HOST with one ks_esdf_sweep_device call per greedy round over all live paths
      (torch builds the 64 candidate segments of every live path on the device and picks from the statuses; wall clock, lookahead 64).
      It must give the same waypoints, and the tool asserts that it does.  It is not the same work in two respects: it sweeps 64
      segments per live path in every round, the lanes a clipped chunk leaves out as NaN segments that end INVALID at once, and it
      makes no length and no min_clearance.
The paths that come back UNVERIFIED are looked at once: every adjacent segment of each is swept on its own (ks_esdf_sweep), and the
statuses of those that are not FREE, their positions in the path and their smallest clearances are recorded.
Waypoints in and out, sweeps, samples and the share of unverified segments are recorded with the times.  Nothing is gated on these
numbers.  Writes profiles/path_shorten_rate.json (or --out)."""
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


def host_driven(g, torch, stream, d_wp, d_nw, mw, radius, lookahead):
    """The contract's greedy rule with one ks_esdf_sweep_device call per round: (waypoints_out, n_out, rounds)."""
    n = d_nw.shape[0]
    with torch.cuda.stream(stream):
        m = d_nw.to(torch.int64)
        ok = (m >= 1) & (m <= mw) & torch.isfinite(torch.where((torch.arange(mw, device="cuda")[None, :] < m[:, None])[:, :, None], d_wp, 0.0)).all(dim=2).all(dim=1)
        out = torch.full_like(d_wp, -7.0)
        out[ok, 0] = d_wp[ok, 0]
        k = ok.to(torch.int64)
        a = torch.zeros(n, dtype=torch.int64, device="cuda")
        live = ok & (a < m - 1)
        top = torch.minimum(a + lookahead, m - 1)
        lanes = torch.arange(64, device="cuda")[None, :]
        rounds = 0
        while True:
            at = torch.nonzero(live)[:, 0]
            if at.numel() == 0:
                break
            rounds += 1
            j = top[at][:, None] - lanes
            has = j >= (a[at] + 1)[:, None]
            seg = torch.cat([d_wp[at, a[at]][:, None, :].expand(-1, 64, -1), d_wp[at[:, None], j.clamp(min=0)]], dim=2)
            seg = torch.where(has[:, :, None], seg, float("nan")).contiguous()
            status = torch.empty((at.numel(), 64), dtype=torch.uint8, device="cuda")
            g.esdf_sweep_device(seg.data_ptr(), at.numel() * 64, d_status=status.data_ptr(), stats=False, radius_m=radius)
            free = (status == 0) & has
            found = free.any(dim=1)
            last = (top[at] - a[at]) <= 64
            take = found | last
            j_star = torch.where(found, top[at] - free.to(torch.int64).argmax(dim=1), a[at] + 1)
            sel = at[take]
            out[sel, k[sel]] = d_wp[sel, j_star[take]]
            k[sel] += 1
            a[sel] = j_star[take]
            top[sel] = torch.minimum(a[sel] + lookahead, m[sel] - 1)
            live[sel] = a[sel] < m[sel] - 1
            top[at[~take]] -= 64
        stream.synchronize()
    return out, k, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40, help="frames of the C2 ring integrated before anything is measured")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--starts", type=int, default=10 ** 4)
    ap.add_argument("--max-waypoints", type=int, default=1024)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_shorten_rate.json"))
    a = ap.parse_args()
    import torch
    wl = bench.WORKLOADS["C2"]
    g = B.HipIntegrator(B.default_config(max_tiles=1 << 13, max_points=wl["w"] * wl["h"], pipeline_frames=0, **bench.integ_cfg(wl)))
    last = None
    for f in bench.make_frames(wl, range(a.frames)):
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        last = f
    g.synchronize()
    g.esdf_update()
    idx = g.block_indices()
    vs, vps = float(g.cfg.voxel_size), g.vps
    goal = np.asarray(last.T_G_C[4:7], np.float32).reshape(1, 3)
    g.nav_update(goal, radius_m=a.radius)
    blocks = g.nav_blocks(idx)
    rng = np.random.default_rng(1)                                               # the starts of tools/nav_rate.py
    free = np.argwhere(blocks != B.KS_NAV_BLOCKED)
    pick = free[rng.choice(len(free), a.starts, replace=len(free) < a.starts)]
    local = np.stack([pick[:, 1] % vps, (pick[:, 1] // vps) % vps, pick[:, 1] // (vps * vps)], axis=1)
    starts = ((idx[pick[:, 0]].astype(np.int64) * vps + local + 0.5) * vs).astype(np.float32)
    n, mw = a.starts, a.max_waypoints

    d_starts = torch.from_numpy(starts).to("cuda")
    d_wp = torch.full((n, mw, 3), -7.0, dtype=torch.float32, device="cuda")
    d_nw = torch.zeros((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    path_stats = g.nav_paths_device(d_starts.data_ptr(), n, mw, d_n_waypoints=d_nw.data_ptr(), d_waypoints=d_wp.data_ptr())
    wp, nw = d_wp.cpu().numpy(), d_nw.cpu().numpy().view(np.uint32)
    d_out = dict(status=torch.empty((n,), dtype=torch.uint8, device="cuda"), n_waypoints=torch.empty((n,), dtype=torch.int32, device="cuda"),
                 waypoints=torch.full((n, mw, 3), -7.0, dtype=torch.float32, device="cuda"), length=torch.empty((n,), dtype=torch.float32, device="cuda"),
                 min_clearance=torch.empty((n,), dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(g.stream)
    outs = [d_out[k].data_ptr() for k in ("status", "n_waypoints", "waypoints", "length", "min_clearance")]

    def device(lookahead, stats=False):
        return g.shorten_paths_device(d_wp.data_ptr(), d_nw.data_ptr(), n, mw, *outs, stats=stats, radius_m=a.radius, lookahead=lookahead)

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

    # what the calls compute, and that the host-driven rule gives the same waypoints
    stats = {look: device(look, stats=True) for look in (64, 1024)}
    device(64)
    g.synchronize()
    want_wp, want_k = d_out["waypoints"].cpu().numpy(), d_out["n_waypoints"].cpu().numpy()
    y_wp, y_k, y_rounds = host_driven(g, torch, stream, d_wp, d_nw, mw, a.radius, 64)
    assert (y_k.cpu().numpy() == want_k).all() and y_wp.cpu().numpy().tobytes() == want_wp.tobytes(), "the host-driven rule gives other waypoints"

    # the UNVERIFIED paths: which of their own segments no sweep verifies, and how that sweep ends
    bad = np.nonzero(d_out["status"].cpu().numpy() == B.KS_SHORTEN_UNVERIFIED)[0]
    segs, where = [], []
    for i in bad:
        m = int(nw[i])
        segs.append(np.concatenate([wp[i, :m - 1], wp[i, 1:m]], axis=1))
        where += [(int(i), k, m) for k in range(m - 1)]
    unverified = {"paths": int(len(bad))}
    if segs:
        sw = g.esdf_sweep(np.concatenate(segs), radius_m=a.radius)
        names = {B.KS_SWEEP_COLLISION: "collision", B.KS_SWEEP_UNKNOWN: "unknown", B.KS_SWEEP_INVALID: "invalid"}
        blocked = np.nonzero(sw["status"] != B.KS_SWEEP_FREE)[0]
        unverified.update(
            adjacent_segments=len(where), adjacent_segments_not_free=int(len(blocked)),
            not_free_by_status={v: int((sw["status"][blocked] == k).sum()) for k, v in names.items()},
            not_free_at_the_first_segment=int(sum(1 for j in blocked if where[j][1] == 0)),
            not_free_at_the_last_segment=int(sum(1 for j in blocked if where[j][1] == where[j][2] - 2)),
            t_stop_of_the_not_free_m=[round(float(v), 4) for v in sw["t_stop"][blocked]][:40],
            min_clearance_of_the_not_free_m=[round(float(v), 4) for v in sw["min_clearance"][blocked]][:40])

    candidates = {
        "shorten_device_lookahead_64": lambda: timed_device(lambda: device(64)),
        "shorten_device_lookahead_1024": lambda: timed_device(lambda: device(1024)),
        "shorten_host_lookahead_64": lambda: timed_host(lambda: g.shorten_paths(wp, nw, stats=False, radius_m=a.radius, lookahead=64)),
        "host_driven_sweeps_lookahead_64": lambda: timed_host(lambda: host_driven(g, torch, stream, d_wp, d_nw, mw, a.radius, 64)),
    }
    names = list(candidates)
    got = {k: [] for k in names}
    for r in range(a.warmup + a.reps):
        for k in (names if r % 2 == 0 else names[::-1]):
            ms = candidates[k]()
            if r >= a.warmup:
                got[k].append(ms)
    ms = {k: med(v) for k, v in got.items()}
    segments = {look: s["waypoints_out"] - s["paths_ok"] - s["paths_unverified"] for look, s in stats.items()}
    out = {
        "workload": "C2", "frames_integrated": a.frames, "reps": a.reps, "warmup": a.warmup,
        "map": {"tiles": len(g.tile_keys()), "blocks": int(len(idx))},
        "inputs": {"radius_m": a.radius, "starts": n, "max_waypoints": mw, "paths": path_stats},
        "shorten": {"lookahead_%d" % look: dict(s, segments_out=segments[look],
                                                 unverified_share=round(s["segments_unverified"] / max(1, segments[look]), 6)) for look, s in stats.items()},
        "unverified_paths_lookahead_64": unverified,
        "host_driven": {"rounds": y_rounds, "sweep_calls": y_rounds, "same_waypoints": True, "segments_swept_per_live_path_and_round": 64,
                        "makes_length_and_min_clearance": False},
        "ms": ms,
        "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in got.items()},
        "rates": {"device_lookahead_64_Msweeps_per_s": round(stats[64]["sweeps"] / ms["shorten_device_lookahead_64"] * 1e-3, 2),
                  "device_lookahead_64_Msamples_per_s": round(stats[64]["samples"] / ms["shorten_device_lookahead_64"] * 1e-3, 2),
                  "device_lookahead_1024_Msamples_per_s": round(stats[1024]["samples"] / ms["shorten_device_lookahead_1024"] * 1e-3, 2)},
        "note": "shorten_device: events on ks_stream around the enqueue (counter memset + kernel); shorten_host: wall clock around the synchronous call "
                "(pageable NumPy arrays, all max_waypoints rows of every path staged in and out); host_driven_sweeps: wall clock, torch on ks_stream builds "
                "the candidates and reads the statuses, one ks_esdf_sweep_device call per greedy round; candidates alternating in one process.  Not "
                "measured: other maps, C4, long known-free corridors, more than one GPU",
    }
    g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
