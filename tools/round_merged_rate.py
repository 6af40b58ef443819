#!/usr/bin/env python3
"""What the EXACT frame-sharded round of `merged` costs next to the plain one-GPU path (ks_integrate_round_exact with
method = 1, csrc/ks_k_shard_merged.h).

Eight 640x480 arc-pose frames (BASELINE configuration 5's shape), every repetition on an EMPTY map (ks_clear), after one
warm-up batch that sizes every buffer; a synchronised perf_counter around the whole batch; median and spread over --reps.
  round   ks_integrate_round_exact, world 1: march on one context, records, import, second sort, update on the other
  plain   ks_integrate_points with method = merged, pipeline_frames = 0, same frames, same empty-map start
  wire    bytes sent per update at world 2 (two processes on this GPU, the librccl test double; one round of two frames),
          from ks_round_stats — next to the 20 bytes of a `fast` record
One JSON record on stdout and in --out.  `--only round` runs the rounds alone (for a kernel trace of them)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kimera_semantics_amd import binding as B   # noqa: E402
from kimera_semantics_amd import synth           # noqa: E402

W, H, N_FRAMES = 640, 480, 8


def ctx():
    return B.HipIntegrator(B.default_config(method=1, max_tiles=1 << 15, max_points=W * H, pipeline_frames=0, voxels_per_side=8,
                                            semantic_measurement_probability=0.8, dynamic_labels=[20],
                                            label_rgba=synth.default_label_colors()))


def timed(reps, batch, reset):
    """ms per frame of `batch()` for each repetition; `reset()` empties the maps before each."""
    out = []
    for rep in range(reps + 1):   # repetition 0 is the warm-up: buffers grow to their steady size
        reset()
        t0 = time.perf_counter()
        updates = batch(rep)
        dt = time.perf_counter() - t0
        if rep:
            out.append(1e3 * dt / N_FRAMES)
    return out, updates


def summary(ms):
    return dict(median_ms_per_frame=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4), reps=len(ms))


def wire_bytes_per_update():
    mock = os.path.join(ROOT, "tests", "mock_rccl", "libmock_rccl.so")
    lib = C.CDLL(mock)

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_byte * 128)]
    uid = UniqueId()
    assert lib.ncclGetUniqueId(C.byref(uid)) == 0
    env = dict(os.environ, KS_RCCL_LIB=mock, KS_ROUND_WH=f"{W}x{H}")
    with tempfile.TemporaryDirectory() as tmp:
        procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "round_merged_worker.py"), str(r), "2", bytes(uid).hex(), tmp,
                                   "round:1"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
        for p in procs:
            try:
                out, _ = p.communicate(timeout=300)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
            if p.returncode:
                raise RuntimeError(out[-2000:])
        sent = marched = 0
        for r in range(2):
            with np.load(os.path.join(tmp, f"round_rank{r}.npz")) as z:
                sent += int(z["sent"].sum())
                marched += int(z["marched"].sum())
    # (about half of a rank's updates stay at home: per update SENT the figure is what the wire format costs)
    return dict(world=2, bytes_sent=sent, updates_marched=marched, bytes_per_update_marched=round(sent / marched, 3))


def main():
    global W, H
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["round", "plain"], default=None)
    ap.add_argument("--no-wire", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round_merged_rate.json"))
    ap.add_argument("--width", type=int, default=W)   # (smaller sizes: rehearsals only)
    ap.add_argument("--height", type=int, default=H)
    a = ap.parse_args()
    W, H = a.width, a.height
    sc = synth.make_scene("room")
    frames = [synth.render_frame(sc, synth.arc_pose(k, n=N_FRAMES), W, H, seed=100 + k) for k in range(N_FRAMES)]
    rec = dict(tool="tools/round_merged_rate.py", frames=N_FRAMES, width=W, height=H, method="merged", voxel_size=0.05)
    if a.only != "plain":
        marcher, owner = ctx(), ctx()

        def reset():
            marcher.clear()
            owner.clear()

        def batch(rep):
            n = 0
            for k, f in enumerate(frames):
                n += owner.integrate_round_exact(marcher, None, 0, 1, rep * N_FRAMES + k, f.T_G_C, f.xyz, f.rgba, f.labels)["updates_applied"]
            owner.synchronize()
            return n
        ms, updates = timed(a.reps, batch, reset)
        rec["round_world1"] = dict(summary(ms), updates_per_batch=updates)
        marcher.close()
        owner.close()
    if a.only != "round":
        h = ctx()

        def batch_plain(rep):
            n = 0
            for f in frames:
                n += h.integrate(f.T_G_C, f.xyz, f.rgba, f.labels).n_voxel_updates
            h.synchronize()
            return n
        ms, updates = timed(a.reps, batch_plain, h.clear)
        rec["plain_merged"] = dict(summary(ms), updates_per_batch=updates)
        h.close()
    if a.only is None and not a.no_wire:
        rec["wire"] = dict(wire_bytes_per_update(), fast_record_bytes=20)
    line = json.dumps(rec)
    print(line)
    if a.only is None:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
