#!/usr/bin/env python3
"""Evidence for the refactoring of the per-frame host path (frame_front, launch_batch, frame_tail): the sequence of launches,
copies, memsets, event records, waits and host synchronisations of every stream, on the host functional model.

    python profiles/frame_path_refactor/record_trace.py <tree> <out.txt>

runs the cases below against <tree>/tools/emu/_build/libks_hip_emu.so (built by <tree>/tools/emu/build_emu.sh) with EMU_TRACE=1,
one child process per case, and writes one line per (case, stream): the number of trace lines of that stream and the SHA-256 of
their sequence.  The caller and the tail's helper thread enqueue side by side, so only the order within a stream is defined:
lines are grouped by stream ordinal (host waits for an event, which have no stream, by event ordinal) and keep their order.
Template arguments are dropped from the kernels' names: a launch inside a function template names its kernel by the template's
parameters, not by their values.  Two trees enqueue the same work when their files are equal:

    diff profiles/frame_path_refactor/parent.txt profiles/frame_path_refactor/change.txt
"""
import hashlib
import json
import os
import re
import subprocess
import sys

SMALL = dict(max_tiles=4096, max_points=1024)
CASES = {
    "fast_unpipelined": dict(cfg=dict(method=0, pipeline_frames=0), budget=8),
    "fast_p12_budget4": dict(cfg=dict(method=0, pipeline_frames=12), budget=4),
    "fast_p12_budget8": dict(cfg=dict(method=0, pipeline_frames=12), budget=8),
    "phased_p4": dict(cfg=dict(method=0, pipeline_frames=4, early_out_phase_growth=32), budget=4),
    "merged_p8_budget3": dict(cfg=dict(method=1, pipeline_frames=8), budget=3),
    "merged_p8_budget8": dict(cfg=dict(method=1, pipeline_frames=8), budget=8),
    "fast_p4_profile1": dict(cfg=dict(method=0, pipeline_frames=4), budget=8, profile=1),
    "merged_p8_profile2": dict(cfg=dict(method=1, pipeline_frames=8), budget=4, profile=2),
    # tests/stream_plan_case.py: a fallback, the growth of the mark buffers and a cloud that outgrows max_points
    "stream_p12_budget4": dict(stream=dict(pipeline=12, budget=4, streams=4)),
}


def child(spec):
    from tests import stream_plan_case as SP
    if "stream" in spec:
        SP.run_stream(spec["stream"])
        return
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    SP.set_budget(spec["budget"])
    g = B.HipIntegrator(SP.config(**dict(SMALL, **spec["cfg"])))
    if spec.get("profile"):
        g.profile_enable(spec["profile"])
    sc = synth.make_scene("room")
    for i in range(10):
        w, h = (32, 24) if i % 3 == 2 else (16, 12)
        f = synth.render_frame(sc, synth.trajectory_pose(3 * i), w, h, seed=700 + i)
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        if i == 6:
            g.flush()   # (a batch that goes out before it is full)
    g.flush()
    g.close()


def digest(trace):
    per = {}
    for line in trace.splitlines():
        if not line.startswith("emu: "):
            continue
        m = re.match(r"emu: launch (.*) (grid .*)$", line)
        if m:
            line = "launch " + re.sub(r"<.*>", "", m.group(1)).strip("()") + " " + m.group(2)
        m = re.search(r" stream (\d+)$", line)
        key = "stream %02d" % int(m.group(1)) if m else "host, " + re.search(r"event \d+", line).group(0)
        per.setdefault(key, []).append(line)
    return {k: (len(v), hashlib.sha256("\n".join(v).encode()).hexdigest()) for k, v in per.items()}


def main():
    if sys.argv[1] == "--child":
        child(json.loads(sys.argv[2]))
        return
    tree, out = os.path.abspath(sys.argv[1]), sys.argv[2]
    env = dict(os.environ, KS_HIP_LIB=os.path.join(tree, "tools", "emu", "_build", "libks_hip_emu.so"), EMU_TRACE="1", PYTHONPATH=tree)
    procs = {name: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", json.dumps(spec)], cwd=tree, env=env,
                                    stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True) for name, spec in CASES.items()}
    with open(out, "w") as f:
        for name, p in procs.items():
            err = p.communicate()[1]
            assert p.returncode == 0, (name, err[-3000:])
            if len(sys.argv) > 3:   # the traces themselves, for a look at a difference
                open(os.path.join(sys.argv[3], name + ".trace"), "w").write(err)
            for key, (n, h) in sorted(digest(err).items()):
                f.write(f"{name}  {key}  {n} lines  {h}\n")


if __name__ == "__main__":
    main()
