#!/usr/bin/env python3
"""Evidence for the refactoring of the map's readers (block lists, ks_mesh_update, ks_esdf_update, ks_esdf_refresh, rendering): the
sequence of launches, copies, memsets, event operations and synchronisations of every stream, on the host functional model.

    python profiles/map_readers_refactor/record_trace.py <tree> <out.txt> [<directory for the traces>]

runs every entry of SPECS of tests/mesh_case.py, esdf_case.py, esdf_refresh_case.py and render_case.py of <tree> against
<tree>/tools/emu/_build/libks_hip_emu.so (built by <tree>/tools/emu/build_emu.sh) with EMU_TRACE=1, one child process per case,
and writes one line per (case, stream): the number of trace lines of that stream and the SHA-256 of their sequence (digest() of
profiles/frame_path_refactor/record_trace.py).  Blocking hipMemcpy / hipMemset calls are traced on the null stream with their
kind and byte count, so both trees are recorded with the same tools/emu/hip/hip_runtime.h.  Two trees enqueue the same work
when their files are equal:

    diff profiles/map_readers_refactor/parent.txt profiles/map_readers_refactor/change.txt
"""
import concurrent.futures
import importlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "frame_path_refactor"))
from record_trace import digest  # noqa: E402

MODULES = ("mesh_case", "esdf_case", "esdf_refresh_case", "render_case")


def main():
    tree, out = os.path.abspath(sys.argv[1]), sys.argv[2]
    sys.path.insert(0, tree)
    env = dict(os.environ, KS_HIP_LIB=os.path.join(tree, "tools", "emu", "_build", "libks_hip_emu.so"), EMU_TRACE="1", PYTHONPATH=tree)
    jobs = [(m, name, spec) for m in MODULES for name, spec in importlib.import_module("tests." + m).SPECS.items()]

    def run(job):
        m, name, spec = job
        p = subprocess.run([sys.executable, os.path.join(tree, "tests", m + ".py"), json.dumps(spec)], cwd=tree, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0 and "_CASE_OK" in p.stdout, (m, name, p.stdout[-1000:], p.stderr[-3000:])
        return p.stderr

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool, open(out, "w") as f:
        for (m, name, _), err in zip(jobs, pool.map(run, jobs)):
            if len(sys.argv) > 3:   # the traces themselves, for a look at a difference
                open(os.path.join(sys.argv[3], f"{m}.{name}.trace"), "w").write(err)
            for key, (n, h) in sorted(digest(err).items()):
                f.write(f"{m}.{name}  {key}  {n} lines  {h}\n")


if __name__ == "__main__":
    main()
