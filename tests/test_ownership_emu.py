"""CPU tier: every device buffer, pinned buffer, event and stream of a context has one owner (csrc/ks_owned.h) — checked on the host
functional model of the library (tools/emu), whose runtime stand-in keeps a ledger of what is live and can make the k-th
allocation fail (tools/emu/README.md).  The cases are in tests/ownership_case.py; every case is one child process, they run
side by side.

Balance: a context is used and destroyed, and the ledger is what it was before ks_create — `fast` in its default mode
unpipelined and with pipeline_frames = 8, `fast` with ordered phases, `merged` in the reference's bundle order and with
anti-grazing, a cloud that outgrows max_points, a map that outgrows max_tiles (grow_pool between frames and inside an upload), the
mesh (full, then only_stale), block upload / download / updated voxels, ks_clear and ks_clear_voxels in mid-stream,
ks_debug_radix_sort, and one ks_integrate_round_exact round at world 1 for both methods (that entry point runs on the functional
model as it is; with world > 1 it needs the communicator double of tests/test_round_exact_merged_cpu.py, which owns nothing here).

Failure paths, every index, no sampling: each allocation of ks_create fails once (`fast` and `merged`, max_tiles 64, max_points
1024, unpipelined: 121 and 91 allocations — and the pipelined `fast` context too, pipeline_frames = 8: its sweep of 502 allocations
takes 56 s alone on 8 cores, so it stays in); each allocation of one ks_upload_blocks, one ks_mesh_update (the first on a map, and
one that grows its scratch), one ks_debug_radix_sort and one growing ks_integrate_points call on a live context fails once: the
call returns an error, ks_destroy balances the ledger, and — upload, mesh, sort — the call repeated without injection gives the
result of a context that never failed.  (An upload that has to grow the pool is swept too; grow_pool's first allocation may fail
without an error, by design, so that case only asks for no crash and a balanced ledger.)"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "emu", "_build", "libks_hip_emu.so")

BALANCE = ["fast_default", "fast_pipelined", "fast_phased", "merged_reference", "merged_anti_grazing", "grow_points", "grow_pool", "mesh",
           "block_io", "clear_mid_stream", "radix_sort", "round_exact_fast", "round_exact_merged"]
SWEEPS = ["create_fast", "create_merged", "create_pipelined", "upload", "upload_growing_pool", "mesh", "mesh_first", "grow_points", "radix_sort"]
CASES = {"balance_" + n: {"balance": n} for n in BALANCE}
CASES.update({"sweep_" + n: {"sweep": n} for n in SWEEPS})


@pytest.fixture(scope="module")
def children(request):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("host clang++ of the ROCm toolchain not found")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emu", "build_emu.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    wanted = {it.callspec.params["name"] for it in request.session.items if str(it.fspath) == str(request.fspath) and hasattr(it, "callspec")}
    procs = {}
    for name in sorted(wanted or CASES):
        procs[name] = subprocess.Popen([sys.executable, "-m", "tests.ownership_case", json.dumps(CASES[name])], cwd=ROOT,
                                       env=dict(os.environ, KS_HIP_LIB=LIB), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    yield procs
    for p in procs.values():
        if p.poll() is None:
            p.kill()
            p.communicate()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_resource_of_a_context_has_one_owner(children, name):
    p = children[name]
    try:
        out, err = p.communicate(timeout=1500)
    except subprocess.TimeoutExpired:
        p.kill()
        out, err = p.communicate()
        err += "\n[timed out]"
    assert p.returncode == 0 and "OWNERSHIP_OK" in out, out[-3000:] + err[-3000:]
