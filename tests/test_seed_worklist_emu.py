"""CPU tier: the early-out seed's work list (k_seed_list -> k_test) on the host functional model of the device code (tools/emu),
against the oracle — tests/seed_case.py: frames of 1, 1023, 1024, 2047, 2048, 3047 and 5000 points, a frame whose rays are all
live and one with none, integrated one after the other into a context of 7000 points (capacity != n: the seed's launches and
its lists are sized by the capacity), unpipelined and in batches of four frames per launch; the ordered-phase mode against its
CPU restatement and the default mode against the reference's serial loop; and the guard for a list that does not fit its launch.
Every case is one child process; they run side by side."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "emu", "_build", "libks_hip_emu.so")

CASES = {
    "phased_unpipelined": (dict(mode="phased", pipeline=0), {}),
    "phased_batches_of_four": (dict(mode="phased", pipeline=8), {}),
    "serial_unpipelined": (dict(mode="serial", pipeline=0), {}),
    "serial_batches_of_four": (dict(mode="serial", pipeline=8), {}),
    # the other reading of the "mixed" order: 1024 chains whatever n, n / 1024 generations
    "phased_1024_groups": (dict(mode="phased", pipeline=0, order=2), {}),
    "phased_sorted_order": (dict(mode="phased", pipeline=0, order=1, sizes=[1023, 3047]), {}),
    "overflow_phased": (dict(mode="phased", overflow=True), {"KS_DEBUG": "1", "KS_SEED_CAP_ITEMS": "4"}),
    "overflow_serial": (dict(mode="serial", overflow=True), {"KS_DEBUG": "1", "KS_SEED_CAP_ITEMS": "4"}),
}


@pytest.fixture(scope="module")
def children(request):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("host clang++ of the ROCm toolchain not found")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emu", "build_emu.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    wanted = {it.callspec.params["name"] for it in request.session.items if str(it.fspath) == str(request.fspath) and hasattr(it, "callspec")}
    procs = {}
    for name in sorted(wanted or CASES):
        spec, env = CASES[name]
        procs[name] = subprocess.Popen([sys.executable, "-m", "tests.seed_case", json.dumps(spec)], cwd=ROOT,
                                       env=dict(os.environ, KS_HIP_LIB=LIB, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    yield procs
    for p in procs.values():
        if p.poll() is None:
            p.kill()
            p.communicate()


@pytest.mark.parametrize("name", sorted(CASES))
def test_seed_work_list_on_the_functional_model_equals_oracle(children, name):
    p = children[name]
    try:
        out, err = p.communicate(timeout=900)
    except subprocess.TimeoutExpired:
        p.kill()
        out, err = p.communicate()
        err += "\n[timed out]"
    assert p.returncode == 0 and "SEED_CASE_OK" in out, out[-3000:] + err[-3000:]
