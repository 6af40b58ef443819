"""CPU tier: the tail of a batch of frames in one pass (csrc/ks_hip.hip: tail_batch) on the host functional model of the library
(tools/emu).  Three cases of tests/tail_batch_case.py at 64 x 48, one child process each, side by side: the default tail against
KS_DEBUG=1 KS_TAIL_BATCH=0 and against the serial CPU oracle (batches of 4, 4 and a partial 3), point counts on both sides of a
power of two inside one batch, and a label outside the table in the middle of a batch (the same error code at the same call, the
batch frame by frame)."""
import json
import os
import subprocess
import sys

import pytest

from tests.tail_batch_case import EMU_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "emu", "_build", "libks_hip_emu.so")


@pytest.fixture(scope="module")
def children(request):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("host clang++ of the ROCm toolchain not found")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emu", "build_emu.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    wanted = {it.callspec.params["name"] for it in request.session.items if str(it.fspath) == str(request.fspath) and hasattr(it, "callspec")}
    env = {k: v for k, v in os.environ.items() if k not in ("KS_DEBUG", "KS_TAIL_BATCH")}
    procs = {}
    for name in sorted(wanted or EMU_CASES):
        procs[name] = subprocess.Popen([sys.executable, "-m", "tests.tail_batch_case", json.dumps(EMU_CASES[name])], cwd=ROOT,
                                       env=dict(env, KS_HIP_LIB=LIB), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    yield procs
    for p in procs.values():
        if p.poll() is None:
            p.kill()
            p.communicate()


@pytest.mark.parametrize("name", sorted(EMU_CASES))
def test_batch_tail_on_the_functional_model(children, name):
    p = children[name]
    try:
        out, err = p.communicate(timeout=1500)
    except subprocess.TimeoutExpired:
        p.kill()
        out, err = p.communicate()
        err += "\n[timed out]"
    assert p.returncode == 0 and "TAIL_BATCH_OK" in out, out[-3000:] + err[-3000:]
