"""CPU tier: the stream plan — which chain of a frame runs on which stream, fitted into the hardware queues the process has
(csrc/ks_hip.hip: stream_plan; ks_stream_plan) — on the host functional model of the library (tools/emu), whose runtime stand-in
keeps a ledger of the live streams.  The cases are in tests/stream_plan_case.py; every case is one child process, they run side
by side.

table: budgets 1, 3, 4, 5, 6, 8 and 32 (through KS_DEBUG=1 KS_HW_QUEUES; without it the budget is what the inherited environment's
GPU_MAX_HW_QUEUES says, which the library only reads and no test writes) x `fast` in its default mode at pipeline_frames 0 / 4 / 8 / 12 / 16, `fast` with ordered phases at 4 and 12, `merged`
at 0 and 8: ks_stream_plan equals the table written out in the case file, the ledger holds as many more streams after ks_create
as the plan has distinct ones — an alias is the same stream, created once — and is back where it was after ks_destroy.

stream_*: 32 small frames through the pipelined default mode at a budget of 4 (both side chains on the stage-T stream), 5 (the
xlong chain alone) and 8 (the layout as it always was), and through the unpipelined context at a budget of 1 (one stream for
everything): the blocks, every voxel and the summed frame statistics equal the unpipelined three-stream context's, bit for bit.
The stream holds frames whose marks do not fit KS_EXACT_CAP_MARKS (the fallback to the host-driven loop) and frames that outgrow
max_points (every slot's buffers grow): both drain the pipeline.

tsan: tools/emu/run_tsan.sh — the frame pipeline with its helper thread under ThreadSanitizer, streams and events modelled as the
happens-before edges they stand for — over the budget-4 plan of the headline context (pipeline_frames = 12): no report."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "emu", "_build", "libks_hip_emu.so")

CASES = {
    "table": dict(table=1),
    "stream_pipeline12_budget4": dict(stream=dict(pipeline=12, budget=4, streams=4)),
    "stream_pipeline12_budget5": dict(stream=dict(pipeline=12, budget=5, streams=5)),
    "stream_pipeline12_budget8": dict(stream=dict(pipeline=12, budget=8, streams=6)),
    "stream_pipeline16_budget4": dict(stream=dict(pipeline=16, budget=4, streams=4)),
    "stream_unpipelined_budget1": dict(stream=dict(pipeline=0, budget=1, streams=1, min_fallbacks=0)),
}


def _have_toolchain():
    return os.path.exists("/opt/rocm/lib/llvm/bin/clang++")


@pytest.fixture(scope="module")
def children(request):
    if not _have_toolchain():
        pytest.skip("host clang++ of the ROCm toolchain not found")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emu", "build_emu.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    wanted = {it.callspec.params["name"] for it in request.session.items if str(it.fspath) == str(request.fspath) and hasattr(it, "callspec")}
    env = {k: v for k, v in os.environ.items() if k not in ("KS_DEBUG", "KS_HW_QUEUES")}
    procs = {}
    for name in sorted(wanted or CASES):
        procs[name] = subprocess.Popen([sys.executable, "-m", "tests.stream_plan_case", json.dumps(CASES[name])], cwd=ROOT,
                                       env=dict(env, KS_HIP_LIB=LIB), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    yield procs
    for p in procs.values():
        if p.poll() is None:
            p.kill()
            p.communicate()


@pytest.mark.parametrize("name", sorted(CASES))
def test_stream_plan_on_the_functional_model(children, name):
    p = children[name]
    try:
        out, err = p.communicate(timeout=1500)
    except subprocess.TimeoutExpired:
        p.kill()
        out, err = p.communicate()
        err += "\n[timed out]"
    assert p.returncode == 0 and "STREAM_PLAN_OK" in out, out[-3000:] + err[-3000:]


def test_thread_sanitizer_over_the_budget_4_plan():
    if not _have_toolchain():
        pytest.skip("host clang++ of the ROCm toolchain not found")
    env = dict(os.environ)
    env.update(KS_DEBUG="1", KS_HW_QUEUES="4", TSAN_CASES="0 12 16 24 18", TSAN_TAIL="400")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emu", "run_tsan.sh")], capture_output=True, text=True, env=env, timeout=1500)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "method 0 pipeline 12: 16 frames of 24x18" in out, out[-4000:]   # (the run completed)
    assert "ThreadSanitizer" not in out, out[-6000:]
