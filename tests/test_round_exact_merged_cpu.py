"""CPU tier: the EXACT frame-sharded rounds of `merged` (ks_integrate_round_exact, method = 1) on the host functional model of
the library (tools/emu), two ranks exchanging their records and tables through the librccl test double.

64x48 frames with 10 cm voxels: at 48x36 / 5 cm (the `fast` test's size) no frame has a mixed-label bundle; here every one of
the four has some, and the sensor's voxel collects one update per bundle (~1 900) — both asserted below from a numpy count."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from kimera_semantics_amd import binding as B
from kimera_semantics_amd import parallel as PAR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
WORKER = os.path.join(ROOT, "tests", "round_merged_worker.py")
LONG_RUN = 32   # kLongRun (csrc/ks_types.h): a run of more updates is taken by wavefronts


def _model_and_double(tmp_path):
    if not os.path.exists(CXX):
        pytest.skip("host clang++ of the ROCm toolchain not found")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emu", "build_emu.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    emu = os.path.join(ROOT, "tools", "emu", "_build", "libks_hip_emu.so")
    mock = str(tmp_path / "libmock_rccl_emu.so")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-fPIC", "-shared", "-DKS_EMU_BUILD", "-Wno-unknown-attributes", "-I", os.path.join(ROOT, "tools", "emu"),
                        "-o", mock, os.path.join(ROOT, "tests", "mock_rccl", "mock_rccl.cpp"), "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(mock)

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_byte * 128)]
    uid = UniqueId()
    assert lib.ncclGetUniqueId(C.byref(uid)) == 0
    env = dict(os.environ, KS_HIP_LIB=emu, KS_RCCL_LIB=mock, KS_ROUND_WH="64x48", KS_ROUND_VOXEL="0.1")
    return env, bytes(uid).hex()


def _run_all(procs, timeout):
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("a rank hung")
        outs.append(o)
    return outs


def test_the_frames_have_mixed_label_bundles_and_a_long_run(monkeypatch):
    """What the round test below relies on, from numpy alone (never from the code under test)."""
    from tests.round_merged_worker import bundle_census, round_frames
    monkeypatch.setenv("KS_ROUND_WH", "64x48")
    for f in round_frames(4):
        bundles, mixed = bundle_census(f, 0.1)
        assert mixed > 0 and bundles > LONG_RUN, (bundles, mixed)


def test_merged_round_two_ranks_on_the_functional_model_is_the_sequential_map(tmp_path):
    """World 2, two rounds, plus the sequential process: the tiles a rank owns are the tiles of ONE `merged` context integrating
    the four frames in order, bit for bit; every byte that left a rank is counted (records, bundle tables, mixed-label rows).
    (The three processes take 16 - 18 s on the functional model, printed below.)"""
    env, uid = _model_and_double(tmp_path)
    world, n_rounds = 2, 2
    t0 = time.time()
    procs = [subprocess.Popen([sys.executable, WORKER, str(rk), str(world), uid, str(tmp_path), f"round:{n_rounds}"], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rk in range(world)]
    procs.append(subprocess.Popen([sys.executable, WORKER, "seq", str(tmp_path), str(world * n_rounds)], env=env, stdout=subprocess.PIPE,
                                  stderr=subprocess.STDOUT, text=True))
    outs = _run_all(procs, 900)
    print("three processes on the functional model: %.1f s" % (time.time() - t0))
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    with np.load(os.path.join(str(tmp_path), "round_seq.npz")) as npz:
        want = dict(zip(npz["keys"].tolist(), npz["rec"]))
    owners = PAR.owner_of(np.array(sorted(want), dtype=np.uint64), world)
    marched = applied = 0
    for rk in range(world):
        with np.load(os.path.join(str(tmp_path), f"round_rank{rk}.npz")) as npz:
            got = {k: npz[k] for k in npz.files}
        assert not got["origin"].any()   # always 0 for `merged`
        mine = {k for k, ow in zip(sorted(want), owners.tolist()) if ow == rk}
        assert set(got["keys"].tolist()) == mine
        for i, k in enumerate(got["keys"].tolist()):
            assert np.array_equal(got["rec"][i], want[k]), f"rank {rk} tile {k}"
        marched += int(got["marched"].sum())
        applied += int(got["applied"].sum())
        assert int(got["sent"].sum()) > 0
    assert marched == applied > 0


def test_a_failing_rank_does_not_hang_its_peer_on_the_functional_model(tmp_path):
    """Rank 1 passes a label 21 in round 0: both processes come back within the timeout, both with an error whose text names
    the cause — rank 1 its own (the label), rank 0 the rank that failed — and rank 0 has applied nothing."""
    env, uid = _model_and_double(tmp_path)
    procs = [subprocess.Popen([sys.executable, WORKER, str(rk), "2", uid, str(tmp_path), "fail"], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for rk in range(2)]
    outs = _run_all(procs, 600)
    assert all(p.returncode == 3 for p in procs), "\n".join(outs)
    res = [json.load(open(os.path.join(str(tmp_path), f"fail_rank{rk}.json"))) for rk in range(2)]
    assert res[1]["code"] == B.KS_ERR_LABEL_RANGE and "label" in res[1]["text"], res
    assert res[0]["code"] == B.KS_ERR_PEER_FAILED and "rank 1" in res[0]["text"] and str(B.KS_ERR_LABEL_RANGE) in res[0]["text"], res
    assert res[0]["tiles_after"] == 0 and res[1]["tiles_after"] == 0, res


def test_the_peer_failure_code_mirrors_the_header():
    """KS_ERR_PEER_FAILED is the last entry of the header's enum and the binding carries the same value."""
    import re
    text = open(os.path.join(ROOT, "include", "ks_hip.h")).read()
    codes = re.findall(r"^\s*(KS_ERR_[A-Z_]+) = (-\d+)", text, flags=re.M)
    assert codes[-1] == ("KS_ERR_PEER_FAILED", str(B.KS_ERR_PEER_FAILED))
    assert dict(codes)["KS_ERR_INVALID_ARG"] == str(B.KS_ERR_INVALID_ARG)
    assert len({v for _, v in codes}) == len(codes)
