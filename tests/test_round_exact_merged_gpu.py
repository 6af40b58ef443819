"""-m gpu: the EXACT frame-sharded integration of `merged` (ks_integrate_round_exact with method = 1, csrc/ks_k_shard_merged.h).

The owners' tiles must be, bit for bit, what ONE `merged` context integrating the frames in order holds — and therefore the
serial oracle's and the real reference's map.  The frames are those of the `fast` round tests (tests/reduce_worker.round_frames);
a numpy count asserts that every one of them has mixed-label bundles (the 21-float vectors travel) and a voxel run far longer
than the wavefront threshold (the sensor's voxel: one update per bundle)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from kimera_semantics_amd import binding as B
from kimera_semantics_amd import parallel as PAR
from kimera_semantics_amd import synth
from oracle import oracle_py as O
from oracle import ref_py as R
from tests.reduce_worker import export_all, round_frames
from tests.round_merged_worker import bundle_census, merged_config_kw
from tests.util import compare_maps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "mock_rccl", "libmock_rccl.so")
WORKER = os.path.join(ROOT, "tests", "round_merged_worker.py")
LONG_RUN = 32   # kLongRun (csrc/ks_types.h): a run of more updates is taken by wavefronts


def _ctx(max_tiles=4096, max_points=1 << 15, **kw):
    return B.HipIntegrator(B.default_config(max_tiles=max_tiles, max_points=max_points, **merged_config_kw(**kw)))


def _tiles(h):
    keys, rec = export_all(h)
    return dict(zip(keys.tolist(), rec[:, :, :25]))


def _assert_same_tiles(got, want):
    assert sorted(got) == sorted(want)
    for k in got:
        assert np.array_equal(got[k], want[k]), k


def _full_size_frames():
    sc = synth.make_scene("room")
    return [synth.render_frame(sc, synth.arc_pose(k, 8), 640, 480, seed=100 + k) for k in range(8)]


def _spawn(tmp_path, world, what):
    if not os.path.exists(MOCK):
        pytest.fail("tests/mock_rccl/libmock_rccl.so not built: run __graft_entry__.build()")
    lib = C.CDLL(MOCK)

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_byte * 128)]
    uid = UniqueId()
    assert lib.ncclGetUniqueId(C.byref(uid)) == 0
    env = dict(os.environ, KS_RCCL_LIB=MOCK)
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), bytes(uid).hex(), str(tmp_path), what], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("a rank hung")
        outs.append(out)
    return procs, outs


def test_the_frames_have_mixed_label_bundles_and_long_runs():
    """Counted with numpy, never by the code under test: the tests below exercise the tables and the long-run kernel."""
    for f in round_frames(4) + round_frames(6) + _full_size_frames():
        bundles, mixed = bundle_census(f, 0.05)
        assert mixed > 0 and bundles > LONG_RUN, (bundles, mixed)


@pytest.mark.parametrize("bundle_order", [0, 1])
@pytest.mark.parametrize("color_mode", [1, 2])
def test_merged_round_on_one_rank_is_the_sequential_map_the_oracle_and_the_reference(tmp_path, color_mode, bundle_order):
    kw = dict(color_mode=color_mode, bundle_order=bundle_order)
    frames = round_frames(4)
    marcher, owner, seq = _ctx(**kw), _ctx(**kw), _ctx(**kw)
    o = O.Oracle(O.default_config(integrator_threads=1, **merged_config_kw(**kw)))
    ref = None
    if R.available() and bundle_order == 0:   # (the reference has its container's order only)
        csv = str(tmp_path / "labels.csv")
        R.write_label_csv(csv, synth.default_label_colors())
        ref = R.Reference("merged", csv, voxel_size=0.05, vps=8, truncation=0.2, max_ray=5.0, order_mode="mixed", color_mode=color_mode)
    for k, f in enumerate(frames):
        so = o.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        st = owner.integrate_round_exact(marcher, None, 0, 1, k, f.T_G_C, f.xyz, f.rgba, f.labels)
        seq.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        if ref is not None:
            ref.integrate(f.T_G_C, f.xyz, f.rgba)
        print("frame", k, st, "oracle updates", so.n_voxel_updates, "oracle rays", so.n_rays_cast)
        assert st["updates_marched"] == st["updates_applied"] == so.n_voxel_updates, st
        assert not st["origin_voxel_touched"] and st["rays_cast"] == so.n_rays_cast and st["bytes_sent"] == 0, st
    _assert_same_tiles(_tiles(owner), _tiles(seq))
    compare_maps(o, owner, exact=True)
    if ref is not None:
        ri = ref.block_indices()
        assert np.array_equal(ri, owner.block_indices()), "allocated block sets differ"
        _, rt, rs = ref.download(ri)
        _, ht, hs = owner.download(ri)
        if color_mode == 2:  # colours through exp(): a colour LSB may differ on <= 1e-3 of the voxels (tests/test_hip_vs_ref_gpu.py)
            assert (rt["color"] != ht["color"]).any(axis=-1).mean() <= 1e-3
            ht["color"] = rt["color"]
        assert np.array_equal(rs["label"], hs["label"])
        assert np.array_equal(rs["priors"].view(np.uint32), hs["priors"].view(np.uint32))
        assert np.array_equal(rt["distance"].view(np.uint32), ht["distance"].view(np.uint32))
        assert np.array_equal(rt["weight"].view(np.uint32), ht["weight"].view(np.uint32))
        assert np.array_equal(rt["color"], ht["color"]) and np.array_equal(rs["color"], hs["color"])


@pytest.mark.parametrize("world", [2, 3])
def test_merged_round_multi_rank_is_the_sequential_map_bit_for_bit(tmp_path, world):
    """Two rounds over 2 / 3 ranks (processes sharing the GPU, the librccl test double): each rank's tiles are the tiles it owns
    of the sequential `merged` map, bit for bit; the bytes a rank reports as sent include the two tables."""
    n_rounds = 2
    procs, outs = _spawn(tmp_path, world, f"round:{n_rounds}")
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    seq = _ctx()
    for f in round_frames(world * n_rounds):
        seq.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    want = _tiles(seq)
    want_owner = PAR.owner_of(np.array(sorted(want), dtype=np.uint64), world)
    want_by_rank = {r: {k for k, ow in zip(sorted(want), want_owner.tolist()) if ow == r} for r in range(world)}
    marched = applied = sent = 0
    for r in range(world):
        with np.load(os.path.join(str(tmp_path), f"round_rank{r}.npz")) as npz:
            got = {k: npz[k] for k in npz.files}
        assert not got["origin"].any()
        marched += int(got["marched"].sum())
        applied += int(got["applied"].sum())
        assert int(got["sent"].sum()) > 0
        sent += int(got["sent"].sum())
        gk = got["keys"].tolist()
        assert set(gk) == want_by_rank[r], f"rank {r}: the tiles it holds are not the tiles it owns of the sequential map"
        for i, k in enumerate(gk):
            assert np.array_equal(got["rec"][i], want[k]), f"rank {r} tile {k}"
    assert marched == applied > 0
    print("world", world, "bytes sent per update marched", sent / marched)


def test_merged_round_full_size_frames_are_the_sequential_map():
    """Eight 640x480 arc-pose frames (BASELINE configuration 5's shape) at world 1 against one plain `merged` context."""
    big = dict(max_tiles=1 << 15, max_points=1 << 19)
    marcher, owner, seq = _ctx(**big), _ctx(**big), _ctx(**big)
    for k, f in enumerate(_full_size_frames()):
        st = owner.integrate_round_exact(marcher, None, 0, 1, k, f.T_G_C, f.xyz, f.rgba, f.labels)
        fs = seq.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        assert st["updates_marched"] == st["updates_applied"] == fs.n_voxel_updates > 0, (st, fs.n_voxel_updates)
    _assert_same_tiles(_tiles(owner), _tiles(seq))


def test_merged_round_refusals():
    f = round_frames(1)[0]
    args = (None, 0, 1, 0, f.T_G_C, f.xyz, f.rgba, f.labels)

    def piped():
        return B.HipIntegrator(B.default_config(max_tiles=4096, max_points=1 << 15, pipeline_frames=4, **merged_config_kw()))
    fast = B.HipIntegrator(B.default_config(max_tiles=4096, max_points=1 << 15, **dict(merged_config_kw(), method=0)))
    with pytest.raises(B.KsError) as e:
        fast.integrate_round_exact(_ctx(), *args)   # a `merged` marcher, a `fast` owner
    assert e.value.code == B.KS_ERR_UNSUPPORTED and "same method" in str(e.value)
    with pytest.raises(B.KsError) as e:
        _ctx(color_mode=0).integrate_round_exact(_ctx(color_mode=0), *args)
    assert e.value.code == B.KS_ERR_UNSUPPORTED and "KS_COLOR_MODE_COLOR" in str(e.value)
    with pytest.raises(B.KsError) as e:
        piped().integrate_round_exact(piped(), *args)
    assert e.value.code == B.KS_ERR_UNSUPPORTED and "pipeline_frames" in str(e.value)
    # a cloud the record's 24-bit position cannot index: refused before anything is read (the buffers here are one frame's)
    marcher, owner = _ctx(), _ctx()
    T = np.ascontiguousarray(f.T_G_C, dtype=np.float32)
    xyz, rgba, labels = (np.ascontiguousarray(a) for a in (f.xyz, f.rgba, f.labels))
    st = B.KsRoundStats()
    rc = B.lib().ks_integrate_round_exact(marcher._h, owner._h, None, 0, 1, 0, T.ctypes.data, xyz.ctypes.data, rgba.ctypes.data,
                                          labels.ctypes.data, 1 << 24, 0, C.byref(st))
    assert rc == B.KS_ERR_INVALID_ARG and "2^24" in B.lib().ks_last_error(owner._h).decode()
    # ... and the pair still works afterwards
    st = owner.integrate_round_exact(marcher, *args)
    assert st["updates_marched"] == st["updates_applied"] > 0


def test_a_failing_rank_does_not_hang_its_peer(tmp_path):
    """World 2 through the test double, rank 1 passes a label 21 in round 0: both processes come back within the timeout, both
    with an error whose text names the cause.  (Host logic: the label is refused by the range check, nothing faults.)"""
    procs, outs = _spawn(tmp_path, 2, "fail")
    assert all(p.returncode == 3 for p in procs), "\n".join(outs)
    res = [json.load(open(os.path.join(str(tmp_path), f"fail_rank{r}.json"))) for r in range(2)]
    assert res[1]["code"] == B.KS_ERR_LABEL_RANGE and "label" in res[1]["text"], res
    assert res[0]["code"] == B.KS_ERR_PEER_FAILED and "rank 1" in res[0]["text"], res
    assert res[0]["tiles_after"] == 0 and res[1]["tiles_after"] == 0, res
