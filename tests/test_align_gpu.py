"""GPU tier of the scan alignment: the cases of tests/align_case.py on the real device (the same sizes as on the functional
model), the device-pointer call on a torch tensor, one alignment called while frames are in flight, and the adapter.  The
checker is tests/align_model.py; every comparison is exact and covers the refined pose and every stats field."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import align_case, align_model

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(align_case.SPECS))
def test_align_equals_model(name):
    align_case.run_case(align_case.SPECS[name])


def test_device_pointer_call_on_a_torch_tensor_equals_the_host_call():
    """ks_align_points_device reads the cloud on ks_stream(ctx); 1000 points, stride 3: the same bytes as the host call."""
    import torch
    from tests import mesh_case, render_case
    T_true = render_case.CAMERAS["front"]
    T0 = align_case.perturbed(T_true)
    xyz = align_case.surface_cloud("sphere", 1000, T_true)
    xyz[5::9, 1] = np.nan
    g = mesh_case._integrator(0, 64, 48, vps=8)
    g.upload(*mesh_case.make_field("sphere", 8))
    want = g.align(T0, xyz, point_stride=3)
    assert want[1]["inliers_first"] > 200 and want[1]["iterations"] > 0
    d = torch.from_numpy(xyz).to("cuda")
    torch.cuda.synchronize()
    got = g.align_device(T0, d.data_ptr(), len(xyz), point_stride=3)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], (got, want)
    align_model.assert_same(got, align_model.model_of(g, T0, xyz, dict(point_stride=3)), "device pointer")
    g.close()


def test_align_with_frames_in_flight_equals_model():
    """Four 160 x 120 frames at 5 cm through the frame pipeline (pipeline_frames = 12), the fourth frame's cloud aligned from
    its perturbed pose straight after the fourth integrate (19200 pixels: up to 300 wavefronts, the finisher's strided loop runs
    twice), against the model on the map downloaded afterwards."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    from tests.util import COMMON
    w, h = 160, 120
    sc = synth.make_scene("room")
    frames = [synth.render_frame(sc, synth.trajectory_pose(5 * k), w, h, hfov_deg=90.0, seed=40 + k) for k in range(4)]
    g = B.HipIntegrator(B.default_config(method=0, voxel_size=0.05, voxels_per_side=16, truncation_distance=0.2, max_ray_length_m=5.0,
                                         max_tiles=1 << 13, max_points=w * h, pipeline_frames=12, **COMMON))
    for f in frames:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    assert g.pipeline_shape()["lag"] > 0
    f = frames[-1]
    T0 = align_case.perturbed(f.T_G_C)
    got = g.align(T0, f.xyz)
    model = align_model.model_of(g, T0, f.xyz)
    print("in flight:", got, "model", model[:2], "error", align_case.pose_error(T0, f.T_G_C), "->", align_case.pose_error(got[0], f.T_G_C))
    align_model.assert_same(got, model, "in flight")
    assert len(f.xyz) > 256 * 64 and got[1]["inliers_first"] > 0.3 * got[1]["points_used"] and got[1]["iterations"] > 0
    g.close()


def test_adapter_align_point_cloud_equals_model_on_the_layers_it_synced(tmp_path):
    """HipSemanticTsdfIntegrator::alignPointCloud of the last frame's cloud from that frame's perturbed pose (adapter_demo,
    KS_DEMO_ALIGN) against the model on the layers the demo wrote."""
    import ctypes
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import test_host_adapter_gpu as A
    from tests.util import NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    csv, fin, fout, falign = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin", "align.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    frames = A._frames()
    A._write_in(fin, frames)
    res = subprocess.run([A.DEMO, "fast", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True,
                         env=dict(os.environ, KS_DEMO_ALIGN=falign))
    assert res.returncode == 0 and "adapter_demo: alignPointCloud" in res.stdout, res.stdout + res.stderr
    idx, t, s = A._read_out(fout)
    buf = open(falign, "rb").read()
    assert len(buf) == 56 + 48
    T_in, T_out = np.frombuffer(buf, "<f4", 7, 0).copy(), np.frombuffer(buf, "<f4", 7, 28).copy()
    st = B.KsAlignStats.from_buffer_copy(buf[56:])
    stats = B.HipIntegrator._align_stats(st)
    assert np.abs(T_in - align_case.perturbed(frames[-1].T_G_C)).max() < 1e-6
    model = align_model.align_from_blocks(idx, t, s, 16, 0.05, 0.2, T_in, frames[-1].xyz)
    align_model.assert_same((T_out, stats), model, "adapter")
    assert stats["iterations"] > 0 and stats["inliers_first"] > 0.3 * stats["points_used"], stats
    e0, e1 = align_case.pose_error(T_in, frames[-1].T_G_C), align_case.pose_error(T_out, frames[-1].T_G_C)
    print("adapter:", stats, e0, "->", e1)
