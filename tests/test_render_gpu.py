"""GPU tier of the view rendering: the cases of tests/render_case.py on the real device (the same sizes as on the functional
model), the device-pointer call into torch tensors, one full-size view rendered while frames are in flight, and the adapter.
The checker is tests/render_model.py; every comparison is exact and covers all four images and the stats."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import render_case, render_model

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(render_case.SPECS))
def test_render_equals_model(name):
    render_case.run_case(render_case.SPECS[name])


def test_device_pointer_call_into_torch_tensors_equals_the_host_call():
    """ks_render_view_device on ks_stream(ctx): with stats the call has waited for the kernel; without, the tensors are read
    after the context's own synchronize.  61 x 45: edge tiles on both axes."""
    import torch
    from tests import mesh_case
    w, h = 61, 45
    T, K = render_case.CAMERAS["front"], render_case.K_ODD
    g = mesh_case._integrator(0, 64, 48, vps=8)
    g.upload(*mesh_case.make_field("two_label", 8))
    want = g.render(T, K, w, h)
    assert want[4]["pixels_hit"] > 1000

    def tensors():
        return (torch.full((h, w), 7.0, dtype=torch.float32, device="cuda"), torch.full((h, w), 9, dtype=torch.uint8, device="cuda"),
                torch.full((h, w, 4), 9, dtype=torch.uint8, device="cuda"), torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda"))

    d = tensors()
    torch.cuda.synchronize()
    stats = g.render_device(T, K, w, h, *[t.data_ptr() for t in d])
    assert stats == want[4]
    for a, b in zip(d, want[:4]):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    d = tensors()
    torch.cuda.synchronize()
    assert g.render_device(T, K, w, h, d[0].data_ptr(), d[1].data_ptr(), 0, 0, stats=False) is None   # (enqueued; no host wait)
    g.synchronize()
    assert d[0].cpu().numpy().tobytes() == want[0].tobytes() and d[1].cpu().numpy().tobytes() == want[1].tobytes()
    assert (d[2].cpu().numpy() == 9).all() and (d[3].cpu().numpy() == 7.0).all()   # (outputs that were not asked for are not written)
    g.close()


def test_full_size_view_with_frames_in_flight_equals_model():
    """Four 640 x 480 frames at 5 cm through the frame pipeline (pipeline_frames = 12), rendered at 640 x 480 from the last
    pose straight after the fourth integrate: 80 x 60 pixel tiles, the edge guard at full width, long rays beside short ones in
    one wavefront.  The model on the CPU oracle's map of these frames hits 83.5 % of the pixels."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    from tests.util import COMMON
    w, h = 640, 480
    sc = synth.make_scene("room")
    frames = [synth.render_frame(sc, synth.trajectory_pose(5 * k), w, h, hfov_deg=90.0, seed=40 + k) for k in range(4)]
    g = B.HipIntegrator(B.default_config(method=0, voxel_size=0.05, voxels_per_side=16, truncation_distance=0.2, max_ray_length_m=5.0,
                                         max_tiles=1 << 13, max_points=w * h, pipeline_frames=12, **COMMON))
    for f in frames:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    assert g.pipeline_shape()["lag"] > 0
    f = frames[-1]
    got = g.render(f.T_G_C, f.K, w, h)
    model = render_model.model_of(g, f.T_G_C, f.K, w, h)
    print("full size:", got[4], "model", model["stats"])
    render_model.assert_same(got, model, "full size")
    assert got[4]["pixels_hit"] > 0.5 * w * h, got[4]
    assert len(np.unique(got[1][got[1] != 255])) >= 3
    g.close()


def test_adapter_render_view_equals_model_on_the_layers_it_synced(tmp_path):
    """HipSemanticTsdfIntegrator::renderView from the last frame's pose (adapter_demo, KS_DEMO_RENDER) against the model on
    the layers the demo wrote."""
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import test_host_adapter_gpu as A
    from tests.util import NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    csv, fin, fout, fview = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin", "view.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    frames = A._frames()
    A._write_in(fin, frames)
    res = subprocess.run([A.DEMO, "fast", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True,
                         env=dict(os.environ, KS_DEMO_RENDER=fview))
    assert res.returncode == 0 and "adapter_demo: renderView" in res.stdout, res.stdout + res.stderr
    idx, t, s = A._read_out(fout)
    buf = open(fview, "rb").read()
    w, h = struct.unpack_from("<II", buf, 0)
    T, K = np.frombuffer(buf, "<f4", 7, 8), np.frombuffer(buf, "<f4", 4, 36)
    n, off = w * h, 52
    assert (w, h) == (128, 96) and T.tobytes() == frames[-1].T_G_C.astype("<f4").tobytes() and len(buf) == off + n * (4 + 1 + 4 + 12) + 24
    depth = np.frombuffer(buf, "<f4", n, off).reshape(h, w)
    labels = np.frombuffer(buf, np.uint8, n, off + 4 * n).reshape(h, w)
    rgba = np.frombuffer(buf, np.uint8, 4 * n, off + 5 * n).reshape(h, w, 4)
    normals = np.frombuffer(buf, "<f4", 3 * n, off + 9 * n).reshape(h, w, 3)
    hit, missed, samples = struct.unpack_from("<3Q", buf, off + 21 * n)
    model = render_model.render_from_blocks(idx, t, s, 16, 0.05, T, K, w, h)
    render_model.assert_same((depth, labels, rgba, normals, dict(pixels_hit=hit, pixels_missed=missed, samples=samples)), model, "adapter")
    assert hit > 0.3 * n and len(np.unique(labels[labels != 255])) >= 2
