"""GPU tier of the ESDF reads: the cases of tests/esdf_read_case.py on the real device (the same sizes as on the functional model),
one larger map read while frames are in flight, the device-pointer calls on torch tensors, and the adapter.  The checker is
tests/esdf_read_model.py on the stored ESDF as the library hands it out; every comparison is exact, statistics included."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import esdf_case, esdf_model, esdf_read_case
from tests import esdf_read_model as M

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.mark.parametrize("name", sorted(esdf_read_case.SPECS))
def test_esdf_read_equals_model(name, monkeypatch):
    spec, env = esdf_read_case.SPECS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    esdf_read_case.run_case(spec)


def test_larger_map_read_with_frames_in_flight_equals_model():
    """Four 160x120 frames at 5 cm through the frame pipeline (pipeline_frames = 12).  The ESDF is made after two frames and
    refreshed straight after the fourth integrate, while frames are in flight; then 20 000 points, 2000 segments and a 160 x 120
    slice against the model on the store the library hands out."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    from tests.util import COMMON
    sc = synth.make_scene("room")
    frames = [synth.render_frame(sc, synth.trajectory_pose(k, radius=1.5), 160, 120, hfov_deg=90.0, seed=k) for k in range(4)]
    g = B.HipIntegrator(B.default_config(method=0, voxel_size=0.05, voxels_per_side=16, truncation_distance=0.2, max_ray_length_m=5.0,
                                         max_tiles=1 << 13, max_points=160 * 120, pipeline_frames=12, **COMMON))
    for f in frames[:2]:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.esdf_update(min_distance_m=0.1, max_distance_m=1.0)
    for f in frames[2:]:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    g.esdf_refresh()
    idx = g.block_indices()
    vs, side = 0.05, 16 * 0.05
    lo, hi = idx.min(axis=0) * side, (idx.max(axis=0) + 1) * side
    rng = np.random.default_rng(11)
    xyz = rng.uniform(lo - 0.2, hi + 0.2, (20000, 3)).astype(F)
    a = rng.uniform(lo, hi, (2000, 3))
    d = rng.normal(size=(2000, 3))
    seg = np.concatenate([a, a + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.2, 3.0, (2000, 1))], axis=1).astype(F)
    z = float(frames[-1].T_G_C[6])
    w, h = 160, 120
    o, du, dv = np.array([lo[0], lo[1], z], F), np.array([(hi[0] - lo[0]) / w, 0, 0], F), np.array([0, (hi[1] - lo[1]) / h, 0], F)
    got_p, got_s, got_i = g.esdf_sample(xyz), g.esdf_sweep(seg, radius_m=0.2), g.esdf_slice(o, du, dv, w, h)
    store = M.store_of(g)
    want_p, want_s, want_i = M.sample(store, xyz, vs), M.sweep(store, seg, vs, radius_m=0.2), M.slice_image(store, o, du, dv, w, h, vs)
    print("points", got_p["stats"], "segments", got_s["stats"], "slice", got_i["stats"])
    M.assert_same(got_p, want_p, "points")
    M.assert_same(got_s, want_s, "segments")
    M.assert_same(got_i, want_i, "slice")
    assert want_p["stats"]["points_interpolated"] > 1000 and want_p["stats"]["points_nearest"] > 200
    assert min(want_s["stats"][k] for k in ("segments_free", "segments_collision", "segments_unknown")) > 20, want_s["stats"]
    assert want_i["stats"]["points_interpolated"] > 1000
    g.close()


def test_device_pointer_calls_on_torch_tensors_equal_the_host_calls():
    """The three _device entries on ks_stream(ctx): with stats the call has waited for the kernel and the bytes are the host
    entry's; with stats = NULL the tensors are read after torch.cuda.synchronize().  Outputs that are not asked for are not written."""
    import torch
    spec = dict(field="holes", vps=16)
    g = esdf_read_case._stored(spec)
    xyz, seg = esdf_read_case.mixed_points(3, 3001), esdf_read_case.sweep_segments(4)
    o, du, dv = esdf_read_case.oblique_plane()
    w, h = 61, 45
    want_p, want_s, want_i = g.esdf_sample(xyz), g.esdf_sweep(seg), g.esdf_slice(o, du, dv, w, h)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    ptr = lambda t: t.data_ptr()

    def sample_tensors(shape):
        return dict(distance=torch.full(shape, 7.0, dtype=torch.float32, device="cuda"), gradient=torch.full(shape + (3,), 7.0, dtype=torch.float32, device="cuda"),
                    status=torch.full(shape, 9, dtype=torch.uint8, device="cuda"), label=torch.full(shape, 9, dtype=torch.uint8, device="cuda"),
                    flags=torch.full(shape, 9, dtype=torch.uint8, device="cuda"))

    def same(t, want, keys):
        for k in keys:
            assert t[k].cpu().numpy().tobytes() == np.ascontiguousarray(want[k]).tobytes(), k

    names = ("distance", "gradient", "status", "label", "flags")
    d_xyz, d_seg = dev(xyz), dev(seg)
    # points
    t = sample_tensors((len(xyz),))
    torch.cuda.synchronize()
    assert g.esdf_sample_device(ptr(d_xyz), len(xyz), *[ptr(t[k]) for k in names]) == want_p["stats"]
    same(t, want_p, names)
    t = sample_tensors((len(xyz),))
    torch.cuda.synchronize()
    assert g.esdf_sample_device(ptr(d_xyz), len(xyz), d_distance=ptr(t["distance"]), d_status=ptr(t["status"]), stats=False) is None
    torch.cuda.synchronize()
    same(t, want_p, ("distance", "status"))
    assert (t["gradient"].cpu().numpy() == 7.0).all() and (t["label"].cpu().numpy() == 9).all() and (t["flags"].cpu().numpy() == 9).all()
    # slice
    t = sample_tensors((h, w))
    torch.cuda.synchronize()
    assert g.esdf_slice_device(o, du, dv, w, h, *[ptr(t[k]) for k in names]) == want_i["stats"]
    same(t, want_i, names)
    t = sample_tensors((h, w))
    torch.cuda.synchronize()
    assert g.esdf_slice_device(o, du, dv, w, h, d_gradient=ptr(t["gradient"]), d_label=ptr(t["label"]), stats=False) is None
    torch.cuda.synchronize()
    same(t, want_i, ("gradient", "label"))
    assert (t["distance"].cpu().numpy() == 7.0).all() and (t["status"].cpu().numpy() == 9).all()
    # segments
    snames = ("status", "t_stop", "min_clearance", "t_min")

    def sweep_tensors():
        return dict(status=torch.full((len(seg),), 9, dtype=torch.uint8, device="cuda"), **{k: torch.full((len(seg),), 7.0, dtype=torch.float32, device="cuda")
                                                                                            for k in snames[1:]})

    t = sweep_tensors()
    torch.cuda.synchronize()
    assert g.esdf_sweep_device(ptr(d_seg), len(seg), *[ptr(t[k]) for k in snames]) == want_s["stats"]
    same(t, want_s, snames)
    t = sweep_tensors()
    torch.cuda.synchronize()
    assert g.esdf_sweep_device(ptr(d_seg), len(seg), d_status=ptr(t["status"]), d_min_clearance=ptr(t["min_clearance"]), stats=False) is None
    torch.cuda.synchronize()
    same(t, want_s, ("status", "min_clearance"))
    assert (t["t_stop"].cpu().numpy() == 7.0).all() and (t["t_min"].cpu().numpy() == 7.0).all()
    g.close()


def test_adapter_sample_and_sweep_equal_model_on_the_layers_it_synced(tmp_path):
    """HipSemanticTsdfIntegrator::sampleEsdf and ::sweepEsdf after updateEsdf (adapter_demo, KS_DEMO_ESDF_SAMPLE) against the read model
    on the ESDF model of the layers the demo wrote."""
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import test_host_adapter_gpu as A
    from tests.util import NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    csv, fin, fout, fread = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin", "read.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    A._write_in(fin, A._frames())
    res = subprocess.run([A.DEMO, "fast", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True,
                         env=dict(os.environ, KS_DEMO_ESDF_SAMPLE=fread))
    assert res.returncode == 0 and "adapter_demo: sampleEsdf + sweepEsdf" in res.stdout, res.stdout + res.stderr
    idx, t, s = A._read_out(fout)
    # the demo's options (adapter_demo.cpp): min_distance_m 0.1, max_distance_m 0.4; default sweep options
    esdf = esdf_model.esdf_from_blocks(idx, t, s["label"], 16, 0.05, min_distance_m=0.1, max_distance_m=0.4)
    store = M.Store(idx, esdf.blocks(idx), 16)
    buf = open(fread, "rb").read()
    n, m = struct.unpack_from("<II", buf, 0)
    assert n == 13 ** 3 and m == n // 7 and len(buf) == 8 + n * (12 + 4 + 12 + 3) + m * (24 + 1 + 12)
    off = 8
    take = lambda dtype, count, shape: np.frombuffer(buf, dtype, count, off).reshape(shape)
    xyz = take("<f4", 3 * n, (n, 3)); off += 12 * n
    got = dict(distance=take("<f4", n, (n,)))
    off += 4 * n
    got["gradient"] = take("<f4", 3 * n, (n, 3)); off += 12 * n
    for k in ("status", "label", "flags"):
        got[k] = take(np.uint8, n, (n,)); off += n
    seg = take("<f4", 6 * m, (m, 6)); off += 24 * m
    swept = dict(status=take(np.uint8, m, (m,)))
    off += m
    for k in ("t_stop", "min_clearance", "t_min"):
        swept[k] = take("<f4", m, (m,)); off += 4 * m
    want = M.sample(store, xyz, 0.05)
    M.assert_same(got, want, "adapter sample")
    M.assert_same(swept, M.sweep(store, seg, 0.05), "adapter sweep")
    assert want["stats"]["points_interpolated"] > 100 and len(set(swept["status"])) >= 2, (want["stats"], swept["status"])
