"""GPU tier of the object instances: the cases of tests/objects_case.py on the real device (the same sizes as on the functional
model), one larger map with frames in flight, and the adapter.  The checker is tests/objects_model.py; every comparison is exact
and covers every record, every stat and the id of every voxel of every block."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import objects_case
from tests import objects_model as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(objects_case.SPECS))
def test_objects_equal_model(name):
    objects_case.run_case(objects_case.SPECS[name])


def test_larger_map_with_frames_in_flight_equals_model():
    """Four 160x120 frames at 5 cm through the frame pipeline (pipeline_frames = 12: frames are in flight when the update is called)."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    from tests.util import COMMON
    sc = synth.make_scene("room")
    frames = [synth.render_frame(sc, synth.trajectory_pose(k, radius=1.5), 160, 120, hfov_deg=90.0, seed=k) for k in range(4)]
    g = B.HipIntegrator(B.default_config(method=0, voxel_size=0.05, voxels_per_side=16, truncation_distance=0.2, max_ray_length_m=5.0,
                                         max_tiles=1 << 13, max_points=160 * 120, pipeline_frames=12, **COMMON))
    for f in frames:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    rec, stats, idx, ids, model = objects_case.check(g, {}, "larger map")
    print(stats, "tiles", len(g.tile_keys()), "labels", np.unique(rec["label"]))
    assert stats["objects"] >= 4 and len(np.unique(rec["label"])) >= 4 and stats["largest_object_voxels"] > 1000
    assert objects_case.crossing_a_seam(rec) >= 4
    c = B.object_centroids(rec, 0.05)
    assert np.allclose(c, model.centroids(0.05), rtol=0, atol=0)
    g.close()


def test_adapter_extract_objects_equals_model_on_the_layers_it_synced(tmp_path):
    """HipSemanticTsdfIntegrator::extractObjects against the model on the layers the demo wrote."""
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import test_host_adapter_gpu as A
    from tests.util import NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    csv, fin, fout, fobj = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin", "objects.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    A._write_in(fin, A._frames())
    res = subprocess.run([A.DEMO, "fast", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True,
                         env=dict(os.environ, KS_DEMO_OBJECTS=fobj))
    assert res.returncode == 0 and "adapter_demo: extractObjects" in res.stdout, res.stdout + res.stderr
    idx, t, s = A._read_out(fout)
    model = M.objects_from_blocks(idx, t, s["label"], 16, 0.05)   # the demo's options are the defaults
    buf = open(fobj, "rb").read()
    (n,) = struct.unpack_from("<I", buf, 0)
    assert n == len(model.records) >= 3 and len(buf) == 4 + n * 92
    centroids = model.centroids(np.float32(0.05)).astype(np.float32)   # (the layer's voxel size is an f32)
    for i in range(n):
        label, nv = struct.unpack_from("<II", buf, 4 + 92 * i)
        box = struct.unpack_from("<9q", buf, 4 + 92 * i + 8)
        c = np.frombuffer(buf, np.float32, 3, 4 + 92 * i + 80)
        r = model.records[i]
        assert (label, nv) == (r["label"], r["n_voxels"]), (i, label, nv, r)
        assert box == tuple(int(v) for v in r["first_voxel"]) + tuple(int(v) for v in r["bb_min"]) + tuple(int(v) for v in r["bb_max"]), (i, box, r)
        assert c.tobytes() == centroids[i].tobytes(), (i, c, centroids[i])
