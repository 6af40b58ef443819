"""GPU tier of the indexed mesh: the cases of tests/mesh_index_case.py on the real device (the same sizes as on the
functional model), one full-size map, and the host adapter.  The checker is tests/mesh_index_model.py; every comparison is
exact, nothing is left out."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mesh_index_case, mesh_index_model

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(mesh_index_case.SPECS))
def test_mesh_index_equals_model(name):
    mesh_index_case.run_case(mesh_index_case.SPECS[name])


def test_full_size_pipelined_map():
    """8 frames of 640x480 at 5 cm (the map of tests/test_mesh_gpu.py), frames in flight (pipeline_frames = 12): the index against
    the model applied to the context's own ks_mesh_download (tests/test_mesh_gpu.py ties that to the mesh model).  Dozens
    of scan slices and sort tiles, hundreds of workgroups per kernel, object ids from a stored object set."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    from tests.util import COMMON
    sc = synth.make_scene("room")
    frames = [synth.render_frame(sc, synth.trajectory_pose(k, radius=1.5), 640, 480, hfov_deg=90.0, seed=k) for k in range(8)]
    g = B.HipIntegrator(B.default_config(method=0, voxel_size=0.05, voxels_per_side=16, truncation_distance=0.2, max_ray_length_m=5.0,
                                         max_tiles=1 << 13, max_points=640 * 480, pipeline_frames=12, **COMMON))
    for f in frames:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    mesh = g.mesh()
    g.objects()
    im = mesh_index_case.check(g, mesh, "full size", expect_ids=g.object_query)
    print("full size:", im.stats)
    assert im.n_triangles > 5000 and im.stats["vertices"] < im.stats["corners"] / 3 and len(np.unique(im.labels)) >= 3
    assert len(set(np.unique(im.object_ids).tolist()) - {mesh_index_case.NONE}) >= 2
    g.close()


def test_adapter_index_mesh_equals_model_on_the_layers_it_synced(tmp_path):
    """HipSemanticTsdfIntegrator::indexMesh (no layer sync behind it) against the models on the layers the demo wrote."""
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import mesh_model
    from tests import test_host_adapter_gpu as A
    from tests.util import NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    csv, fin, fout, fmesh = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin", "indexed.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    A._write_in(fin, A._frames())
    res = subprocess.run([A.DEMO, "fast", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True,
                         env=dict(os.environ, KS_DEMO_MESH_INDEXED=fmesh))
    assert res.returncode == 0 and "adapter_demo: indexMesh" in res.stdout, res.stdout + res.stderr
    idx, t, s = A._read_out(fout)
    model = mesh_index_model.index_of(mesh_model.mesh_from_blocks(idx, t, 16, 0.05, labels=s["label"]))
    buf = open(fmesh, "rb").read()
    nv, nc = struct.unpack_from("<2I", buf, 0)
    assert (nv, nc) == (model["stats"]["vertices"], model["stats"]["corners"]) and nv > 1000
    off = 8
    for name, width in (("xyz", 12), ("normals", 12), ("rgba", 4), ("labels", 1)):
        assert buf[off:off + nv * width] == np.ascontiguousarray(model[name]).tobytes(), name
        off += nv * width
    assert buf[off:off + 4 * nv] == b"\xff" * (4 * nv)          # no objects were made: every id is KS_OBJECT_NONE
    off += 4 * nv
    assert buf[off:] == model["indices"].tobytes()
