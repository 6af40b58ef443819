"""GPU tier of the semantic mesh: the cases of tests/mesh_case.py on the real device (the same sizes as on the functional
model), and one full-size map.  The checker is tests/mesh_model.py; every comparison is exact, nothing is left out."""
import time

import numpy as np
import pytest

from tests import mesh_case, mesh_model

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(mesh_case.SPECS))
def test_mesh_equals_model(name):
    mesh_case.run_case(mesh_case.SPECS[name])


def test_full_size_pipelined_incremental_mesh_equals_model():
    """8 frames of 640x480 at 5 cm (the C2 shape of tests/run_configs.py), frames in flight (pipeline_frames = 12), an
    only_stale refresh after every second frame: the stored mesh is the model's of the final map, and the same context's
    from-scratch extraction."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    from tests.util import COMMON
    sc = synth.make_scene("room")
    frames = [synth.render_frame(sc, synth.trajectory_pose(k, radius=1.5), 640, 480, hfov_deg=90.0, seed=k) for k in range(8)]
    g = B.HipIntegrator(B.default_config(method=0, voxel_size=0.05, voxels_per_side=16, truncation_distance=0.2, max_ray_length_m=5.0,
                                         max_tiles=1 << 13, max_points=640 * 480, pipeline_frames=12, **COMMON))
    meshed = []
    for k, f in enumerate(frames):
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
        if k % 2 == 1:
            m = g.mesh(only_stale=True)
            meshed.append((m.stats["blocks_meshed"], m.stats["blocks_total"]))
    t0 = time.perf_counter()
    model = mesh_model.model_of(g)
    t_model = time.perf_counter() - t0
    print("refreshes (blocks meshed, blocks in the map):", meshed, "triangles", m.n_triangles, "model %.1f s" % t_model)
    # (not trivial: one 90-degree view from the middle of the room sees well over 6 m^2 of wall and floor; a surface crossing
    # 5 cm cubes leaves about two triangles per 25 cm^2, i.e. 800 per m^2)
    assert m.n_triangles > 5000, m.n_triangles
    assert len(np.unique(m.labels)) >= 3
    mesh_model.assert_same(m, model, "stored mesh after the last refresh")
    full = g.mesh(only_stale=False)
    assert full.stats["blocks_meshed"] == full.stats["blocks_total"]
    mesh_model.assert_same(full, model, "from-scratch extraction of the same context")
    idle = g.mesh(only_stale=True)
    assert idle.stats["blocks_meshed"] == 0
    mesh_model.assert_same(idle, model, "idle refresh")
    g.close()


def test_adapter_update_mesh_equals_model_on_the_layers_it_synced(tmp_path):
    """HipSemanticTsdfIntegrator::updateMesh (no layer sync behind it) against the model on the layers the demo wrote."""
    import os
    import struct
    import subprocess
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import test_host_adapter_gpu as A
    from tests.util import NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    csv, fin, fout, fmesh = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin", "mesh.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    A._write_in(fin, A._frames())
    res = subprocess.run([A.DEMO, "fast", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True,
                         env=dict(os.environ, KS_DEMO_MESH=fmesh))
    assert res.returncode == 0 and "adapter_demo: updateMesh" in res.stdout, res.stdout + res.stderr
    idx, t, s = A._read_out(fout)
    model = mesh_model.mesh_from_blocks(idx, t, 16, 0.05, labels=s["label"])
    buf = open(fmesh, "rb").read()
    (nb,), off = struct.unpack_from("<I", buf, 0), 4
    assert nb == len(idx)          # a full extraction hands back every block, the empty ones too
    got = {}
    for _ in range(nb):
        b = struct.unpack_from("<3i", buf, off)
        (n,) = struct.unpack_from("<I", buf, off + 12)
        got[b] = buf[off + 16: off + 16 + n * 29]
        off += 16 + n * 29
    assert off == len(buf)
    want = {}
    for blk in model["blocks"]:
        a, n = int(blk["first_vertex"]), int(blk["n_vertices"])
        want[tuple(int(v) for v in blk["block"])] = b"".join(np.ascontiguousarray(model[k][a:a + n]).tobytes() for k in ("xyz", "normals", "rgba", "labels"))
    assert len(want) > 10 and {k: v for k, v in got.items() if v} == want
