"""GPU tier of the batch ESDF: the cases of tests/esdf_case.py on the real device (the same sizes as on the functional
model), one larger map with frames in flight, and the adapter.  The checker is tests/esdf_model.py; every comparison is
exact and covers every voxel of every block."""
import os
import struct
import subprocess
import time

import numpy as np
import pytest

from tests import esdf_case, esdf_model

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(esdf_case.SPECS))
def test_esdf_equals_model(name):
    esdf_case.run_case(esdf_case.SPECS[name])


def test_larger_map_with_frames_in_flight_equals_separable_model():
    """Four 160x120 frames at 5 cm through the frame pipeline (pipeline_frames = 12: frames are in flight when the update is
    called), max_distance_m = 1.0: R = 20, lines cross five tiles and more."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    from tests.util import COMMON
    sc = synth.make_scene("room")
    frames = [synth.render_frame(sc, synth.trajectory_pose(k, radius=1.5), 160, 120, hfov_deg=90.0, seed=k) for k in range(4)]
    g = B.HipIntegrator(B.default_config(method=0, voxel_size=0.05, voxels_per_side=16, truncation_distance=0.2, max_ray_length_m=5.0,
                                         max_tiles=1 << 13, max_points=160 * 120, pipeline_frames=12, **COMMON))
    for f in frames:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    cfg = dict(min_distance_m=0.1, max_distance_m=1.0)
    idx, rec, stats = g.esdf(**cfg)
    t0 = time.perf_counter()
    model = esdf_model.model_of(g, cfg)
    t_model = time.perf_counter() - t0
    print("box", stats["box_voxels"], "work space %.1f MiB" % (stats["workspace_bytes"] / 2 ** 20), "observed", stats["voxels_observed"],
          "fixed", stats["voxels_fixed"], "clamped", stats["voxels_clamped"], "model %.1f s" % t_model)
    assert esdf_model.reach(1.0, 0.05) == 20 and min(stats["box_voxels"]) > 40
    esdf_model.assert_same(rec, model.blocks(idx), "larger map")
    for k in ("voxels_observed", "voxels_fixed", "voxels_clamped"):
        assert stats[k] == model.stats[k], (k, stats[k], model.stats[k])
    assert stats["voxels_fixed"] > 5000 and len(np.unique(rec["label"][rec["flags"] == 1])) >= 4
    g.close()


def test_adapter_update_esdf_equals_model_on_the_layers_it_synced(tmp_path):
    """HipSemanticTsdfIntegrator::updateEsdf against the model on the layers the demo wrote."""
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import test_host_adapter_gpu as A
    from tests.util import NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    csv, fin, fout, fesdf = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin", "esdf.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    A._write_in(fin, A._frames())
    res = subprocess.run([A.DEMO, "fast", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True,
                         env=dict(os.environ, KS_DEMO_ESDF=fesdf))
    assert res.returncode == 0 and "adapter_demo: updateEsdf" in res.stdout, res.stdout + res.stderr
    idx, t, s = A._read_out(fout)
    # the demo's options (adapter_demo.cpp): min_distance_m 0.1, max_distance_m 0.4
    model = esdf_model.esdf_from_blocks(idx, t, s["label"], 16, 0.05, min_distance_m=0.1, max_distance_m=0.4)
    buf = open(fesdf, "rb").read()
    nb, vps = struct.unpack_from("<II", buf, 0)
    assert nb == len(idx) > 10 and vps == 16
    off, got_idx, got = 8, [], []
    for _ in range(nb):
        got_idx.append(struct.unpack_from("<3i", buf, off))
        got.append(np.frombuffer(buf, esdf_model.RECORD_DTYPE, vps ** 3, off + 12))
        off += 12 + 8 * vps ** 3
    assert off == len(buf)
    esdf_model.assert_same(np.stack(got), model.blocks(np.array(got_idx)), "adapter")
    assert sorted(got_idx) == sorted(tuple(int(v) for v in b) for b in idx)
    assert (np.stack(got)["flags"] == 3).sum() > 1000
