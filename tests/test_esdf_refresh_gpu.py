"""GPU tier of the incremental ESDF refresh: the cases of tests/esdf_refresh_case.py on the real device (the same sizes as on
the functional model), one larger map refreshed while frames are in flight, the largest window, and the adapter.  The checker
is tests/esdf_model.py (for the largest window also a from-scratch ks_esdf_update on a second context); every comparison is exact
and covers every voxel of every block."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import esdf_case, esdf_model, esdf_refresh_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(esdf_refresh_case.SPECS))
def test_esdf_refresh_equals_model(name):
    esdf_refresh_case.run_case(esdf_refresh_case.SPECS[name])


def test_larger_map_refreshed_with_frames_in_flight_equals_separable_model():
    """Four 160x120 frames at 5 cm through the frame pipeline (pipeline_frames = 12), max_distance_m = 1.0: R = 20, g = 3.  The
    ESDF is made after two frames and refreshed straight after the fourth integrate, while frames are in flight."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    from tests.util import COMMON
    sc = synth.make_scene("room")
    frames = [synth.render_frame(sc, synth.trajectory_pose(k, radius=1.5), 160, 120, hfov_deg=90.0, seed=k) for k in range(4)]
    g = B.HipIntegrator(B.default_config(method=0, voxel_size=0.05, voxels_per_side=16, truncation_distance=0.2, max_ray_length_m=5.0,
                                         max_tiles=1 << 13, max_points=160 * 120, pipeline_frames=12, **COMMON))
    cfg = dict(min_distance_m=0.1, max_distance_m=1.0)
    for f in frames[:2]:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    idx1, _, first = g.esdf(**cfg)
    for f in frames[2:]:
        g.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    st = g.esdf_refresh()
    idx = g.block_indices()
    rec = g.esdf_blocks(idx)
    model = esdf_model.model_of(g, cfg)
    print("refresh", st, "first update", first)
    assert esdf_model.reach(1.0, 0.05) == 20
    esdf_model.assert_same(rec, model.blocks(idx), "larger map")
    for k in ("voxels_observed", "voxels_fixed", "voxels_clamped"):
        assert st[k] == model.stats[k], (k, st[k], model.stats[k])
    assert 0 < st["tiles_stale"] <= st["tiles_recomputed"] <= st["tiles_total"] == len(g.tile_keys()), st
    assert len(idx) >= len(idx1) and st["voxels_fixed"] > 5000
    g.close()


def test_largest_window_refresh_equals_a_fresh_update_on_a_second_context():
    """R = 255, g = 32: every tile of the map is within reach of the overwritten block, the lists are the map dilated by 32
    tiles less the positions that can hold no key.  Device against device, and both against the model (its separable form
    takes a fraction of a second for 32^3 voxels at this window)."""
    from tests import mesh_case
    vps = 8
    cfg = dict(min_distance_m=esdf_case.MIN_DISTANCE, max_distance_m=255 * esdf_case.VOXEL)
    field = esdf_case.make_field("sphere", vps)
    over = esdf_case.random_field([(0, -1, 1)], vps, 71)
    a, b = (mesh_case._integrator(0, 64, 48, vps=vps) for _ in range(2))
    for g in (a, b):
        g.upload(*field)
    a.esdf_update(**cfg)
    for g in (a, b):
        g.upload(*over)
    st = a.esdf_refresh()
    idx = a.block_indices()
    want_idx, want, fresh = b.esdf(**cfg)
    assert (idx == want_idx).all() and esdf_model.reach(cfg["max_distance_m"], esdf_case.VOXEL) == 255
    esdf_model.assert_same(a.esdf_blocks(idx), want, "R = 255")
    for k in ("voxels_observed", "voxels_fixed", "voxels_clamped"):
        assert st[k] == fresh[k], (k, st, fresh)
    for g, counts, what in ((a, st, "refreshed"), (b, fresh, "fresh")):
        model = esdf_model.model_of(g, cfg)
        esdf_model.assert_same(g.esdf_blocks(idx), model.blocks(idx), "R = 255, %s, against the model" % what)
        for k in ("voxels_observed", "voxels_fixed", "voxels_clamped"):
            assert counts[k] == model.stats[k], (what, k, counts[k], model.stats[k])
    assert st["tiles_stale"] == 1 and st["tiles_recomputed"] == st["tiles_total"] == len(idx), st
    # pass x keeps the 8 x 8 rows that hold resident tiles, pass y those dilated by 32 tiles along z — not by 32 along y too
    n_side = round(len(idx) ** (1 / 3))
    assert st["workspace_bytes"] < 2 * (n_side ** 3 + n_side ** 2 * (n_side + 64)) * 8192 + (1 << 20), st
    a.close()
    b.close()


def test_adapter_refresh_esdf_equals_model_on_the_layers_it_synced(tmp_path):
    """HipSemanticTsdfIntegrator::updateEsdf after the first frame, refreshEsdf after the last: the blocks of the update,
    overlaid with the changed blocks the refresh handed back, against the model on the layers the demo wrote."""
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import test_host_adapter_gpu as A
    from tests.util import NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    csv, fin, fout, fesdf = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin", "esdf.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    A._write_in(fin, A._frames())
    res = subprocess.run([A.DEMO, "fast", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True,
                         env=dict(os.environ, KS_DEMO_ESDF_REFRESH=fesdf))
    assert res.returncode == 0 and "adapter_demo: updateEsdf after 1 frames" in res.stdout and "adapter_demo: refreshEsdf" in res.stdout, res.stdout + res.stderr
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
    assert got_idx == sorted(tuple(int(v) for v in b) for b in idx)
    assert (np.stack(got)["flags"] == 3).sum() > 1000
