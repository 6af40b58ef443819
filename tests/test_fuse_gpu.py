"""GPU tier of submap fusion (ks_fuse_map): the cases of tests/fuse_case.py on the real device (the same sizes
as on the functional model), and the adapter's scene through adapter_demo.  The yardstick is tests/fuse_model.py; every comparison
is exact."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fuse_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(fuse_case.SPECS))
def test_fuse_equals_model(name):
    fuse_case.run_case(fuse_case.SPECS[name])


def _demo_frames():
    from kimera_semantics_amd import synth
    sc = synth.make_scene("room")
    return [synth.render_frame(sc, synth.trajectory_pose(12 * k), 96, 72, seed=700 + k) for k in range(4)]


@pytest.mark.parametrize("pipeline", [0, 1])
def test_adapter_fuses_a_submap_and_the_host_layers_follow(tmp_path, pipeline):
    """HipSemanticTsdfIntegrator::fuseSubmap: the first half of the frames in a submap integrator, the rest in the main one, the
    submap fused at a generic pose.  The host layers the demo dumps — brought up to date by the integrator's own sync policy, at
    once or by the final syncLayers() — equal what two contexts driven through the C ABI hold after the same calls."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import test_host_adapter_gpu as A
    from tests.util import COMMON, NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    frames = _demo_frames()
    T = fuse_case.pose((2, -1, 1), 7.0, (0.12, -0.21, 0.07))
    csv, fin, fout = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    A._write_in(fin, frames)
    env = dict(os.environ, KS_DEMO_FUSE=" ".join(repr(float(v)) for v in T))
    res = subprocess.run([A.DEMO, "merged", csv, fin, fout, "1", str(NO_EARLY_OUT), "-1", str(pipeline)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    m = re.search(r"fuseSubmap [0-9.]+ ms, (\d+) source tiles, (\d+) of (\d+) candidate tiles touched, (\d+) allocated, (\d+) voxels fused, submap host layers (\d+) blocks", res.stdout)
    assert m, res.stdout
    # the same calls through the C ABI
    make = lambda: B.HipIntegrator(B.default_config(device_id=0, max_tiles=4096, max_points=1 << 18, method=1, max_consecutive_ray_collisions=NO_EARLY_OUT, **COMMON))
    sub, g = make(), make()
    for k, f in enumerate(frames):
        (sub if 2 * k < len(frames) else g).integrate(f.T_G_C, f.xyz, None, f.labels)
    sub_blocks = len(sub.block_indices())
    st = g.fuse(sub, T)
    got = [int(v) for v in m.groups()]
    assert got[:5] == [st["tiles_source"], st["tiles_touched"], st["tiles_candidate"], st["tiles_allocated"], st["voxels_fused"]], (got, st)
    assert st["voxels_fused"] > 1000 and st["tiles_allocated"] > 0 and got[5] == (0 if pipeline else sub_blocks)   # (on demand: the submap's layers were never asked for)
    hidx, ht, hs = A._read_out(fout)
    assert (hidx == g.block_indices()).all()
    _, gt, gs = g.download(hidx)
    assert ht.tobytes() == gt.tobytes() and hs.tobytes() == gs.tobytes()
    sub.close()
    g.close()
