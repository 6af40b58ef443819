"""GPU tier of block removal: the cases of tests/remove_case.py on the real device (the same sizes as on
the functional model), and the adapter's scene through adapter_demo.  The yardsticks are tests/remove_model.py and equivalence
with a fresh context that only ever held the kept blocks; every comparison is exact."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import remove_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(remove_case.SPECS))
def test_remove_equals_model(name):
    remove_case.run_case(remove_case.SPECS[name])


def _demo_frames():
    from kimera_semantics_amd import synth
    sc = synth.make_scene("room")
    return [synth.render_frame(sc, synth.trajectory_pose(12 * k), 96, 72, seed=500 + k) for k in range(4)]


PRUNE_RADIUS = 2.21   # metres around the sensor


@pytest.mark.parametrize("drop_semantic", [True, False])
def test_adapter_prunes_device_map_and_host_layers_alike(tmp_path, drop_semantic):
    """HipSemanticTsdfIntegrator with a pruning radius, as integration/server.patch sets it: after every integratePointCloud the
    far blocks leave the device map and the host TSDF layer.  The host layers the demo dumps equal what a context driven through
    the C ABI holds after the same calls — with the semantic layer kept (the reference's behaviour) the surviving semantic halves go
    back up, with it dropped the map really shrinks."""
    from kimera_semantics_amd import binding as B
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import remove_model as M
    from tests import test_host_adapter_gpu as A
    from tests.util import COMMON, NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    frames = _demo_frames()
    csv, fin, fout = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    A._write_in(fin, frames)
    env = dict(os.environ, KS_DEMO_PRUNE=repr(PRUNE_RADIUS), KS_DEMO_PRUNE_DROP_SEMANTIC="1" if drop_semantic else "0")
    res = subprocess.run([A.DEMO, "merged", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = re.findall(r"pruned after frame (\d+): (\d+) blocks removed, (\d+) tiles resident of a pool of (\d+), host layers (\d+) tsdf / (\d+) semantic", res.stdout)
    assert len(lines) == len(frames), res.stdout
    # the same calls through the C ABI
    g = B.HipIntegrator(B.default_config(device_id=0, max_tiles=4096, max_points=1 << 18, method=1, max_consecutive_ray_collisions=NO_EARLY_OUT, **COMMON))
    seen = set()
    for k, f in enumerate(frames):
        g.integrate(f.T_G_C, f.xyz, None, f.labels)
        idx, t, s = g.download()
        seen |= {tuple(r) for r in idx.tolist()}
        centre = [float(v) for v in f.T_G_C[4:7]]
        gap = np.abs(M.distance_f64(idx, centre, 0.05, 16) - float(np.float32(PRUNE_RADIUS))).min()
        assert gap > 1e-3, gap                       # (no block near the threshold: the scene is chosen for it)
        st = g.remove_distant(centre, PRUNE_RADIUS)
        removed = g.removed_blocks()
        assert (removed == M.removed_of_distance(idx, centre, PRUNE_RADIUS, 0.05, 16)).all()
        if not drop_semantic and len(removed):
            rows = {tuple(r): j for j, r in enumerate(idx.tolist())}
            g.upload(removed, None, s[[rows[tuple(r)] for r in removed.tolist()]])
            g.updated_block_indices(reset=True)
        n_removed, resident, pool, host_tsdf, host_sem = (int(v) for v in lines[k][1:])
        assert n_removed == st["blocks_removed"] and resident == st["tiles_resident"] and pool == st["pool_capacity_tiles"], (lines[k], st)
        if drop_semantic:
            assert host_tsdf == host_sem == len(idx) - len(removed), (lines[k], len(idx), len(removed))
        else:   # (the device holds every block ever seen again; the host TSDF layer only what was written since it was pruned)
            assert host_sem == len(seen) == len(g.block_indices()) and host_tsdf <= len(idx) - len(removed), (lines[k], len(seen))
    assert sum(int(l[1]) for l in lines) > 0, lines
    hidx, ht, hs = A._read_out(fout)
    _, gt, gs = g.download(hidx)
    assert len(hidx) == int(lines[-1][4])
    assert ht.tobytes() == gt.tobytes() and hs.tobytes() == gs.tobytes()
    if drop_semantic:
        assert (hidx == g.block_indices()).all()
    g.close()
