"""GPU tier of the exploration frontiers: the cases of tests/frontier_case.py on the real device (the same sizes as on the
functional model) and the adapter.  The checker is tests/frontier_model.py on the stored ESDF and the stored navigation field as the
library hands them out; every comparison is exact."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import esdf_model, frontier_case
from tests import esdf_read_model as E
from tests import frontier_model as M
from tests import nav_model as N

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(frontier_case.SPECS))
def test_frontiers_equal_model(name):
    frontier_case.run_case(frontier_case.SPECS[name])


def test_adapter_frontiers_equal_model_on_the_layers_it_synced(tmp_path):
    """HipSemanticTsdfIntegrator::extractFrontiers after updateEsdf and updateNavField (adapter_demo, KS_DEMO_FRONTIERS) against the
    model on the ESDF model of the layers the demo wrote."""
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import test_host_adapter_gpu as A
    from tests.util import NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    csv, fin, fout, ffr = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin", "frontiers.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    A._write_in(fin, A._frames())
    res = subprocess.run([A.DEMO, "fast", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True, env=dict(os.environ, KS_DEMO_FRONTIERS=ffr))
    assert res.returncode == 0 and "adapter_demo: extractFrontiers" in res.stdout, res.stdout + res.stderr
    idx, t, s = A._read_out(fout)
    # the demo's options (adapter_demo.cpp): min_distance_m 0.1, max_distance_m 0.4; radius 0.2 for the field and the frontiers
    esdf = esdf_model.esdf_from_blocks(idx, t, s["label"], 16, 0.05, min_distance_m=0.1, max_distance_m=0.4)
    store = E.Store(idx, esdf.blocks(idx), 16)
    buf = open(ffr, "rb").read()
    n, = struct.unpack_from("<I", buf, 0)
    goal = np.frombuffer(buf, "<f4", 3, 4).reshape(1, 3)
    stats = np.frombuffer(buf, "<u8", 9, 16)
    rec = np.frombuffer(buf, M.RECORD_DTYPE, n, 16 + 72)
    metric = np.frombuffer(buf, "<f4", 6 * n, 16 + 72 + 88 * n).reshape(n, 6)
    assert len(buf) == 16 + 72 + 88 * n + 24 * n
    model = M.frontiers(store, N.field(store, goal, 0.05, radius_m=0.2), radius_m=0.2, vps=16)
    assert rec.tobytes() == model.records.tobytes() and n >= 2, (n, model.stats)
    assert dict(zip(M.STAT_KEYS, (int(v) for v in stats[:8]))) == model.stats
    centroid = ((rec["sum"].astype(np.float64) / rec["n_voxels"][:, None] + 0.5) * np.float64(np.float32(0.05))).astype(np.float32)
    target = (rec["nav_voxel"].astype(np.float32) + np.float32(0.5)) * np.float32(0.05)
    assert metric[:, :3].tobytes() == centroid.tobytes() and metric[:, 3:].tobytes() == target.tobytes()
