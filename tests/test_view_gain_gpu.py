"""GPU tier of the view information gain: the cases of tests/view_gain_case.py on the real device (the same sizes as on the
functional model), the device-pointer entry on torch tensors, and the adapter.  The checker is tests/view_gain_model.py on the stored
ESDF as the library hands it out; every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

from tests import esdf_model, frontier_case, view_gain_case
from tests import esdf_read_model as E
from tests import view_gain_model as M

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.mark.parametrize("name", sorted(view_gain_case.SPECS))
def test_view_gain_equals_model(name):
    view_gain_case.run_case(view_gain_case.SPECS[name])


def test_device_pointer_entry_on_torch_tensors_equals_the_host_entry():
    """ks_view_gain_device on ks_stream(ctx): with stats the call has waited for the kernels and the bytes are the host entry's;
    without, it returns None and the tensor is read after torch.cuda.synchronize().  A record beyond n is not written."""
    import torch
    vox = frontier_case.random_voxels()
    g = view_gain_case._stored(vox, 16)
    w, h = 13, 5
    K = view_gain_case.K_of(w, h)
    poses = np.array(view_gain_case.path_poses(vox), F)
    cfg = dict(max_range_m=1.5, label=0)
    want, want_stats = g.view_gain(poses, K, w, h, **cfg)
    M.assert_same((want, want_stats), M.model_of(g, poses, K, width=w, height=h, **cfg), "host entry")
    n = len(poses)
    d_poses = torch.from_numpy(poses).to("cuda")
    for with_stats in (True, False):
        out = torch.full((n + 1, 8), 9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        got = g.view_gain_device(d_poses.data_ptr(), n, K, w, h, d_out=out.data_ptr(), stats=with_stats, **cfg)
        assert got == (want_stats if with_stats else None)
        torch.cuda.synchronize()
        back = out.cpu().numpy()
        assert back[:n].tobytes() == want.tobytes() and (back[n] == 9).all()
    g.close()


def test_adapter_view_gain_equals_model_on_the_layers_it_synced(tmp_path):
    """HipSemanticTsdfIntegrator::scoreViews after updateEsdf (adapter_demo, KS_DEMO_VIEW_GAIN) against the model on the ESDF model
    of the layers the demo wrote."""
    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import test_host_adapter_gpu as A
    from tests.util import NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    csv, fin, fout, fvg = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin", "view_gain.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    A._write_in(fin, A._frames())
    res = subprocess.run([A.DEMO, "fast", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True, env=dict(os.environ, KS_DEMO_VIEW_GAIN=fvg))
    assert res.returncode == 0 and "adapter_demo: scoreViews" in res.stdout, res.stdout + res.stderr
    idx, t, s = A._read_out(fout)
    # the demo's options (adapter_demo.cpp): min_distance_m 0.1, max_distance_m 0.4 for the ESDF
    esdf = esdf_model.esdf_from_blocks(idx, t, s["label"], 16, 0.05, min_distance_m=0.1, max_distance_m=0.4)
    store = E.Store(idx, esdf.blocks(idx), 16)
    buf = open(fvg, "rb").read()
    n, w, h, label = (int(v) for v in np.frombuffer(buf, "<u4", 4, 0))
    K = np.frombuffer(buf, "<f4", 4, 16)
    max_range = float(np.frombuffer(buf, "<f4", 1, 32)[0])
    stats = np.frombuffer(buf, "<u8", 11, 40)
    poses = np.frombuffer(buf, "<f4", 7 * n, 40 + 88).reshape(n, 7)
    rec = np.frombuffer(buf, M.RECORD_DTYPE, n, 40 + 88 + 28 * n)
    assert len(buf) == 40 + 88 + 28 * n + 32 * n and (n, w, h, label) == (8, 16, 12, 4)
    mrec, mstats = M.view_gain(store, poses, K, 0.05, width=w, height=h, max_range_m=max_range, label=label)
    assert rec.tobytes() == mrec.tobytes(), (rec, mrec)
    names = ("views_valid", "views_invalid") + M.COUNTERS
    assert {k: int(v) for k, v in zip(names, stats[:9])} == {k: mstats[k] for k in names} and int(stats[10]) == mstats["views_in_lds"]
    assert mstats["views_valid"] == 8 and mstats["unknown_voxels"] > 0 and mstats["surface_voxels"] > 0 and mstats["free_voxels"] > 0, mstats
