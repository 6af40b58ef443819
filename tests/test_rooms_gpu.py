"""GPU tier of the rooms: the cases of tests/rooms_case.py on the real device, at the same sizes as on the functional model.  The
checker is tests/rooms_model.py on the stored ESDF and the stored object ids as the library hands them out; every comparison is exact."""
import pytest

from tests import rooms_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(rooms_case.SPECS))
def test_rooms_equal_model(name):
    rooms_case.run_case(rooms_case.SPECS[name])


def test_adapter_rooms_equal_model_on_the_layers_it_synced(tmp_path):
    """HipSemanticTsdfIntegrator::segmentRooms after updateEsdf and extractObjects (adapter_demo, KS_DEMO_ROOMS) against the model on
    the ESDF model and the objects model of the layers the demo wrote."""
    import os
    import struct
    import subprocess

    import numpy as np

    from kimera_semantics_amd import synth
    from oracle import ref_py as R
    from tests import esdf_model, objects_model
    from tests import esdf_read_model as E
    from tests import rooms_model as M
    from tests import test_host_adapter_gpu as A
    from tests.util import NO_EARLY_OUT
    assert os.path.exists(A.DEMO), "adapter_demo not built: run __graft_entry__.build()"
    csv, fin, fout, frm = (str(tmp_path / n) for n in ("labels.csv", "in.bin", "out.bin", "rooms.bin"))
    R.write_label_csv(csv, synth.default_label_colors())
    A._write_in(fin, A._frames())
    res = subprocess.run([A.DEMO, "fast", csv, fin, fout, "1", str(NO_EARLY_OUT)], capture_output=True, text=True, env=dict(os.environ, KS_DEMO_ROOMS=frm))
    assert res.returncode == 0 and "adapter_demo: segmentRooms" in res.stdout, res.stdout + res.stderr
    idx, t, s = A._read_out(fout)
    # the demo's options (adapter_demo.cpp): min_distance_m 0.1, max_distance_m 0.4; default objects; core_distance_m 0.3, min_core_voxels 8
    esdf = esdf_model.esdf_from_blocks(idx, t, s["label"], 16, 0.05, min_distance_m=0.1, max_distance_m=0.4)
    store = E.Store(idx, esdf.blocks(idx), 16)
    objects = objects_model.objects_from_blocks(idx, t, s["label"], 16, 0.05)
    assert tuple(objects.origin) == tuple(store.org) and objects.ids.shape == store.shape
    buf = open(frm, "rb").read()
    n, nl, no, _ = struct.unpack_from("<4I", buf, 0)
    at = 16
    stats = np.frombuffer(buf, "<u8", 15, at)
    at += 120
    rec = np.frombuffer(buf, M.ROOM_DTYPE, n, at)
    at += 96 * n
    links = np.frombuffer(buf, M.LINK_DTYPE, nl, at)
    at += 32 * nl
    room_of = np.frombuffer(buf, "<u4", no, at)
    at += 4 * no
    room_m = np.frombuffer(buf, "<f4", 7 * n, at).reshape(n, 7)
    at += 28 * n
    link_m = np.frombuffer(buf, "<f4", 4 * nl, at).reshape(nl, 4)
    assert len(buf) == at + 16 * nl
    model = M.rooms(store, (len(objects.records), objects.ids), core_distance_m=0.3, min_core_voxels=8, vps=16)
    assert n >= 1 and no == len(objects.records) >= 2, (n, no, model.stats)
    assert rec.tobytes() == model.records.tobytes() and links.tobytes() == model.links.tobytes() and room_of.tobytes() == model.room_of_object.tobytes()
    assert dict(zip(M.STAT_KEYS, (int(v) for v in stats[:12]))) == model.stats
    v = np.float32(0.05)
    centroid = ((rec["sum"].astype(np.float64) / rec["n_voxels"][:, None] + 0.5) * np.float64(v)).astype(np.float32)
    centre = (rec["centre_voxel"].astype(np.float32) + np.float32(0.5)) * v
    assert room_m[:, :3].tobytes() == centroid.tobytes() and room_m[:, 3:6].tobytes() == centre.tobytes()
    assert room_m[:, 6].tobytes() == rec["clearance_bits"].view(np.float32).tobytes()
    door = (links["door_voxel"].astype(np.float32) + np.float32(0.5)) * v
    assert link_m[:, :3].tobytes() == door.tobytes() and link_m[:, 3].tobytes() == links["clearance_bits"].view(np.float32).tobytes()
