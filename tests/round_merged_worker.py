"""One process of tests/test_round_exact_merged_{cpu,gpu}.py: the EXACT frame-sharded rounds of `merged`
(ks_integrate_round_exact with method = 1) through the communicator library named by KS_RCCL_LIB (the test double
tests/mock_rccl), or all frames in order on one plain `merged` context.

    round_merged_worker.py seq OUT N_FRAMES
    round_merged_worker.py RANK WORLD UID_HEX OUT round:N_ROUNDS
    round_merged_worker.py RANK WORLD UID_HEX OUT fail        rank 1 passes a label 21 in round 0: nobody may hang

KS_ROUND_WH=WxH and KS_ROUND_VOXEL=<metres> choose the frame size (tests/reduce_worker.round_frames) and the voxel size."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.reduce_worker import export_all, round_frames   # noqa: E402


def merged_config_kw(color_mode=1, bundle_order=0):
    from kimera_semantics_amd import synth
    kw = dict(semantic_measurement_probability=0.8, dynamic_labels=[20], label_rgba=synth.default_label_colors(), method=1,
              voxels_per_side=8, color_mode=color_mode, bundle_order=bundle_order)
    if os.environ.get("KS_ROUND_VOXEL"):
        vs = float(os.environ["KS_ROUND_VOXEL"])
        kw.update(voxel_size=vs, truncation_distance=4 * vs)
    return kw


def bundle_census(f, voxel_size, min_ray=0.1, max_ray=5.0):
    """(bundles, mixed-label bundles) of a frame, counted with numpy alone: the points whose ray is min_ray .. max_ray long,
    grouped by the voxel floor(point_G / voxel_size) they end in; a bundle is mixed if its points carry more than one label.
    Every bundle's ray starts in the sensor's voxel, so that voxel's run of updates is `bundles` long."""
    from kimera_semantics_amd import synth
    p = f.xyz.astype(np.float64)
    r = np.linalg.norm(p, axis=1)
    keep = (r >= min_ray) & (r <= max_ray)
    g = p[keep] @ synth.quat_to_R(f.T_G_C).astype(np.float64).T + f.T_G_C[4:7].astype(np.float64)
    vox = np.floor(g / voxel_size).astype(np.int64)
    _, inv = np.unique(vox, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    pairs = np.unique(np.stack([inv, f.labels[keep].astype(np.int64)], axis=1), axis=0)
    labels_per_bundle = np.bincount(pairs[:, 0], minlength=inv.max() + 1)
    return int(inv.max() + 1), int((labels_per_bundle > 1).sum())


def make(**kw):
    from kimera_semantics_amd import binding as B
    w, h = (int(x) for x in os.environ.get("KS_ROUND_WH", "160x120").split("x"))
    return B.HipIntegrator(B.default_config(max_tiles=4096, max_points=max(1 << 15, w * h), **merged_config_kw(**kw)))


def main_seq(out, n_frames):
    h = make()
    for f in round_frames(n_frames):
        h.integrate(f.T_G_C, f.xyz, f.rgba, f.labels)
    keys, rec = export_all(h)
    np.savez(os.path.join(out, "round_seq.npz"), keys=keys, rec=rec[:, :, :25])
    h.close()
    print("sequential ok", len(keys), "tiles")


def main_round(rank, world, comm, out, n_rounds):
    frames = round_frames(world * n_rounds)
    marcher, owner = make(), make()
    stats = []
    for r in range(n_rounds):
        f = frames[r * world + rank]
        stats.append(owner.integrate_round_exact(marcher, comm, rank, world, r * world, f.T_G_C, f.xyz, f.rgba, f.labels))
    keys, rec = export_all(owner)
    np.savez(os.path.join(out, f"round_rank{rank}.npz"), keys=keys, rec=rec[:, :, :25],
             marched=np.array([s["updates_marched"] for s in stats]), applied=np.array([s["updates_applied"] for s in stats]),
             sent=np.array([s["bytes_sent"] for s in stats]), origin=np.array([int(s["origin_voxel_touched"]) for s in stats]))
    marcher.close()
    owner.close()
    print("round worker", rank, "ok", stats)


def main_fail(rank, world, comm, out):
    """Round 0 with a label 21 on rank 1.  Every rank must come back with an error; what it was goes to fail_rank<r>.json."""
    from kimera_semantics_amd import binding as B
    f = round_frames(world)[rank]
    labels = f.labels.copy()
    if rank == 1:
        labels[len(labels) // 2] = 21
    marcher, owner = make(), make()
    res = dict(rank=rank, code=0, text="")
    try:
        owner.integrate_round_exact(marcher, comm, rank, world, 0, f.T_G_C, f.xyz, f.rgba, labels)
    except B.KsError as e:
        res.update(code=int(e.code), text=str(e))
    res["tiles_after"] = int(len(owner.tile_keys()))
    with open(os.path.join(out, f"fail_rank{rank}.json"), "w") as fh:
        json.dump(res, fh)
    marcher.close()
    owner.close()
    print("fail worker", rank, res)
    sys.exit(3 if res["code"] else 0)   # non-zero: the call failed, as it must


def main():
    if sys.argv[1] == "seq":
        return main_seq(sys.argv[2], int(sys.argv[3]))
    rank, world, uid_hex, out, what = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    lib = C.CDLL(os.environ["KS_RCCL_LIB"])

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_byte * 128)]
    uid = UniqueId()
    C.memmove(C.byref(uid), bytes.fromhex(uid_hex), 128)
    comm = C.c_void_p()
    lib.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    assert lib.ncclCommInitRank(C.byref(comm), world, uid, rank) == 0
    if what == "fail":
        return main_fail(rank, world, comm.value, out)
    return main_round(rank, world, comm.value, out, int(what.split(":")[1]))


if __name__ == "__main__":
    main()
