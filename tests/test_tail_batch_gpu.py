"""GPU tier: the tail of a batch of frames in one pass — one pair sort and one voxel update for the frames whose stage B went
out together (csrc/ks_hip.hip: tail_batch; ks_tail_batch_stats).  The cases are in tests/tail_batch_case.py: every one runs its
frames through the same pipelined `fast` context with the default tail and with KS_DEBUG=1 KS_TAIL_BATCH=0 (every frame's tail on
its own) and asserts equal blocks, tile keys and voxel records byte for byte, equal ks_frame_stats or error codes at every call,
through ks_tail_batch_stats that the path it means to test was taken, and both maps equal to the serial CPU oracle's bit for bit.

default_against_switch   11 trajectory frames at pipeline_frames = 12: batches of 4, 4 and a partial 3 at the flush
batches_of_eight         pipeline_frames = 16: three frame bits in the keys (8, 8 and a partial 3)
across_a_power_of_two    point counts of 4000 .. 4200 inside one batch: one width of the sequence field for all of them
long_only_when_merged    eight frames of 32 x 24 from one pose, the early-out off (every ray walks back to the sensor): voxels around
                         the sensor collect runs that are short per frame and long over the batch, the sensor's own a run
                         that is long per frame and xlong over the batch (checked below on the CPU)
color_mode_color         the gather that reads both halves of the ray descriptor
ordered_phases           early_out_phase_growth = 32, against the oracle's restatement of that schedule
error_in_a_batch         one frame carries a label outside the table: the same error code at the same call, its batch frame by frame
fallback_in_a_batch      one frame's marks do not fit KS_EXACT_CAP_MARKS: its fix point falls back, its batch goes frame by frame
slot_reuse               30 frames at pipeline_frames = 12: every slot is used twice"""
import numpy as np
import pytest

from tests import tail_batch_case as case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(case.GPU_CASES))
def test_batch_tail_equals_the_per_frame_tail(name):
    rep = case.run(case.GPU_CASES[name])
    print(name, rep)


def test_long_only_when_merged_has_such_runs():
    """The geometry of long_only_when_merged, checked on the CPU: the updates a voxel gets per frame (the oracle's weights of a
    constant-weight map without drop-off count them) stay at or below kLongRun = 32 for some voxel whose eight frames together
    exceed it (short per frame, long in the batch), and at or below kXLongRun = 1024 for some voxel whose eight frames exceed
    that (the batch's run is on the xlong list, no frame's is).  (Pure CPU; it lives here because it vouches for a GPU case.)"""
    from oracle import oracle_py as O
    spec = case.GPU_CASES["long_only_when_merged"]
    frames = case.frames_of(spec)
    cfg = case.config(spec, use_const_weight=True, use_weight_dropoff=False, max_weight=1e9, early_out_phase_growth=0)
    per_frame = []
    for T, xyz, rgba, labels in frames:
        o = O.Oracle(O.default_config(integrator_threads=1, **cfg))
        o.integrate(T, xyz, rgba, labels)
        idx = o.block_indices()
        _, t, _ = o.download(idx)
        per_frame.append({tuple(b): np.rint(t[i]["weight"]).astype(np.int64) for i, b in enumerate(idx.tolist())})
        o.close()
    blocks = set().union(*[set(p) for p in per_frame])
    short_to_long = long_to_xlong = 0
    for b in blocks:
        counts = np.stack([p.get(b, np.zeros_like(next(iter(per_frame[0].values())))) for p in per_frame])
        total, most = counts.sum(axis=0), counts.max(axis=0)
        short_to_long += int(((most <= 32) & (total > 32)).sum())
        long_to_xlong += int(((most <= 1024) & (total > 1024)).sum())
    assert short_to_long > 0 and long_to_xlong > 0, (short_to_long, long_to_xlong)
