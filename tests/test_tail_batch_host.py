"""Host logic of the batch tail: the binding exposes ks_tail_batch_stats, and the selection rule — whether a batch's tail runs as
one pass — is a pure function of what the frames' snapshots say (ks_tail_batch_rule: host arithmetic, no device)."""
import ctypes as C
import os

import pytest

from kimera_semantics_amd import binding as B

RUNS_MIN = 1 << 20   # ks_ctx::apply_runs_min_pairs by default


def library():
    if not os.path.exists(B.LIB_PATH):
        B.build()
    lib = C.CDLL(B.LIB_PATH)   # (loads without a GPU: the call is host arithmetic)
    lib.ks_tail_batch_rule.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_int32, C.c_int32, C.c_int32, C.c_uint64]
    return lib


def rule(err, n_pairs, marcher=0, profiling=0, runs_min=RUNS_MIN):
    nb = len(err)
    e = (C.c_uint32 * max(nb, 1))(*err)
    n = (C.c_uint64 * max(nb, 1))(*n_pairs)
    return library().ks_tail_batch_rule(e, n, nb, marcher, profiling, runs_min)


def test_binding_exposes_the_entries():
    assert "ks_tail_batch_stats" in B.ABI_SYMBOLS and "ks_tail_batch_rule" in B.ABI_SYMBOLS
    assert hasattr(B.HipIntegrator, "tail_batch_stats")


TABLE = [
    # err per frame, pairs per frame, marcher, profiling -> one pass?
    ((0, 0, 0, 0), (500000, 510000, 490000, 505000), 0, 0, 1),   # the headline batch
    ((0, 0, 0), (1000, 2000, 3000), 0, 0, 1),                    # a partial batch
    ((0, 0, 0, 0, 0, 0, 0, 0), (9,) * 8, 0, 0, 1),               # eight frames
    ((0, 0, 0, 0), (500, 0, 500, 500), 0, 0, 1),                 # a frame without updates in the middle
    ((0, 0, 0, 0), (500, 500, 500, 500), 0, 2, 1),               # level-2 profile: every 4th k_apply timed — batches stay
    ((0,), (500000,), 0, 0, 0),                                  # nb = 1: nothing to share
    ((0, 0, 0, 0), (0, 0, 0, 0), 0, 0, 0),                       # nothing to apply
    ((0, 1, 0, 0), (500, 500, 500, 500), 0, 0, 0),               # error bits: label range ...
    ((0, 0, 0, 2), (500, 500, 500, 500), 0, 0, 0),
    ((4, 0, 0, 0), (500, 500, 500, 500), 0, 0, 0),
    ((0, 0, 8, 0), (500, 500, 500, 500), 0, 0, 0),               # ... pair-buffer overflow (repair_after_overflow)
    ((0, 0, 64, 0), (500, 500, 500, 500), 0, 0, 0),              # ... a fix point that fell back (repair_after_fallback)
    ((0, 0, 0, 0), (500, RUNS_MIN, 500, 500), 0, 0, 0),          # a frame AT apply_runs_min_pairs keeps k_apply_runs
    ((0, 0, 0, 0), (500, RUNS_MIN - 1, 500, 500), 0, 0, 1),      # ... one below it does not
    ((0, 0, 0, 0), (500, 500, 500, 500), 1, 0, 0),               # a marcher exports its updates
    ((0, 0, 0, 0), (500, 500, 500, 500), 0, 1, 0),               # the stage profile launches batches of one
]


@pytest.mark.parametrize("row", TABLE)
def test_selection_rule(row):
    err, pairs, marcher, profiling, want = row
    assert rule(err, pairs, marcher, profiling) == want, row


def test_selection_rule_refuses_bad_arguments():
    assert rule((0,) * 9, (1,) * 9) < 0                          # more frames than a batch holds
    assert library().ks_tail_batch_rule(None, None, 2, 0, 0, RUNS_MIN) < 0
    # KS_APPLY_RUNS=1 (tests): k_apply_runs for every frame — no batch is ever taken
    assert rule((0, 0), (500, 500), runs_min=0) == 0
