"""CPU tier: the host arithmetic that sizes the launches of the early-out's ordered phases (ks_seed_launch_shape =
seed_launch_shape of csrc/ks_hip.hip: no device involved).  A phase's launch has one wavefront per (chain, sub-run) work item;
it must cover what ANY frame that fits the slot's capacity can have in that phase, and must not fall back to the product of
the largest chain count and the largest generation count, which no frame reaches together.

Checked by enumerating EVERY n <= capacity (vectorised): the (chain, sub-run) pairs that exist in phase [g0, g1) of a frame of n
points — integration position s = chain s % chains, generation s / chains; a chain's generations inside the phase cut into
sub-runs of 16 — restated here from the schedule's definition, independently of the library's closed form.

Bound on the total, stated before measuring: the library takes per phase the maximum over all n, so the sum over the phases
is the sum of those per-phase maxima exactly (factor 1.0 asserted as <= 1.02 to leave room for a cheaper closed form); and since
different phases peak at different n, that sum may exceed the most wavefronts one frame has in total — by less than 2x for
every case below (reasoning: the early phases peak at the largest n, where chains are many; only the phases beyond generation
1024 of the default order peak at small n, and a frame of one chain has at most 2047 / 16 items there).  The product bound
the change replaces is 6x the true maximum at 307 200 points, so either assertion fails if it comes back."""
import ctypes

import numpy as np
import pytest

from kimera_semantics_amd import binding as B

SUB_RUN = 16
ORDER_STEP = 1024
MIXED, SORTED, MIXED_1024_GROUPS = 0, 1, 2


def launch_shape(order, growth, cap):
    if not __import__("os").path.exists(B.LIB_PATH):
        B.build()
    lib = ctypes.CDLL(B.LIB_PATH)   # (loads without a GPU: the call is host arithmetic)
    lib.ks_seed_launch_shape.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int32]
    n_ph = lib.ks_seed_launch_shape(order, growth, cap, None, 0)
    assert n_ph > 0, n_ph
    out = (ctypes.c_uint32 * (3 * n_ph))()
    assert lib.ks_seed_launch_shape(order, growth, cap, out, n_ph) == n_ph
    return np.array(out, dtype=np.int64).reshape(n_ph, 3)


def phase_bounds_model(n_gen, growth):
    """early_out_phase_growth in 1/16ths: a phase is (growth - 16) / 16 times as long as everything before it, one generation at least."""
    b = [0]
    while True:
        inc = max(1, b[-1] * (growth - 16) // 16)
        if b[-1] + inc >= n_gen:
            return b
        b.append(b[-1] + inc)


def existing_items(order, cap, g0, g1):
    """[n] for n = 0..cap: (chain, sub-run) pairs of phase [g0, g1) with at least one integration position below n."""
    n = np.arange(cap + 1, dtype=np.int64)
    chains = np.where((n >= ORDER_STEP) & (order == MIXED), n // ORDER_STEP, ORDER_STEP)
    full, part = n // chains, n % chains   # every chain has `full` generations, the first `part` chains one more

    def subs(gens):
        length = np.clip(np.minimum(g1, gens) - g0, 0, None)
        return (length + SUB_RUN - 1) // SUB_RUN

    return (chains - part) * subs(full) + part * subs(full + 1)


@pytest.mark.parametrize("growth", [22, 32])
@pytest.mark.parametrize("order", [MIXED, SORTED, MIXED_1024_GROUPS])
@pytest.mark.parametrize("cap", [1024, 7000, 76800, 307200, 921600])
def test_every_phase_launch_covers_every_frame_that_fits_and_no_more(cap, order, growth):
    shape = launch_shape(order, growth, cap)
    n_gen_cap = (2 * ORDER_STEP - 1) if order == MIXED else (cap + ORDER_STEP - 1) // ORDER_STEP
    bounds = phase_bounds_model(n_gen_cap, growth)
    assert shape[:, 0].tolist() == bounds and shape[:-1, 1].tolist() == bounds[1:] and shape[-1, 1] == n_gen_cap
    total = np.zeros(cap + 1, dtype=np.int64)
    need_sum = 0
    for g0, g1, launched in shape.tolist():
        items = existing_items(order, cap, g0, g1)
        need = int(items.max())
        assert launched >= need, (g0, g1, launched, need, int(items.argmax()))
        if need == 0:
            assert launched == 0, (g0, g1, launched)   # a phase no admissible frame reaches is not launched
        total += items
        need_sum += need
    launched_sum = int(shape[:, 2].sum())
    most_of_one_frame = int(total.max())
    print(f"cap {cap} order {order} growth {growth}: launched {launched_sum}, sum of per-phase maxima {need_sum}, "
          f"most of one frame {most_of_one_frame} (n = {int(total.argmax())})")
    assert launched_sum <= 1.02 * need_sum, (launched_sum, need_sum)
    assert launched_sum <= 2 * most_of_one_frame, (launched_sum, most_of_one_frame)


def test_the_headline_frame_and_its_capacity():
    """640x480, 5 cm, growth 22 (the seed of the default mode): capacity 307 200; the bench frame has 305 664 points = 298 chains of
    1026 generations.  The launches the capacity product gave (1024 chains x 2047 generations) were 147 456 wavefronts per frame."""
    shape = launch_shape(MIXED, 22, 307200)
    assert len(shape) == 25
    launched = int(shape[:, 2].sum())
    exist = sum(int(existing_items(MIXED, 307200, g0, g1)[305664]) for g0, g1, _ in shape.tolist())
    print("launched per frame", launched, "exist in the bench frame", exist, shape[:, 2].tolist())
    assert exist <= launched < 147456 // 5
    assert shape[-2:, 2].tolist() == [46, 28]   # generations [1171, 1610) and [1610, 2047): only a frame of one or two chains gets there


def test_arguments_are_checked():
    lib = ctypes.CDLL(B.LIB_PATH)
    lib.ks_seed_launch_shape.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int32]
    for order, growth, cap in ((3, 22, 1000), (0, 15, 1000), (0, 22, 0), (0, 22, 1 << 22)):
        assert lib.ks_seed_launch_shape(order, growth, cap, None, 0) == B.KS_ERR_INVALID_ARG
