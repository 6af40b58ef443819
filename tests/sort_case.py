"""The cases of the radix sort (csrc/ks_radix_sort.h) through its two diagnostic entries, shared by both tiers: the GPU tier
(tests/test_sort_gpu.py) calls run_case in-process, the CPU tier (tests/test_sort_cpu.py) runs the specs that fit the host functional
model of the device code as child processes:
    KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.sort_case '<json spec>'
The yardstick of a sort of the bits [b, e) is NumPy's stable argsort of those bits alone (`expected`): whole keys come back, the bits
outside the range carried along unchanged, and the values (0, 1, 2, ...: the input positions) show the stability.  A sort has no
tolerance: every comparison is exact.

What the keys are drawn for (`make_keys`): inside the range most keys come from a pool of 37 values, so equal keys are the rule and
their order matters; below b and above e every bit is random, so a sort that looks at a bit outside its range, or drops one, shows."""
import json
import os
import sys
import time

import numpy as np

SIZES = [1, 63, 2048, 2049, 3 * 2048 + 5]     # one key, less than a wave's round, exactly a tile, a tile and a key, three tiles and a rest
FILL = 0xA5                                   # ks_debug_radix_sort_batch fills the second buffer set with this byte


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
def clamp(key_bits, b, e):
    return b, max(b, min(e, key_bits))


def field_of(keys, b, e):
    """The bits [b, e) of the keys, as u64 (e already clamped to the key width)."""
    return (keys.astype(np.uint64) >> np.uint64(b)) & np.uint64((1 << (e - b)) - 1)


def expected(keys, vals, b, e):
    b, e = clamp(keys.dtype.itemsize * 8, b, e)
    order = np.argsort(field_of(keys, b, e), kind="stable")
    return keys[order], None if vals is None else vals[order]


def make_keys(rng, n, key_bits, b, e, equal=False):
    b, e = clamp(key_bits, b, e)
    w = e - b
    keys = rng.integers(0, (1 << 64) - 1, size=n, dtype=np.uint64, endpoint=True)
    if w:
        pool = rng.integers(0, (1 << w) - 1, size=37, dtype=np.uint64, endpoint=True)
        field = pool[rng.integers(0, len(pool), size=n)]
        if equal:
            field[:] = pool[0]
        else:
            field[::5] = rng.integers(0, (1 << w) - 1, size=len(field[::5]), dtype=np.uint64, endpoint=True)   # ... and a fifth from the whole range
        keys = (keys & ~np.uint64(((1 << w) - 1) << b)) | (field << np.uint64(b))
    return keys.astype(np.uint32 if key_bits == 32 else np.uint64)


def _context():
    from kimera_semantics_amd import binding as B
    from tests.util import COMMON
    return B.HipIntegrator(B.default_config(max_tiles=64, max_points=1024, **dict(COMMON, method=0)))


def sort_and_check(g, keys, pairs, b, e, what):
    vals = np.arange(len(keys), dtype=np.uint32) if pairs else None
    k, v = g.debug_radix_sort_range(keys, vals, b, e)
    ek, ev = expected(keys, vals, b, e)
    if not np.array_equal(k, ek):
        i = int(np.argmax(k != ek))
        raise AssertionError("%s: keys differ at %d of %d entries, first at %d: %#x, expected %#x" % (what, int((k != ek).sum()), len(k), i, int(k[i]), int(ek[i])))
    if pairs and not np.array_equal(v, ev):
        i = int(np.argmax(v != ev))
        raise AssertionError("%s: keys right, values differ at %d entries (not stable?), first at %d: %d, expected %d" % (what, int((v != ev).sum()), i, int(v[i]), int(ev[i])))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def case_range(spec):
    """Bits [b, e) of u32 / u64 keys, keys only and with values, at every size of the spec, on one context."""
    g = _context()
    rng = np.random.default_rng(spec.get("seed", 1))
    kb, b, e = spec["key_bits"], spec["b"], spec["e"]
    modes = spec.get("modes", [False, True])
    for n in spec.get("sizes", SIZES):
        keys = make_keys(rng, n, kb, b, e, equal=spec.get("equal", False))
        lo, hi = clamp(kb, b, e)
        k64 = keys.astype(np.uint64)
        if n > 100 and hi > lo:   # what the keys are drawn for
            assert len(np.unique(field_of(keys, lo, hi))) < n, "no equal keys"
            assert lo == 0 or len(np.unique(k64 & np.uint64((1 << lo) - 1))) > 1, "no bits below the range"
            assert hi == kb or len(np.unique(k64 >> np.uint64(hi))) > 1, "no bits above the range"
        for pairs in modes:
            what = "u%d bits [%d, %d), n = %d, %s" % (kb, b, e, n, "with values" if pairs else "keys only")
            if spec.get("equal") or hi == lo:
                ek, _ = expected(keys, None, b, e)
                assert np.array_equal(ek, keys), what            # (the yardstick: nothing to order, the input comes back)
            sort_and_check(g, keys, pairs, b, e, what)
    g.close()
    return {"sorts": len(spec.get("sizes", SIZES)) * len(modes)}


# (n, key width, with values, b, e): the sizes go up and down across tile counts and tile shapes, the kinds alternate.  The last step
# needs more workspace than a quarter above anything before it: the workspace is allocated anew.
SEQUENCE = [(300000, 64, True, 19, 40), (5, 32, False, 0, 21), (2049, 64, False, 44, 64), (70000, 32, True, 3, 32), (1, 64, True, 0, 64),
            (300001, 32, False, 0, 21), (4096, 64, True, 56, 64), (123457, 64, False, 19, 56), (2048, 32, True, 13, 13), (6149, 64, True, 24, 45),
            (65, 64, False, 3, 4), (700000, 64, True, 0, 64)]
SEQUENCE_SMALL = [(6149, 64, True, 19, 40), (5, 32, False, 0, 21), (2049, 64, False, 44, 64), (4100, 32, True, 3, 32), (1, 64, True, 0, 64),
                  (6150, 32, False, 0, 21), (4096, 64, True, 56, 64), (2047, 64, False, 19, 56), (2048, 32, True, 13, 13), (63, 64, True, 24, 45),
                  (65, 64, False, 3, 4), (9000, 64, True, 0, 64)]


def workspace_words(n, b, e):
    """What ksrs::sort_rb asks of one half of the workspace for a sort of n <= 2^20 keys: head + passes x tiles x 256 status words."""
    return 8 * 2048 + 8 + ((e - b + 7) // 8) * ((n + 2047) // 2048) * 256


def case_sequence(spec):
    """One context, a dozen sorts one after another, twice: every sort runs in the workspace half the sort before it left to be cleared."""
    g = _context()
    steps = SEQUENCE_SMALL if spec.get("small") else SEQUENCE
    rng = np.random.default_rng(7)
    inputs = [make_keys(rng, n, kb, b, e) for (n, kb, _, b, e) in steps]
    for rnd in range(2):
        for i, ((n, kb, pairs, b, e), keys) in enumerate(zip(steps, inputs)):
            sort_and_check(g, keys, pairs, b, e, "round %d, sort %d: u%d bits [%d, %d), n = %d, %s" % (rnd, i, kb, b, e, n, "with values" if pairs else "keys only"))
    g.close()
    return {"sorts": 2 * len(steps)}


def check_batch(g, keys, vals, counts, b, e, what):
    nb, cap = keys.shape
    k, v = g.debug_radix_sort_batch(keys, vals, counts, b, e)
    in_b = ((e - b + 7) // 8) % 2 == 1
    for y in range(nb):
        c = min(int(counts[y]), cap)
        ek, ev = expected(keys[y, :c], vals[y, :c], b, e)
        w = "%s, sort %d of %d, count %d of cap %d" % (what, y, nb, int(counts[y]), cap)
        assert np.array_equal(k[y, :c], ek), w + ": keys"
        assert np.array_equal(v[y, :c], ev), w + ": values"
        # nothing is scattered beyond the count: the second buffer set still holds its fill there, the first the input
        rest_k = np.full(cap - c, int.from_bytes(bytes([FILL] * 8), "little"), np.uint64) if in_b else keys[y, c:]
        rest_v = np.full(cap - c, int.from_bytes(bytes([FILL] * 4), "little"), np.uint32) if in_b else vals[y, c:]
        assert np.array_equal(k[y, c:], rest_k), w + ": keys written beyond the count"
        assert np.array_equal(v[y, c:], rest_v), w + ": values written beyond the count"


def case_batch(spec):
    """ksrs::sort_dev_batch: counts in device memory, up to 8 sorts per launch, both parities of the pass count."""
    g = _context()
    cap, counts = spec["cap"], np.array(spec["counts"], np.uint64)
    nb = len(counts)
    rng = np.random.default_rng(11)
    for (b, e) in spec.get("ranges", [(44, 64), (48, 64)]):     # three passes: the result is in b; two: in a
        keys = make_keys(rng, nb * cap, 64, b, e).reshape(nb, cap)
        vals = np.arange(nb * cap, dtype=np.uint32).reshape(nb, cap)
        for rnd in range(2):
            check_batch(g, keys, vals, counts, b, e, "bits [%d, %d), call %d" % (b, e, rnd))
    g.close()
    return {"sorts": 2 * 2 * nb}


def case_errors(spec):
    """What the two entries refuse, and that the context sorts correctly afterwards."""
    from kimera_semantics_amd import binding as B
    L = B.lib()
    g = _context()
    rng = np.random.default_rng(13)
    keys = make_keys(rng, 2049, 64, 19, 40)
    vals = np.arange(len(keys), dtype=np.uint32)
    sort_and_check(g, keys, True, 19, 40, "before")
    k, v = keys.copy(), vals.copy()
    p = lambda a: a.ctypes.data
    for bad_bits in (0, 16, 31, 33, 63, 65, 128, -32):
        assert L.ks_debug_radix_sort_range(g._h, p(k), p(v), len(k), bad_bits, 19, 40) == B.KS_ERR_INVALID_ARG, bad_bits
    assert L.ks_debug_radix_sort_range(g._h, None, p(v), len(k), 64, 19, 40) == B.KS_ERR_INVALID_ARG
    assert L.ks_debug_radix_sort_range(None, p(k), p(v), len(k), 64, 19, 40) == B.KS_ERR_INVALID_ARG
    assert L.ks_debug_radix_sort_range(g._h, None, None, 0, 64, 19, 40) == 0                  # (nothing to sort: no array needed)
    cap = 2049
    counts = np.full(9, cap, np.uint64)
    bk, bv = np.tile(keys, 9), np.tile(vals, 9)
    for nb in (0, 9, -1):
        assert L.ks_debug_radix_sort_batch(g._h, p(bk), p(bv), p(counts), nb, cap, 44, 64) == B.KS_ERR_INVALID_ARG, nb
    for args in ((None, p(bv), p(counts)), (p(bk), None, p(counts)), (p(bk), p(bv), None)):
        assert L.ks_debug_radix_sort_batch(g._h, *args, 2, cap, 44, 64) == B.KS_ERR_INVALID_ARG
    assert L.ks_debug_radix_sort_batch(None, p(bk), p(bv), p(counts), 2, cap, 44, 64) == B.KS_ERR_INVALID_ARG
    assert L.ks_debug_radix_sort_batch(g._h, p(bk), p(bv), p(counts), 2, 0, 44, 64) == B.KS_ERR_INVALID_ARG
    assert L.ks_debug_radix_sort_batch(g._h, p(bk), p(bv), p(counts), 2, cap, 44, 44) == B.KS_ERR_INVALID_ARG
    assert L.ks_debug_radix_sort_batch(g._h, p(bk), p(bv), p(counts), 2, cap, 44, 65) == B.KS_ERR_INVALID_ARG
    # none of the refused calls touched the arrays
    assert np.array_equal(k, keys) and np.array_equal(v, vals) and np.array_equal(bk, np.tile(keys, 9)) and np.array_equal(bv, np.tile(vals, 9))
    # ... and the context still sorts
    sort_and_check(g, keys, True, 19, 40, "after the refusals")
    sort_and_check(g, keys.astype(np.uint32), False, 0, 21, "after the refusals")
    check_batch(g, bk[:2 * cap].reshape(2, cap), np.arange(2 * cap, dtype=np.uint32).reshape(2, cap), counts[:2], 44, 64, "after the refusals")
    g.close()
    return {"refused": 20}


CASES = {"range": case_range, "sequence": case_sequence, "batch": case_batch, "errors": case_errors}

RANGES_64 = [(0, 21), (19, 40), (19, 56), (24, 45), (44, 64), (56, 64), (3, 4), (0, 64), (13, 13), (56, 70)]   # (56, 70): clamped to [56, 64)
RANGES_32 = [(0, 21), (19, 40), (24, 45), (3, 4), (0, 32), (13, 13)]                                           # (19, 40), (24, 45): clamped to 32
BIG = (1 << 20) + 1

# name -> spec.  gpu: more than the functional model sorts in its minute (test_sort_cpu.py leaves the spec out).
SPECS = {}
for _kb, _ranges in ((64, RANGES_64), (32, RANGES_32)):
    for _b, _e in _ranges:
        SPECS["range_u%d_%d_%d" % (_kb, _b, _e)] = dict(case="range", key_bits=_kb, b=_b, e=_e, seed=100 * _b + _e + _kb)
SPECS.update({
    "range_u64_equal_in_range": dict(case="range", key_bits=64, b=19, e=40, equal=True, seed=3),
    "range_u32_equal_in_range": dict(case="range", key_bits=32, b=3, e=21, equal=True, seed=4),
    # 2^20 + 1 keys: the 8192-key tile (with values) and the LDS-reordering variant (keys only), the smallest size that takes them (the
    # functional model sorts them in ten seconds); 2^24 + 1: the 16384-key tile, on the device only
    "range_u64_8192_tile_pairs": dict(case="range", key_bits=64, b=19, e=40, sizes=[BIG], modes=[True], seed=5),
    "range_u64_reorder_keys_only": dict(case="range", key_bits=64, b=19, e=56, sizes=[BIG], modes=[False], seed=6),
    "range_u32_reorder_keys_only": dict(case="range", key_bits=32, b=0, e=21, sizes=[BIG], modes=[False], seed=7),
    "range_u64_16384_tile_pairs": dict(case="range", key_bits=64, b=24, e=40, sizes=[(1 << 24) + 1], modes=[True], seed=8, gpu=True),
    "sequence": dict(case="sequence", gpu=True),
    "sequence_small": dict(case="sequence", small=True),
    "batch_3_of_6144": dict(case="batch", cap=6144, counts=[0, 1, 6144]),
    "batch_8_of_10000": dict(case="batch", cap=10000, counts=[10000, 9999, 2048, 2049, 4096, 0, 5000, 20000]),   # (20000: clamped to cap)
    "batch_1_of_6144": dict(case="batch", cap=6144, counts=[4097]),
    "batch_4_of_8192_tiles": dict(case="batch", cap=BIG, counts=[BIG, 1 << 20, 8193, 0], gpu=True),
    "errors": dict(case="errors"),
})


def run_case(spec):
    return CASES[spec["case"]](spec)


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    t0 = time.time()
    rep = run_case(spec)
    rep["seconds"] = round(time.time() - t0, 1)
    print("SORT_CASE_OK", json.dumps(rep))


if __name__ == "__main__":
    main()
