"""CPU tier of the radix sort's own tests (csrc/ks_radix_sort.h through ks_debug_radix_sort_range / ks_debug_radix_sort_batch).
1. the yardstick on its own: tests/sort_case.expected against Python's sorted(..., key=...) on small inputs, and the keys the cases
   draw hold what they are drawn for — validated before they judge anything;
2. the DEVICE CODE on the host functional model (tools/emu): one child process per spec of tests/sort_case.py that fits the model
   (the 2048-key tile, up to five tiles, a few thousand keys; and the 8192-key tile and the LDS-reordering variant once each, at
   2^20 + 1 keys), started side by side like those of tests/test_emu_parity.py.
3. the ABI of the two entries: declared, listed, exported, and bound with as many parameters as the header gives them.
Part 1 needs no library.  The 16384-key tile, the frame-sized sequence and the large batch are tests/test_sort_gpu.py's alone."""
import json
import sys

import numpy as np
import pytest

from tests import sort_case as S
from tests import test_emu_parity as EP

CPU_SPECS = {k: v for k, v in S.SPECS.items() if not v.get("gpu")}


@pytest.mark.parametrize("key_bits,b,e", [(64, 0, 21), (64, 19, 40), (64, 44, 64), (64, 3, 4), (64, 13, 13), (64, 56, 70), (32, 0, 21), (32, 19, 40), (32, 0, 32)])
def test_yardstick_equals_python_sorted(key_bits, b, e):
    rng = np.random.default_rng(b * 64 + e)
    keys = S.make_keys(rng, 300, key_bits, b, e)
    vals = np.arange(300, dtype=np.uint32)
    hi = min(e, key_bits)
    field = lambda k: (k >> b) & ((1 << max(hi - b, 0)) - 1)
    want = sorted(zip((int(k) for k in keys), range(300)), key=lambda kv: field(kv[0]))     # (sorted() is stable)
    ek, ev = S.expected(keys, vals, b, e)
    assert [int(k) for k in ek] == [k for k, _ in want] and [int(v) for v in ev] == [v for _, v in want]
    assert ek.dtype == keys.dtype and sorted(int(k) for k in ek) == sorted(int(k) for k in keys)
    if hi > b:
        f = [field(int(k)) for k in ek]
        assert f == sorted(f) and len(set(f)) < 300                     # ordered by the field, with equal keys among them
        if b > 0 or hi < key_bits:
            assert any(int(k) != field(int(k)) << b for k in keys)          # ... and bits outside it
            assert [int(k) for k in ek] != sorted(int(k) for k in keys)     # not the order of the whole keys
    else:
        assert np.array_equal(ek, keys) and np.array_equal(ev, vals)


def test_specs_hold_what_they_are_chosen_for():
    for kb, ranges in ((64, S.RANGES_64), (32, S.RANGES_32)):
        assert {(0, 21), (3, 4), (0, kb), (13, 13)} <= set(ranges) and any(e > kb for _, e in ranges)
    assert {(19, 40), (19, 56), (24, 45), (44, 64), (56, 64)} <= set(S.RANGES_64)
    assert S.SIZES == [1, 63, 2048, 2049, 3 * 2048 + 5]
    for name in ("range_u64_equal_in_range", "range_u32_equal_in_range"):
        sp = S.SPECS[name]
        keys = S.make_keys(np.random.default_rng(1), 500, sp["key_bits"], sp["b"], sp["e"], equal=True)
        assert len(np.unique(S.field_of(keys, sp["b"], sp["e"]))) == 1 and len(np.unique(keys)) > 400
        assert np.array_equal(S.expected(keys, None, sp["b"], sp["e"])[0], keys)
    # both sequences: sizes up and down across tile counts, both key widths, both kinds, and a last step whose workspace does not
    # fit what the steps before it made the context allocate (ksrs::ensure allocates a quarter more than it is asked for)
    for steps in (S.SEQUENCE, S.SEQUENCE_SMALL):
        assert len(steps) >= 12 and {s[1] for s in steps} == {32, 64} and {s[2] for s in steps} == {True, False}
        words = [S.workspace_words(n, *S.clamp(kb, b, e)) for (n, kb, _, b, e) in steps]
        assert words[-1] > max(words[:-1]) * 5 // 4 + 4
        assert all(n <= 1 << 20 for n, *_ in steps)
    assert all(n <= 10000 for n, *_ in S.SEQUENCE_SMALL)
    assert S.SPECS["batch_3_of_6144"]["counts"] == [0, 1, 6144] and S.SPECS["batch_8_of_10000"]["counts"] == [10000, 9999, 2048, 2049, 4096, 0, 5000, 20000]
    assert len(S.SPECS["batch_1_of_6144"]["counts"]) == 1
    assert S.SPECS["batch_4_of_8192_tiles"]["counts"] == [S.BIG, 1 << 20, 8193, 0] and S.SPECS["batch_4_of_8192_tiles"]["cap"] == S.BIG == (1 << 20) + 1


def test_diagnostic_entries_are_declared_listed_exported_and_bound_with_the_header_s_parameters():
    import ctypes
    import os
    import re
    from kimera_semantics_amd import binding as B
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(EP.ROOT, "include", "ks_hip.h")).read(), flags=re.S)
    if not os.path.exists(B.LIB_PATH):
        B.build()
    raw, L = ctypes.CDLL(B.LIB_PATH), B.lib()
    for sym, n_params in (("ks_debug_radix_sort", 6), ("ks_debug_radix_sort_range", 7), ("ks_debug_radix_sort_batch", 8)):
        m = re.search(r"\bint %s\s*\(([^)]*)\)\s*;" % sym, header)
        assert m and sym in B.ABI_SYMBOLS and hasattr(raw, sym), sym
        assert len(m.group(1).split(",")) == n_params == len(getattr(L, sym).argtypes), (sym, m.group(1))
    assert callable(B.HipIntegrator.debug_radix_sort_range) and callable(B.HipIntegrator.debug_radix_sort_batch)
    # a NULL context is refused before a device is looked at
    k, v, c = np.zeros(4, np.uint64), np.zeros(4, np.uint32), np.full(1, 4, np.uint64)
    assert L.ks_debug_radix_sort_range(None, k.ctypes.data, v.ctypes.data, 4, 64, 0, 8) == B.KS_ERR_INVALID_ARG
    assert L.ks_debug_radix_sort_batch(None, k.ctypes.data, v.ctypes.data, c.ctypes.data, 1, 4, 0, 8) == B.KS_ERR_INVALID_ARG


# ---- 2. the device code on the functional model: one child per spec, started together by test_emu_parity's fixture ----
for _name, _spec in CPU_SPECS.items():
    EP.JOBS["test_sort_device_code_on_the_host_equals_yardstick[%s]" % _name] = ([sys.executable, "-m", "tests.sort_case", json.dumps(_spec)], {}, 900,
                                                                                   20 if _spec.get("sizes") else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(CPU_SPECS))
def test_sort_device_code_on_the_host_equals_yardstick(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "SORT_CASE_OK" in out, out[-3000:] + err[-3000:]
