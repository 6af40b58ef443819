"""The ABI of the ESDF reads: the three structs as the C compiler sees include/ks_hip.h against the ctypes mirrors, the enums, the
default sweep configuration, the symbol list, and what the calls refuse without looking at a device (no compute calls: there is no
GPU in the CPU test tier; every KS_ERR_* on a live context is the case `errors` of tests/esdf_read_case.py, in both tiers)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from kimera_semantics_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ks_esdf_sample", "ks_esdf_sample_device", "ks_esdf_slice", "ks_esdf_slice_device", "ks_esdf_sweep_default_config", "ks_esdf_sweep",
           "ks_esdf_sweep_device")
STRUCTS = (("ks_esdf_sample_stats", B.KsEsdfSampleStats, 24), ("ks_esdf_sweep_config", B.KsEsdfSweepConfig, 16),
           ("ks_esdf_sweep_stats", B.KsEsdfSweepStats, 40))


def _lib():
    if not os.path.exists(B.LIB_PATH):
        B.build()
    return B.lib()


def test_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "ks_hip.h")).read()
    _lib()
    lib = ctypes.CDLL(B.LIB_PATH)
    for sym in SYMBOLS:
        assert sym in B.ABI_SYMBOLS and ("int %s(" % sym) in header and hasattr(lib, sym), sym


def test_ctypes_mirrors():
    for name, mirror, size in STRUCTS:
        assert ctypes.sizeof(mirror) == size, name
    assert [f for f, _ in B.KsEsdfSampleStats._fields_] == ["points_interpolated", "points_nearest", "points_unknown"]
    assert [f for f, _ in B.KsEsdfSweepConfig._fields_] == ["radius_m", "min_step_m", "unknown_is_free", "max_samples"]
    assert [f for f, _ in B.KsEsdfSweepStats._fields_] == ["segments_free", "segments_collision", "segments_unknown", "segments_invalid", "samples"]
    assert (B.KS_ESDF_UNKNOWN, B.KS_ESDF_NEAREST, B.KS_ESDF_INTERPOLATED) == (0, 1, 2)
    assert (B.KS_SWEEP_FREE, B.KS_SWEEP_COLLISION, B.KS_SWEEP_UNKNOWN, B.KS_SWEEP_INVALID) == (0, 1, 2, 3)


def test_structs_match_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    prints, want = [], []
    for name, mirror, size in STRUCTS:
        prints.append('printf(" %%zu", sizeof(%s));' % name)
        want.append(size)
        for f, _ in mirror._fields_:
            prints.append('printf(" %%zu", offsetof(%s, %s));' % (name, f))
            want.append(getattr(mirror, f).offset)
    prints.append('printf(" %d %d %d %d %d %d %d", KS_ESDF_UNKNOWN, KS_ESDF_NEAREST, KS_ESDF_INTERPOLATED, KS_SWEEP_FREE, KS_SWEEP_COLLISION,'
                  ' KS_SWEEP_UNKNOWN, KS_SWEEP_INVALID);')
    want += [0, 1, 2, 0, 1, 2, 3]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ks_hip.h"\nint main(void){\n' + "\n".join(prints) + '\nprintf("\\n"); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_default_sweep_config():
    L = _lib()
    cfg = B.KsEsdfSweepConfig(radius_m=7.0, min_step_m=7.0, unknown_is_free=9, max_samples=3)
    assert L.ks_esdf_sweep_default_config(ctypes.byref(cfg)) == 0
    assert cfg.radius_m == np.float32(0.3) and cfg.min_step_m == 0.0 and cfg.unknown_is_free == 0 and cfg.max_samples == 4096
    assert L.ks_esdf_sweep_default_config(None) == B.KS_ERR_INVALID_ARG


def test_null_contexts_are_refused_without_a_device():
    L = _lib()
    st, ss, cfg = B.KsEsdfSampleStats(points_unknown=5), B.KsEsdfSweepStats(samples=6), B.KsEsdfSweepConfig()
    L.ks_esdf_sweep_default_config(ctypes.byref(cfg))
    a = np.zeros(8, np.float32)
    p = a.ctypes.data
    for fn in (L.ks_esdf_sample, L.ks_esdf_sample_device):
        assert fn(None, p, 1, p, None, None, None, None, ctypes.byref(st)) == B.KS_ERR_INVALID_ARG
    for fn in (L.ks_esdf_slice, L.ks_esdf_slice_device):
        assert fn(None, p, p, p, 1, 1, p, None, None, None, None, ctypes.byref(st)) == B.KS_ERR_INVALID_ARG
    for fn in (L.ks_esdf_sweep, L.ks_esdf_sweep_device):
        assert fn(None, p, 1, ctypes.byref(cfg), None, p, None, None, ctypes.byref(ss)) == B.KS_ERR_INVALID_ARG
