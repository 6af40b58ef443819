"""The ABI of the view information gain: the three structs as the C compiler sees include/ks_hip.h against the ctypes mirrors, the
default configuration, the symbol list, and what the calls refuse without looking at a device (no compute calls: there is no GPU in
the CPU test tier; every KS_ERR_* on a live context is the case `errors` of tests/view_gain_case.py, in both tiers)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from kimera_semantics_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ks_view_gain_default_config", "ks_view_gain", "ks_view_gain_device")
STRUCTS = (("ks_view_gain_config", "KsViewGainConfig", 56), ("ks_view_gain_stats", "KsViewGainStats", 88))
RECORD = ("unknown_voxels", "free_voxels", "surface_voxels", "label_voxels", "rays_hit", "rays_open", "samples", "flags")


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
        assert ctypes.sizeof(getattr(B, mirror)) == size, name
    assert [f for f, _ in B.KsViewGainConfig._fields_] == ["min_range_m", "max_range_m", "step_m", "stop_distance_m", "width", "height", "K", "label", "pad",
                                                           "max_workspace_bytes"]
    assert [f for f, _ in B.KsViewGainStats._fields_] == ["views_valid", "views_invalid", "unknown_voxels", "free_voxels", "surface_voxels", "label_voxels",
                                                          "rays_hit", "rays_open", "samples", "workspace_bytes", "views_in_lds"]
    assert B.VIEW_GAIN_DTYPE.names == RECORD and B.VIEW_GAIN_DTYPE.itemsize == 32 and B.KS_VIEW_GAIN_VALID == 1
    assert all(B.VIEW_GAIN_DTYPE.fields[k] == (np.dtype("<u4"), 4 * j) for j, k in enumerate(RECORD))


def test_structs_and_constants_match_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    prints, want = [], []
    for name, mirror, size in STRUCTS:
        prints.append('printf(" %%zu", sizeof(%s));' % name)
        want.append(size)
        for f, _ in getattr(B, mirror)._fields_:
            prints.append('printf(" %%zu", offsetof(%s, %s));' % (name, f))
            want.append(getattr(getattr(B, mirror), f).offset)
    prints.append('printf(" %zu", sizeof(ks_view_gain_record));')
    want.append(32)
    for j, f in enumerate(RECORD):
        prints.append('printf(" %%zu", offsetof(ks_view_gain_record, %s));' % f)
        want.append(4 * j)
    prints.append('printf(" %llu", (unsigned long long)KS_VIEW_GAIN_VALID);')
    want.append(B.KS_VIEW_GAIN_VALID)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ks_hip.h"\nint main(void){\n' + "\n".join(prints) + '\nprintf("\\n"); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_default_config():
    L = _lib()
    cfg = B.KsViewGainConfig(min_range_m=7.0, max_range_m=7.0, step_m=7.0, stop_distance_m=7.0, width=7, height=7, label=7, pad=7, max_workspace_bytes=7)
    cfg.K = (ctypes.c_float * 4)(7, 7, 7, 7)
    assert L.ks_view_gain_default_config(ctypes.byref(cfg)) == 0
    assert (cfg.min_range_m, cfg.max_range_m, cfg.step_m, cfg.stop_distance_m) == (0.0, 5.0, 0.0, 0.0)
    assert (cfg.width, cfg.height, cfg.label, cfg.pad, cfg.max_workspace_bytes) == (32, 24, 255, 0, 1 << 30) and list(cfg.K) == [0.0] * 4
    assert L.ks_view_gain_default_config(None) == B.KS_ERR_INVALID_ARG


def test_null_contexts_are_refused_without_a_device():
    L = _lib()
    cfg, st = B.KsViewGainConfig(), B.KsViewGainStats(samples=5)
    L.ks_view_gain_default_config(ctypes.byref(cfg))
    a = np.zeros(8, np.float32)
    p = a.ctypes.data
    for fn in (L.ks_view_gain, L.ks_view_gain_device):
        assert fn(None, p, 1, ctypes.byref(cfg), p, ctypes.byref(st)) == B.KS_ERR_INVALID_ARG
