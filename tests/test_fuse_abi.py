"""The ABI of submap fusion: the structs as the C compiler sees include/ks_hip.h against the ctypes mirror, the default config, the
symbol list, and what the call refuses without looking at a device (no compute calls: there is no GPU in the CPU test tier; every
KS_ERR_* of the contract's point 9 on a live context is the case `errors` of tests/fuse_case.py, in both tiers)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from kimera_semantics_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ks_fuse_default_config", "ks_fuse_map")
STATS_FIELDS = ["tiles_source", "tiles_candidate", "tiles_touched", "tiles_allocated", "voxels_fused", "chunks", "workspace_bytes"]


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


def test_ctypes_mirror():
    assert ctypes.sizeof(B.KsFuseConfig) == 16 and ctypes.sizeof(B.KsFuseStats) == 56
    assert [f for f, _ in B.KsFuseConfig._fields_] == ["min_weight", "pad", "max_workspace_bytes"]
    assert [getattr(B.KsFuseConfig, f).offset for f, _ in B.KsFuseConfig._fields_] == [0, 4, 8]
    assert [f for f, _ in B.KsFuseStats._fields_] == STATS_FIELDS
    assert [getattr(B.KsFuseStats, f).offset for f in STATS_FIELDS] == [8 * k for k in range(7)]
    assert callable(B.HipIntegrator.fuse)


def test_structs_match_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "ks_hip.h"\n'
        'int main(void){printf("%zu %zu %zu %zu %zu", sizeof(ks_fuse_config), offsetof(ks_fuse_config, min_weight), offsetof(ks_fuse_config, pad),'
        ' offsetof(ks_fuse_config, max_workspace_bytes), sizeof(ks_fuse_stats));\n'
        + "".join('printf(" %%zu", offsetof(ks_fuse_stats, %s));\n' % f for f in STATS_FIELDS) + 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [16, 0, 4, 8, 56] + [8 * k for k in range(7)]


def test_default_config():
    L = _lib()
    cfg = B.KsFuseConfig(min_weight=7.0, pad=9, max_workspace_bytes=3)
    assert L.ks_fuse_default_config(ctypes.byref(cfg)) == 0
    assert cfg.min_weight == np.float32(1e-4) and cfg.pad == 0 and cfg.max_workspace_bytes == 1 << 30
    assert L.ks_fuse_default_config(None) == B.KS_ERR_INVALID_ARG


def test_null_contexts_are_refused_without_a_device():
    L = _lib()
    cfg, st = B.KsFuseConfig(), B.KsFuseStats(tiles_source=5, chunks=6)
    L.ks_fuse_default_config(ctypes.byref(cfg))
    T = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)
    assert L.ks_fuse_map(None, None, T.ctypes.data, ctypes.byref(cfg), ctypes.byref(st)) == B.KS_ERR_INVALID_ARG
    assert st.tiles_source == 0 and st.chunks == 0           # the stats are zeroed before anything is looked at
    assert L.ks_fuse_map(None, None, None, None, None) == B.KS_ERR_INVALID_ARG
