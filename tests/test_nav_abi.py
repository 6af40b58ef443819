"""The ABI of the navigation field: the three structs as the C compiler sees include/ks_hip.h against the ctypes mirrors, the
constants, the default configuration, the symbol list, and what the calls refuse without looking at a device (no compute calls:
there is no GPU in the CPU test tier; every KS_ERR_* on a live context is the case `errors` of tests/nav_case.py, in both tiers)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from kimera_semantics_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ks_nav_default_config", "ks_nav_update", "ks_nav_query", "ks_nav_query_device", "ks_nav_download_blocks", "ks_nav_paths",
           "ks_nav_paths_device")
STRUCTS = (("ks_nav_config", B.KsNavConfig, 16), ("ks_nav_stats", B.KsNavStats, 64), ("ks_nav_path_stats", B.KsNavPathStats, 40))
CONSTANTS = ("KS_NAV_BLOCKED", "KS_NAV_UNREACHED", "KS_NAV_MAX_COST", "KS_NAV_COST_FACE", "KS_NAV_COST_EDGE", "KS_NAV_COST_CORNER",
             "KS_NAV_PATH_REACHED", "KS_NAV_PATH_UNREACHABLE", "KS_NAV_PATH_BLOCKED", "KS_NAV_PATH_TRUNCATED", "KS_NAV_PATH_INVALID")


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
    assert [f for f, _ in B.KsNavConfig._fields_] == ["radius_m", "max_cost", "max_rounds", "pad"]
    assert [f for f, _ in B.KsNavStats._fields_] == ["voxels_traversable", "voxels_reached", "goals_used", "goals_blocked", "largest_cost", "rounds",
                                                     "tile_relaxations", "workspace_bytes"]
    assert [f for f, _ in B.KsNavPathStats._fields_] == ["paths_reached", "paths_unreachable", "paths_blocked", "paths_truncated", "waypoints"]
    assert (B.KS_NAV_BLOCKED, B.KS_NAV_UNREACHED, B.KS_NAV_MAX_COST) == (0xffffffff, 0xfffffffe, 0xffffff00)
    assert (B.KS_NAV_COST_FACE, B.KS_NAV_COST_EDGE, B.KS_NAV_COST_CORNER) == (10, 14, 17)


def test_structs_and_constants_match_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    prints, want = [], []
    for name, mirror, size in STRUCTS:
        prints.append('printf(" %%zu", sizeof(%s));' % name)
        want.append(size)
        for f, _ in mirror._fields_:
            prints.append('printf(" %%zu", offsetof(%s, %s));' % (name, f))
            want.append(getattr(mirror, f).offset)
    for name in CONSTANTS:
        prints.append('printf(" %%llu", (unsigned long long)%s);' % name)
        want.append(getattr(B, name))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ks_hip.h"\nint main(void){\n' + "\n".join(prints) + '\nprintf("\\n"); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_default_config():
    L = _lib()
    cfg = B.KsNavConfig(radius_m=7.0, max_cost=7, max_rounds=7, pad=7)
    assert L.ks_nav_default_config(ctypes.byref(cfg)) == 0
    assert cfg.radius_m == np.float32(0.3) and (cfg.max_cost, cfg.max_rounds, cfg.pad) == (0, 0, 0)
    assert L.ks_nav_default_config(None) == B.KS_ERR_INVALID_ARG


def test_null_contexts_are_refused_without_a_device():
    L = _lib()
    cfg, st, ps = B.KsNavConfig(), B.KsNavStats(rounds=5), B.KsNavPathStats(waypoints=6)
    L.ks_nav_default_config(ctypes.byref(cfg))
    a = np.zeros(8, np.float32)
    p = a.ctypes.data
    assert L.ks_nav_update(None, p, 1, ctypes.byref(cfg), ctypes.byref(st)) == B.KS_ERR_INVALID_ARG
    for fn in (L.ks_nav_query, L.ks_nav_query_device, L.ks_nav_download_blocks):
        assert fn(None, p, 1, p) == B.KS_ERR_INVALID_ARG
    for fn in (L.ks_nav_paths, L.ks_nav_paths_device):
        assert fn(None, p, 1, 4, p, None, None, None, ctypes.byref(ps)) == B.KS_ERR_INVALID_ARG
