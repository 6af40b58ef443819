"""The ABI of path shortening: the two structs as the C compiler sees include/ks_hip.h against the ctypes mirrors, the enum, the
default configuration, the symbol list in the library and the binding, and what the calls refuse without looking at a device (no
compute calls: there is no GPU in the CPU test tier; every KS_ERR_* on a live context is the case `errors` of
tests/path_shorten_case.py, in both tiers)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

from kimera_semantics_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ks_path_shorten_default_config", "ks_path_shorten", "ks_path_shorten_device")
CONSTANTS = (("KS_SHORTEN_OK", 0), ("KS_SHORTEN_UNVERIFIED", 1), ("KS_SHORTEN_INVALID", 2))


def _structs():
    return (("ks_path_shorten_config", B.KsPathShortenConfig, 32), ("ks_path_shorten_stats", B.KsPathShortenStats, 64))


def _lib():
    if not os.path.exists(B.LIB_PATH):
        B.build()
    return B.lib()


def test_symbols_are_declared_listed_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ks_hip.h")).read()
    _lib()
    lib = ctypes.CDLL(B.LIB_PATH)
    for sym in SYMBOLS:
        assert sym in B.ABI_SYMBOLS and ("int %s(" % sym) in header and hasattr(lib, sym), sym
    for method in ("shorten_paths", "shorten_paths_device", "path_shorten_config"):
        assert callable(getattr(B.HipIntegrator, method)), method
    assert len(getattr(B.lib(), "ks_path_shorten").argtypes) == len(getattr(B.lib(), "ks_path_shorten_device").argtypes) == 12


def test_ctypes_mirrors():
    for name, mirror, size in _structs():
        assert ctypes.sizeof(mirror) == size, name
    assert [f for f, _ in B.KsPathShortenConfig._fields_] == ["radius_m", "min_step_m", "unknown_is_free", "max_samples", "lookahead", "pad"]
    assert [f for f, _ in B.KsPathShortenStats._fields_] == ["paths_ok", "paths_unverified", "paths_invalid", "waypoints_in", "waypoints_out",
                                                             "segments_unverified", "sweeps", "samples"]
    assert [getattr(B, name) for name, _ in CONSTANTS] == [value for _, value in CONSTANTS]


def test_structs_and_constants_match_the_c_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no C compiler"
    prints, want = [], []
    for name, mirror, size in _structs():
        prints.append('printf(" %%zu", sizeof(%s));' % name)
        want.append(size)
        for f, _ in mirror._fields_:
            prints.append('printf(" %%zu", offsetof(%s, %s));' % (name, f))
            want.append(getattr(mirror, f).offset)
    for name, value in CONSTANTS:
        prints.append('printf(" %%llu", (unsigned long long)%s);' % name)
        want.append(value)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ks_hip.h"\nint main(void){\n' + "\n".join(prints) + '\nprintf("\\n"); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_default_config():
    L = _lib()
    cfg = B.KsPathShortenConfig(radius_m=7.0, min_step_m=7.0, unknown_is_free=7, max_samples=7, lookahead=7, pad=(7, 7, 7))
    assert L.ks_path_shorten_default_config(ctypes.byref(cfg)) == 0
    assert cfg.radius_m == np.float32(0.3) and (cfg.min_step_m, cfg.unknown_is_free, cfg.max_samples, cfg.lookahead, tuple(cfg.pad)) == (0.0, 0, 4096, 64, (0, 0, 0))
    assert L.ks_path_shorten_default_config(None) == B.KS_ERR_INVALID_ARG


def test_null_contexts_are_refused_without_a_device():
    L = _lib()
    cfg, st = B.KsPathShortenConfig(), B.KsPathShortenStats(sweeps=5)
    L.ks_path_shorten_default_config(ctypes.byref(cfg))
    p = np.zeros(8, np.float32).ctypes.data
    for fn in (L.ks_path_shorten, L.ks_path_shorten_device):
        assert fn(None, p, p, 1, 2, ctypes.byref(cfg), p, None, None, None, None, ctypes.byref(st)) == B.KS_ERR_INVALID_ARG
