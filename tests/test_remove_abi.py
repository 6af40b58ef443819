"""The ABI of block removal: the struct as the C compiler sees include/ks_hip.h against the ctypes mirror, the symbol list (no
compute calls: there is no GPU in the CPU test tier)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from kimera_semantics_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ks_remove_blocks", "ks_remove_distant_blocks", "ks_removed_blocks")


def test_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "ks_hip.h")).read()
    if not os.path.exists(B.LIB_PATH):
        B.build()
    lib = ctypes.CDLL(B.LIB_PATH)
    for sym in SYMBOLS:
        assert sym in B.ABI_SYMBOLS and ("int %s(" % sym) in header and hasattr(lib, sym), sym


def test_ctypes_mirror():
    assert ctypes.sizeof(B.KsRemoveStats) == 40
    assert [f for f, _ in B.KsRemoveStats._fields_] == ["blocks_removed", "tiles_removed", "tiles_moved", "tiles_resident", "pool_capacity_tiles"]
    assert [getattr(B.KsRemoveStats, f).offset for f, _ in B.KsRemoveStats._fields_] == [0, 8, 16, 24, 32]
    for name in ("remove_blocks", "remove_distant", "removed_blocks"):
        assert callable(getattr(B.HipIntegrator, name))


def test_struct_matches_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "ks_hip.h"\n'
        'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ks_remove_stats), offsetof(ks_remove_stats, blocks_removed),'
        ' offsetof(ks_remove_stats, tiles_removed), offsetof(ks_remove_stats, tiles_moved), offsetof(ks_remove_stats, tiles_resident),'
        ' offsetof(ks_remove_stats, pool_capacity_tiles)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [40, 0, 8, 16, 24, 32]


def test_null_context_is_refused_without_a_device():
    if not os.path.exists(B.LIB_PATH):
        B.build()
    L = B.lib()
    n = ctypes.c_size_t()
    assert L.ks_remove_blocks(None, None, 0, None) == B.KS_ERR_INVALID_ARG
    assert L.ks_remove_distant_blocks(None, None, 1.0, None) == B.KS_ERR_INVALID_ARG
    assert L.ks_removed_blocks(None, None, 0, ctypes.byref(n)) == B.KS_ERR_INVALID_ARG
