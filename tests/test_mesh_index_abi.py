"""The ABI of the indexed mesh: the struct as the C compiler sees include/ks_hip.h against the ctypes mirror, the symbol list, and
what the calls refuse without looking at a device (no compute calls: there is no GPU in the CPU test tier; every KS_ERR_* of the
contract on a live context is the case `errors` of tests/mesh_index_case.py, in both tiers)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from kimera_semantics_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ks_mesh_index", "ks_mesh_index_size", "ks_mesh_index_download")
STATS_FIELDS = ["corners", "vertices", "max_corners_per_vertex", "workspace_bytes"]


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
    assert ctypes.sizeof(B.KsMeshIndexStats) == 32
    assert [f for f, _ in B.KsMeshIndexStats._fields_] == STATS_FIELDS
    assert [getattr(B.KsMeshIndexStats, f).offset for f in STATS_FIELDS] == [0, 8, 16, 24]
    assert callable(B.HipIntegrator.mesh_index)


def test_struct_matches_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ks_hip.h"\nint main(void){printf("%zu", sizeof(ks_mesh_index_stats));\n'
                   + "".join('printf(" %%zu", offsetof(ks_mesh_index_stats, %s));\n' % f for f in STATS_FIELDS) + 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [32, 0, 8, 16, 24]


def test_null_contexts_are_refused_without_a_device():
    L = _lib()
    st = B.KsMeshIndexStats(corners=5, vertices=6, max_corners_per_vertex=7, workspace_bytes=8)
    assert L.ks_mesh_index(None, ctypes.byref(st)) == B.KS_ERR_INVALID_ARG
    assert (st.corners, st.vertices, st.max_corners_per_vertex, st.workspace_bytes) == (0, 0, 0, 0)   # zeroed before anything is looked at
    assert L.ks_mesh_index(None, None) == B.KS_ERR_INVALID_ARG
    nv, ni = ctypes.c_size_t(3), ctypes.c_size_t(4)
    assert L.ks_mesh_index_size(None, ctypes.byref(nv), ctypes.byref(ni)) == B.KS_ERR_INVALID_ARG and (nv.value, ni.value) == (3, 4)
    assert L.ks_mesh_index_download(None, None, None, None, None, None, 0, None, 0) == B.KS_ERR_INVALID_ARG
