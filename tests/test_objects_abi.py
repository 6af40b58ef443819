"""The ABI of the object instances: struct sizes and offsets as the C compiler sees include/ks_hip.h against the ctypes mirrors
and the NumPy record, the defaults, the symbol list (no compute calls: there is no GPU in the CPU test tier)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from kimera_semantics_amd import binding as B
from tests import objects_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ks_objects_default_config", "ks_objects_update", "ks_objects_size", "ks_objects_download", "ks_objects_download_blocks",
           "ks_objects_query")


def test_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "ks_hip.h")).read()
    if not os.path.exists(B.LIB_PATH):
        B.build()
    lib = ctypes.CDLL(B.LIB_PATH)
    for sym in SYMBOLS:
        assert sym in B.ABI_SYMBOLS and ("int %s(" % sym) in header and hasattr(lib, sym), sym


def test_ctypes_mirrors_and_the_record_dtype():
    assert ctypes.sizeof(B.KsObjectsConfig) == 16
    assert [getattr(B.KsObjectsConfig, f).offset for f, _ in B.KsObjectsConfig._fields_] == [0, 4, 8, 12]
    assert ctypes.sizeof(B.KsObjectsStats) == 48 and B.KsObjectsStats.workspace_bytes.offset == 40
    assert [f for f, _ in B.KsObjectsStats._fields_] == ["voxels_surface", "components", "objects", "voxels_in_objects", "largest_object_voxels",
                                                          "workspace_bytes"]
    d = B.OBJECT_DTYPE
    assert d.itemsize == 72 and d == objects_model.RECORD_DTYPE
    assert {k: d.fields[k][1] for k in d.names} == dict(first_voxel=0, n_voxels=12, bb_min=16, bb_max=28, sum=40, label=64, pad=68)
    assert B.KS_OBJECT_NONE == 0xffffffff == int(objects_model.NONE)


def test_structs_match_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "ks_hip.h"\n'
        'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u\\n", sizeof(ks_object), offsetof(ks_object, first_voxel),'
        ' offsetof(ks_object, n_voxels), offsetof(ks_object, bb_min), offsetof(ks_object, bb_max), offsetof(ks_object, sum), offsetof(ks_object, label),'
        ' offsetof(ks_object, pad), sizeof(ks_objects_config), offsetof(ks_objects_config, surface_distance_m), offsetof(ks_objects_config, label_mask),'
        ' offsetof(ks_objects_config, min_voxels), sizeof(ks_objects_stats), offsetof(ks_objects_stats, workspace_bytes), KS_OBJECT_NONE); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [72, 0, 12, 16, 28, 40, 64, 68, 16, 4, 8, 12, 48, 40, 0xffffffff]


def test_defaults():
    if not os.path.exists(B.LIB_PATH):
        B.build()
    cfg = B.KsObjectsConfig()
    assert B.lib().ks_objects_default_config(ctypes.byref(cfg)) == 0
    assert cfg.min_weight == pytest.approx(1e-4, rel=1e-6) and cfg.surface_distance_m == 0.0 and cfg.label_mask == 0x1fffff and cfg.min_voxels == 8
    assert B.lib().ks_objects_default_config(None) == B.KS_ERR_INVALID_ARG
    d = objects_model.DEFAULTS
    assert (d["surface_distance_m"], d["label_mask"], d["min_voxels"]) == (cfg.surface_distance_m, cfg.label_mask, cfg.min_voxels)
