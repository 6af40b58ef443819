"""The ABI of the rooms: the four structs as the C compiler sees include/ks_hip.h against the ctypes mirrors and the NumPy record
types, the constant, the default configuration, the symbol list, and what the calls refuse without looking at a device (no compute
calls: there is no GPU in the CPU test tier).  Every KS_ERR_* on a live context, the n = 0 reads and the capacities that are too
small are the case `errors` of tests/rooms_case.py, which runs in both tiers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from kimera_semantics_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ks_rooms_default_config", "ks_rooms_update", "ks_rooms_size", "ks_rooms_download", "ks_rooms_links_download", "ks_rooms_objects",
           "ks_rooms_download_blocks", "ks_rooms_query")
# (the fields the contract lists for ks_rooms_config take 48 bytes without padding: two floats, three uint32, seven int32)
STRUCTS = (("ks_rooms_config", B.KsRoomsConfig, 48), ("ks_rooms_stats", B.KsRoomsStats, 120))
RECORDS = (("ks_room", B.ROOM_DTYPE, 96), ("ks_room_link", B.ROOM_LINK_DTYPE, 32))


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
    for name, dtype, size in RECORDS:
        assert dtype.itemsize == size, name
    assert [f for f, _ in B.KsRoomsConfig._fields_] == ["free_distance_m", "core_distance_m", "min_core_voxels", "max_cost", "max_rounds", "use_bounds",
                                                        "bounds_min", "bounds_max"]
    assert [f for f, _ in B.KsRoomsStats._fields_] == ["voxels_free", "voxels_core", "components", "rooms", "voxels_assigned", "voxels_unassigned",
                                                       "largest_room_voxels", "largest_cost", "links", "contacts", "objects_seen", "objects_joined",
                                                       "rounds", "tile_relaxations", "workspace_bytes"]
    assert B.KS_ROOM_NONE == 0xffffffff == B.KS_NAV_BLOCKED == B.KS_OBJECT_NONE
    from tests import rooms_model
    assert rooms_model.ROOM_DTYPE == B.ROOM_DTYPE and rooms_model.LINK_DTYPE == B.ROOM_LINK_DTYPE


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
    for name, dtype, size in RECORDS:
        prints.append('printf(" %%zu", sizeof(%s));' % name)
        want.append(size)
        for f in dtype.names:
            prints.append('printf(" %%zu", offsetof(%s, %s));' % (name, f))
            want.append(dtype.fields[f][1])
    prints.append('printf(" %llu", (unsigned long long)KS_ROOM_NONE);')
    want.append(B.KS_ROOM_NONE)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ks_hip.h"\nint main(void){\n' + "\n".join(prints) + '\nprintf("\\n"); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_default_config():
    L = _lib()
    cfg = B.KsRoomsConfig(free_distance_m=7.0, core_distance_m=7.0, min_core_voxels=7, max_cost=7, max_rounds=7, use_bounds=7)
    cfg.bounds_min[1] = cfg.bounds_max[2] = 7
    assert L.ks_rooms_default_config(ctypes.byref(cfg)) == 0
    assert (cfg.free_distance_m, cfg.core_distance_m, cfg.min_core_voxels, cfg.max_cost, cfg.max_rounds, cfg.use_bounds) == (0.0, 0.5, 64, 0, 0, 0)
    assert list(cfg.bounds_min) == [0, 0, 0] == list(cfg.bounds_max)
    assert L.ks_rooms_default_config(None) == B.KS_ERR_INVALID_ARG


def test_null_contexts_are_refused_without_a_device():
    L = _lib()
    cfg, st = B.KsRoomsConfig(), B.KsRoomsStats(rounds=5)
    L.ks_rooms_default_config(ctypes.byref(cfg))
    a = np.zeros(64, np.float32)
    p, n = a.ctypes.data, ctypes.c_size_t(3)
    assert L.ks_rooms_update(None, ctypes.byref(cfg), ctypes.byref(st)) == B.KS_ERR_INVALID_ARG
    assert L.ks_rooms_size(None, ctypes.byref(n), ctypes.byref(n)) == B.KS_ERR_INVALID_ARG
    for fn in (L.ks_rooms_download, L.ks_rooms_links_download, L.ks_rooms_objects):
        assert fn(None, p, 1, ctypes.byref(n)) == B.KS_ERR_INVALID_ARG and n.value == 3
    assert L.ks_rooms_download_blocks(None, p, 1, p, p) == B.KS_ERR_INVALID_ARG
    assert L.ks_rooms_query(None, p, 1, p) == B.KS_ERR_INVALID_ARG
