"""CPU tier of the incremental ESDF refresh (DESIGN.md, section "ESDF", incremental refresh): the DEVICE CODE and the host code
of ks_esdf_refresh on the host functional model (tools/emu) against the NumPy model of the map as it is after each refresh,
bit for bit — one child process per case (tests/esdf_refresh_case.py), started side by side like those of
tests/test_esdf_cpu.py — and the new symbols and the struct layout through the binding."""
import ctypes
import json
import sys

import pytest

from tests import esdf_refresh_case
from tests import test_emu_parity as EP

for _name, _spec in esdf_refresh_case.SPECS.items():
    EP.JOBS["test_esdf_refresh_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.esdf_refresh_case", json.dumps(_spec)], {}, 900, 40 if _spec["case"] in ("mutate", "integrated") else 20)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(esdf_refresh_case.SPECS))
def test_esdf_refresh_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "ESDF_REFRESH_CASE_OK" in out, out[-3000:] + err[-3000:]


def test_esdf_refresh_symbols_and_struct_layout():
    from kimera_semantics_amd import binding as B
    for sym in ("ks_esdf_refresh", "ks_esdf_changed_blocks"):
        assert sym in B.ABI_SYMBOLS and hasattr(B.lib(), sym), sym
    assert ctypes.sizeof(B.KsEsdfRefreshStats) == 56
    assert [n for n, _ in B.KsEsdfRefreshStats._fields_] == ["tiles_stale", "tiles_recomputed", "tiles_total", "voxels_observed",
                                                             "voxels_fixed", "voxels_clamped", "workspace_bytes"]
    assert B.KsEsdfRefreshStats.voxels_observed.offset == 24 and B.KsEsdfRefreshStats.workspace_bytes.offset == 48
    assert ctypes.sizeof(B.KsEsdfConfig) == 48 and ctypes.sizeof(B.KsEsdfStats) == 56   # (unchanged)
    assert B.lib().ks_esdf_refresh(None, 0, None) == B.KS_ERR_INVALID_ARG
    n = ctypes.c_size_t()
    assert B.lib().ks_esdf_changed_blocks(None, None, 0, ctypes.byref(n)) == B.KS_ERR_INVALID_ARG
