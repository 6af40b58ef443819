"""CPU tier of the ESDF where the nearest site is far away (tests/esdf_far_case.py): the DEVICE CODE of ks_esdf_update and
ks_esdf_refresh on the host functional model (tools/emu) against the NumPy model, bit for bit, at R = 32 .. 255 on rods and
plates whose far sites decide the result — one child process per case, started side by side like those of
tests/test_esdf_cpu.py."""
import json
import sys

import pytest

from tests import esdf_far_case
from tests import test_emu_parity as EP

for _name, _spec in esdf_far_case.SPECS.items():
    EP.JOBS["test_esdf_far_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.esdf_far_case", json.dumps(_spec)], {}, 900, 20 if _spec["R"] >= 100 or _spec["case"] == "refresh" else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(esdf_far_case.SPECS))
def test_esdf_far_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "ESDF_FAR_CASE_OK" in out, out[-3000:] + err[-3000:]
