"""CPU tier of the integer-sum voxel update (csrc/ks_k_apply_xl.h) at ties, binade edges and clamps.
1. the plain model (tests/xl_model.py) on its own, no library involved: where its rule holds the integer-sum formula equals the serial
   f32 chain bit for bit, on a constructed tie it does not (for one parity of M: why the kernel replays), the start-state rule, the
   tie-binade rule of the probability search — the yardstick is validated before it judges anything;
2. the DEVICE CODE on the host functional model (tools/emu) against the oracle and the model: one child process per case
   (tests/xl_case.py), started side by side like those of tests/test_emu_parity.py.
The functional model replaces the DPP wavefront sum (wave_sum_i32_dpp) by its own: only tests/test_xl_gpu.py runs that one."""
import json
import sys

import numpy as np
import pytest

from tests import test_emu_parity as EP
from tests import xl_case
from tests import xl_model as M

F = np.float32


def _uniform(n, x_class=-1.609438, x_label=-0.2231436, uw=1.0):
    inc = np.empty((M.CHAINS, n), F)
    inc[:M.NUM_LABELS] = F(x_class)
    inc[3] = F(x_label)
    inc[M.NUM_LABELS] = F(uw)
    return inc


def test_model_no_tie_no_crossing_predicts_no_replay_and_the_integer_sum_is_the_serial_chain():
    p0 = np.concatenate([np.full(M.NUM_LABELS, F(-4100.25), F), [F(2.0)]])
    p0[3] = F(-520.5)
    inc = _uniform(1500)
    R = M.classify(p0, inc, max_weight=2.0)
    assert R.n_chunks == 6 and R.replays_needed == 0 and all(R.ok) and not R.handed_back and R.binades_spanned == 1, R.summary()
    for c in (0, 3, 20):
        assert M.bits(M.integer_sum(p0[c], inc[c])) == M.bits(M.serial_chain(p0[c], inc[c])[-1])
    # ... chunk by chunk as the walk does it, and for a weight below its clamp
    p = p0[0]
    for b in range(R.n_chunks):
        p = M.integer_sum(p, inc[0, b * M.CHUNK:(b + 1) * M.CHUNK])
    assert M.bits(p) == M.bits(R.end[0])
    R = M.classify(np.concatenate([p0[:M.NUM_LABELS], [F(2100.0)]]), inc, max_weight=1e4)
    assert R.replays_needed == 0 and R.end[M.NUM_LABELS] == F(3600.0)
    assert M.bits(M.integer_sum(F(2100.0), inc[M.NUM_LABELS])) == M.bits(F(3600.0))


def test_model_on_a_constructed_tie_the_integer_sum_differs_for_one_parity_of_m():
    x = F(-1.5)                                  # 3 * 2^-1: a tie where the spacing is 1, in [2^23, 2^24)
    E = M.tie_binade(x)
    assert E == 127 + 23 and M.trailing_zeros(x) == 22
    differs = []
    for m in (0x900000, 0x900001):               # an even and an odd M
        p0 = F(-float(m))
        serial = M.serial_chain(p0, [x])[-1]
        assert float(serial) in (-(m + 1.0), -(m + 2.0)) and int(-float(serial)) % 2 == 0   # the tie goes to the even sum
        differs.append(M.bits(M.integer_sum(p0, [x])) != M.bits(serial))
    assert differs.count(True) == 1, differs     # R = 2 for both: right for the even M, wrong for the odd one
    # ... and classify says so: every chunk of a run in that binade needs its replay, and such a run is handed back
    p0 = np.concatenate([np.full(M.NUM_LABELS, F(-float(0x900001)), F), [F(2.0)]])
    inc = _uniform(3000, x_class=-1.5, x_label=-1.5)
    R = M.classify(p0, inc, max_weight=2.0)
    assert R.tie_chunks == list(range(12)) and R.replays_needed == 12 and R.budget == 9 and R.handed_back and R.replayed == 10, R.summary()
    R = M.classify(np.concatenate([np.full(M.NUM_LABELS, F(-4.0e6), F), [F(2.0)]]), inc, max_weight=2.0)
    assert R.tie_chunks == [] and R.replays_needed == 0                       # a binade below: |x| / u = 3, no tie


def test_model_classifies_crossings_far_binades_clamps_and_signs():
    inc = _uniform(2048)
    at_clamp = [F(2.0)]
    R = M.classify(np.concatenate([np.full(M.NUM_LABELS, F(-1900.0), F), at_clamp]), _uniform(1024, x_label=-1.609438), max_weight=2.0)
    crossing = int((2048 - 1900) / 1.609438) // M.CHUNK
    assert [b for b, ok in enumerate(R.ok) if not ok] == [crossing] and R.reasons[crossing] == ["leaves_binade"] and R.binades_spanned == 2
    # a start of -0.6: the increments are 2^22 spacings and more, and the sums cross more than eight binades
    R = M.classify(np.concatenate([np.full(M.NUM_LABELS, M.PRIOR_INIT, F), at_clamp]), _uniform(4000), max_weight=2.0)
    assert R.replays_needed == 16 and R.handed_back and R.binades_spanned >= 9 and "increment_too_large" in R.reasons[0] and "beyond_eight_binades" in R.reasons[-1]
    # the weight meets the clamp in chunk 1 and sits at it afterwards
    R = M.classify(np.concatenate([np.full(M.NUM_LABELS, F(-9000.0), F), [F(1100.0)]]), inc, max_weight=1400.0)
    assert [b for b, ok in enumerate(R.ok) if not ok] == [1] and R.reasons[1] == ["weight_meets_clamp"] and R.end[M.NUM_LABELS] == F(1400.0)
    # a positive class increment
    bad = inc.copy()
    bad[7, 300] = F(0.25)
    R = M.classify(np.concatenate([np.full(M.NUM_LABELS, F(-9000.0), F), at_clamp]), bad, max_weight=2.0)
    assert [b for b, ok in enumerate(R.ok) if not ok] == [1] and R.reasons[1] == ["sign"]


def test_model_start_state_rule():
    ok = dict(distance=F(0.2), weight=F(2.0), priors=np.full(M.NUM_LABELS, F(-100.0), F))
    assert M.accepts(ok, 1, 0.2, 2.0) and M.accepts(ok, 2, 0.2, 2.0) and M.accepts(dict(ok, weight=M.EPS), 1, 0.2, 2.0)
    assert not M.accepts(ok, 0, 0.2, 2.0)
    assert not M.accepts(dict(ok, distance=np.nextafter(F(0.2), F(0))), 1, 0.2, 2.0)
    for w in (0.0, np.nextafter(F(2.0), F(3.0)), np.nextafter(M.EPS, F(0))):
        assert not M.accepts(dict(ok, weight=F(w)), 1, 0.2, 2.0)
    assert not M.accepts(dict(ok, weight=F(2.0)), 1, 0.2, 1e30)
    for b in (0x00000000, 0x80000000, M.bits(F(3.5)), 0x80000001, 0x807FFFFF, 0xFF800000, 0xFF000000, 0xFFC00000):
        pr = ok["priors"].copy()
        pr[7] = M.from_bits(b)
        assert not M.accepts(dict(ok, priors=pr), 1, 0.2, 2.0), hex(b)
    pr = ok["priors"].copy()
    pr[7], pr[8] = M.from_bits(0xFEFFFFFF), M.from_bits(0x80800000)          # the largest and the smallest it takes
    assert M.accepts(dict(ok, priors=pr), 1, 0.2, 2.0)


def test_model_search_finds_a_tie_in_the_asked_binade_only():
    # (NumPy's logarithm stands in for the oracle's here: the search must verify whatever it is given)
    p, x = M.search_probability(lambda q: np.log(F(1) - F(q), dtype=F), 138, lo=0.5005)
    assert 0.5 < p < 0.51 and M.tie_binade(x) == 138 and M.is_tie(x, 138) and not M.is_tie(x, 137) and not M.is_tie(x, 139)
    assert M.tie_binade(F(2) * x) == 139 and M.tie_binade(F(4) * x) == 140     # bundles of `merged`: c log moves the binade
    assert M.tie_binade(F(-1.75)) == 127 + 22                                  # 21 trailing zeros from 2^0 on: ties where no sum ever gets


def test_specs_hold_every_edge_by_name_and_state_a_precondition():
    assert set(xl_case.SPECS) >= {"len_1024", "len_1025", "len_1280", "len_1500", "tie_walked", "tie_handed_back", "tie_merged_bundles",
                                  "binades_nine_handed_back", "binades_seven_walked", "binade_left_on_first_update", "binade_exact_power_of_two",
                                  "weight_meets_clamp", "weight_meets_clamp_late", "weight_at_clamp_from_start", "weight_below_clamp_inverse_square", "distance_leaves_clamp",
                                  "refuse_plus_zero", "refuse_positive", "refuse_denormal", "refuse_minus_inf", "refuse_exponent_254", "refuse_weight_zero",
                                  "refuse_weight_above_max", "refuse_max_weight_1e30", "refuse_distance_one_ulp_below", "refuse_colour_blend",
                                  "merged_lanes_weight_stays_below", "merged_lanes_weight_meets_clamp", "merged_lanes_probability_colours",
                                  "two_runs_different_fates", "two_runs_chunk_cap"}
    for name, sp in xl_case.SPECS.items():
        assert sp["require"], name                                            # every case states its precondition
        assert json.loads(json.dumps(sp)) == sp, name


# ---- 2. the device code on the functional model: one child per case, started together by test_emu_parity's fixture ----
for _name, _spec in xl_case.SPECS.items():
    EP.JOBS["test_xl_device_code_on_the_host_equals_oracle_and_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.xl_case", json.dumps(_spec)], {}, 900, 30 if ("two_runs" in _name or "merged" in _name) else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(xl_case.SPECS))
def test_xl_device_code_on_the_host_equals_oracle_and_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    print(out[-4000:])
    assert rc == 0 and "XL_CASE_OK" in out, out[-3000:] + err[-3000:]
