"""CPU tier of path shortening (DESIGN.md, section "Path shortening").
1. the NumPy model (tests/path_shorten_model.py) on its own, before it judges anything: it equals a scalar restatement of the contract
   on the scalar sweep of tests/test_esdf_read_cpu.py; in the open box every reached path of the navigation model comes out as its two
   ends; endpoints keep their bits, the output is a subsequence of the input, every emitted segment of an OK path is FREE when swept
   again, and the output is no longer than the input up to a rounding bound that the test derives;
2. the DEVICE CODE on the host functional model (tools/emu) against the model, byte for byte: one child process per case
   (tests/path_shorten_case.py), started side by side like those of tests/test_emu_parity.py; then, on what the MODEL gave in those
   cases, that the list exercises what it claims.
Part 1 needs no library.  What fails without the feature is part 2, tests/test_path_shorten_gpu.py and tests/test_path_shorten_abi.py."""
import json
import sys

import numpy as np
import pytest

from tests import esdf_read_model as E
from tests import nav_case
from tests import nav_model as NM
from tests import path_shorten_case
from tests import path_shorten_model as M
from tests import test_emu_parity as EP
from tests import test_esdf_read_cpu as R
from tests import test_nav_cpu as N

F = np.float32
VS = nav_case.VOXEL
U = 2.0 ** -24                   # the unit roundoff of f32


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _walks(seed, lengths, mw):
    """Random walks of 5 cm steps through the box of R._random_store, with a repeated waypoint each."""
    rng = np.random.default_rng(seed)
    paths = []
    for m in lengths:
        d = rng.normal(size=(m, 3))
        p = np.clip(rng.uniform(-0.9, 0.4, 3) + np.cumsum(d / np.linalg.norm(d, axis=1, keepdims=True) * 0.05, axis=0), -0.95, 0.5)
        if m > 3:
            p[m // 2] = p[m // 2 - 1]
        paths.append(p.astype(F))
    wp, nw = path_shorten_case.pack(paths, mw)
    return wp, nw


def _scalar_shorten(blocks, vps, P, m, mw, cfg):
    """One path, rule by rule: (status, Q, length, min_clearance, sweeps, samples, unverified segments)."""
    c = dict(M.DEFAULTS, **cfg)
    inv = E.inv_of(VS)
    min_step = F(c["min_step_m"]) if c["min_step_m"] > 0 else F(0.5) * F(VS)
    sw = lambda a, b: R._scalar_sweep(blocks, vps, np.concatenate([a, b]), inv, F(c["radius_m"]), min_step, c["unknown_is_free"], c["max_samples"])
    if m == 0 or m > mw or not np.isfinite(P[:m]).all():
        return M.INVALID, [], F(0), M.INF, 0, 0, 0
    status, Q, length, min_c, a, sweeps, samples, unverified = M.OK, [P[0]], F(0), M.INF, 0, 0, 0, 0
    while a < m - 1:
        hi = min(a + c["lookahead"], m - 1)
        j_star, chunk = None, 0
        while j_star is None and hi - 64 * chunk >= a + 1:
            res = {}
            for j in range(max(a + 1, hi - 64 * chunk - 63), hi - 64 * chunk + 1):
                res[j] = sw(P[a], P[j])
                sweeps += 1
                samples += res[j][4]
            free = [j for j in res if res[j][0] == E.FREE]
            if free:
                j_star = max(free)
            chunk += 1
        if j_star is None:
            j_star, status = a + 1, M.UNVERIFIED
            unverified += 1
        Q.append(P[j_star])
        with np.errstate(over="ignore"):
            d = [F(q - p) for p, q in zip(P[a], P[j_star])]
            length = F(length + F(np.sqrt(F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2])))))
        mc = res[j_star][2]
        if mc < min_c:
            min_c = mc
        a = j_star
    return status, Q, length, min_c, sweeps, samples, unverified


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(radius_m=0.05, lookahead=1), dict(radius_m=0.05, lookahead=5, unknown_is_free=1),
                                 dict(radius_m=0.0, lookahead=70, min_step_m=0.01, max_samples=40), dict(radius_m=0.02, lookahead=130, unknown_is_free=1)])
def test_model_equals_a_scalar_restatement(cfg):
    store, blocks, vps = R._random_store()
    wp, nw = _walks(5, (1, 2, 5, 30, 66, 140, 9, 9, 0, 4), 140)
    wp[6, 4, 1] = np.nan          # a used row
    wp[7, 9:] = np.nan            # rows that are not used
    nw[9] = 141                   # m > max_waypoints
    got = M.shorten(store, wp, nw, VS, **cfg)
    assert list(got["status"][[6, 8, 9]]) == [M.INVALID] * 3 and got["status"][7] != M.INVALID
    totals = dict.fromkeys(("sweeps", "samples", "segments_unverified"), 0)
    for i in range(len(nw)):
        status, Q, length, min_c, sweeps, samples, unverified = _scalar_shorten(blocks, vps, wp[i], int(nw[i]), 140, cfg)
        assert (status, len(Q)) == (got["status"][i], got["n_waypoints"][i]), (cfg, i)
        assert _bits(np.array(Q, F).reshape(-1, 3)) == _bits(got["waypoints"][i, :len(Q)]) and (got["waypoints"][i, len(Q):] == M.WAYPOINT_FILL).all(), (cfg, i)
        assert _bits(F(length)) == _bits(got["length"][i]) and _bits(F(min_c)) == _bits(got["min_clearance"][i]), (cfg, i, length, got["length"][i])
        for k, v in zip(("sweeps", "samples", "segments_unverified"), (sweeps, samples, unverified)):
            totals[k] += v
    assert totals == {k: got["stats"][k] for k in totals}, (totals, got["stats"])
    assert got["stats"]["paths_invalid"] == 3 and got["stats"]["waypoints_in"] == int(nw[[0, 1, 2, 3, 4, 5, 7]].sum())
    assert got["stats"]["paths_ok"] + got["stats"]["paths_unverified"] == 7


@pytest.mark.parametrize("vps", [8, 16])
def test_open_box_paths_come_out_as_their_two_ends(vps):
    vox = nav_case.open_box_voxels()
    store = N.store_of_voxels(vox, vps)
    fld = NM.field(store, N.centres([nav_case.OPEN_BOX_GOAL]), VS)
    rng = np.random.default_rng(2)
    starts = N.centres(np.array(vox)[rng.choice(len(vox), 60, replace=False)])
    nav = NM.paths(fld, starts, 64)
    assert (nav["status"] == NM.REACHED).all() and nav["n_waypoints"].max() > 10
    out = M.shorten(store, nav["waypoints"], nav["n_waypoints"], VS, radius_m=0.3, lookahead=63)
    assert (out["status"] == M.OK).all() and (out["n_waypoints"] == np.minimum(nav["n_waypoints"], 2)).all()
    ends = nav["waypoints"][np.arange(60), nav["n_waypoints"] - 1]
    assert _bits(out["waypoints"][:, 0]) == _bits(nav["waypoints"][:, 0]) and _bits(out["waypoints"][nav["n_waypoints"] > 1, 1]) == _bits(ends[nav["n_waypoints"] > 1])
    # lookahead 1 with every adjacent segment free: the identity
    same = M.shorten(store, nav["waypoints"], nav["n_waypoints"], VS, radius_m=0.3, lookahead=1)
    assert _bits(same["waypoints"]) == _bits(nav["waypoints"]) and (same["n_waypoints"] == nav["n_waypoints"]).all() and (same["status"] == M.OK).all()


@pytest.mark.parametrize("cfg", [dict(radius_m=0.02, lookahead=16, unknown_is_free=1), dict(radius_m=0.0, lookahead=100, unknown_is_free=1),
                                 dict(radius_m=0.05, lookahead=7)])
def test_invariants(cfg):
    store, _, _ = R._random_store(seed=4)
    lengths = (1, 2, 3, 17, 64, 65, 120, 120, 120, 40)
    wp, nw = _walks(8, lengths, 120)
    out = M.shorten(store, wp, nw, VS, **cfg)
    assert (out["status"] != M.INVALID).all() and (out["status"] == M.OK).any() and (out["n_waypoints"] < nw).any()
    for i, m in enumerate(lengths):
        k = int(out["n_waypoints"][i])
        Q, steps = out["waypoints"][i, :k], out["trace"][i]
        # endpoints keep their bits; Q is the subsequence of P that the trace names
        assert _bits(Q[0]) == _bits(wp[i, 0]) and _bits(Q[-1]) == _bits(wp[i, m - 1])
        picks = [0] + [s[1] for s in steps]
        assert len(picks) == k and all(b > a for a, b in zip(picks, picks[1:])) and _bits(Q) == _bits(wp[i, picks])
        assert all(a == prev for (a, _, _, _, _), prev in zip(steps, picks))
        if out["status"][i] == M.OK and k > 1:
            again = E.sweep(store, np.concatenate([Q[:-1], Q[1:]], axis=1), VS, **{f: v for f, v in cfg.items() if f != "lookahead"})
            assert (again["status"] == E.FREE).all()
            assert _bits(again["min_clearance"].min()) == _bits(out["min_clearance"][i])
        # the length.  Exactly, |Q[k] - Q[k+1]| <= the sum of the input segments between them (the triangle inequality), so the exact
        # sums obey out <= in.  In f32: a length is three differences, three squares, two sums and a root, at most (1 + u)^5 under the
        # root and (1 + u)^3.5 after it: L^ = L (1 + t), |t| <= (1 + u)^4 - 1 (nothing underflows: the steps are 5 cm).  A sum of n
        # terms from the left multiplies each by at most (1 + u)^(n - 1) and at least (1 - u)^(n - 1).  With K = k - 1 output and
        # m - 1 input segments: out^ <= (1 + u)^(K + 3) * exact_out <= (1 + u)^(K + 3) * exact_in <= (1 + u)^(K + 3) / (1 - u)^(m + 2) * in^.
        length_in = F(0)
        for L in M.length_of(wp[i, :m - 1], wp[i, 1:m]):
            length_in = F(length_in + L)
        bound = float(length_in) * ((1 + U) ** (k - 1 + 3) / (1 - U) ** (m + 2) - 1)
        assert float(out["length"][i]) <= float(length_in) + bound, (i, out["length"][i], length_in, bound)


# ---- 2. the device code on the functional model: one child per case, started together by test_emu_parity's fixture ----
for _name, (_spec, _env) in path_shorten_case.SPECS.items():
    EP.JOBS["test_path_shorten_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.path_shorten_case", json.dumps(_spec)], dict(_env), 900, 40 if _spec["case"] in ("many", "reads_only", "errors") else 10)

emu_jobs = EP.emu_jobs


def _result(emu_jobs, name):
    rc, out, err = emu_jobs.result("test_path_shorten_device_code_on_the_host_equals_model[%s]" % name)
    assert rc == 0 and "PATH_SHORTEN_CASE_OK" in out, out[-3000:] + err[-3000:]
    return json.loads(out[out.index("PATH_SHORTEN_CASE_OK") + len("PATH_SHORTEN_CASE_OK"):].strip().splitlines()[0])


@pytest.mark.parametrize("name", sorted(path_shorten_case.SPECS))
def test_path_shorten_device_code_on_the_host_equals_model(emu_jobs, request, name):
    _result(emu_jobs, name)


def test_the_cases_exercise_what_they_claim(emu_jobs):
    """On the model's own output, as the cases report it: a shortened path, an UNVERIFIED one, an INVALID one, a j* that is not in
    chunk 0, and a j* with a nearer candidate that is not free."""
    total = {}
    for name in path_shorten_case.SPECS:
        for k, v in _result(emu_jobs, name).items():
            total[k] = total.get(k, 0) + v
    for k in ("shortened", "paths_unverified", "paths_invalid", "late_chunk", "nearer_blocked", "paths_ok", "segments_unverified"):
        assert total[k] > 0, (k, total)
