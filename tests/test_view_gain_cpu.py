"""CPU tier of the view information gain (DESIGN.md, section "View information gain").
1. the NumPy model (tests/view_gain_model.py) on its own, before it judges anything: it equals an independent scalar restatement
   (plain Python loops, a set of voxel tuples per view, numpy.float32 scalars) on the random field; empty space, the closed room,
   the room with a door, two identical rays and a voxel with a NaN distance give what the contract says in closed form.  The stores
   are made by hand (frontier_case.hand_store): no library is needed;
2. the DEVICE CODE on the host functional model (tools/emu) against the model, byte for byte: one child process per case
   (tests/view_gain_case.py), started side by side like those of tests/test_emu_parity.py.
What fails without the feature is part 2, tests/test_view_gain_abi.py and tests/test_view_gain_gpu.py."""
import json
import sys

import numpy as np
import pytest

from tests import frontier_case as FC
from tests import view_gain_case as C
from tests import view_gain_model as M
from tests import test_emu_parity as EP

F = np.float32
VS = C.VOXEL


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------
def scalar_view(store, T, K, w, h, voxel_size, min_range_m=0.0, max_range_m=5.0, step_m=0.0, stop_distance_m=0.0, label=255):
    """One view, ray by ray and sample by sample: (record values (7,), per ray the list of (voxel, state) it visited)."""
    T = [F(v) for v in T]
    fx, fy, cx, cy = [F(v) for v in K]
    kx, ky = F(np.float64(1.0) / np.float64(fx)), F(np.float64(1.0) / np.float64(fy))
    inv = F(1.0 / np.float64(F(voxel_size)))
    rmin, rmax, stop = F(min_range_m), F(max_range_m), F(stop_distance_m)
    step = F(step_m) if F(step_m) > 0 else F(voxel_size)
    N = int(np.floor((rmax - rmin) / step)) + 1
    qw, qv, o = T[0], T[1:4], T[4:7]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    seen, rays = {}, []
    hits = opens = samples = 0
    lim = F((1 << 20) - 1)
    with np.errstate(all="ignore"):
        for v in range(h):
            for u in range(w):
                dcx, dcy = (F(u) - cx) * kx, (F(v) - cy) * ky
                ln = np.sqrt((dcx * dcx + dcy * dcy) + F(1))
                uc = [dcx / ln, dcy / ln, F(1) / ln]
                uv = cross(qv, uc)
                uv = [a + a for a in uv]
                c2 = cross(qv, uv)
                dg = [(uc[k] + qw * uv[k]) + c2[k] for k in range(3)]
                visited, hit = [], False
                for k in range(N):
                    t = rmin + F(k) * step
                    p = [o[a] + t * dg[a] for a in range(3)]
                    if not all(np.isfinite(x) for x in p):
                        break
                    c = [np.floor(x * inv + F(1e-6)) for x in p]
                    if not all(abs(x) < lim for x in c):
                        break
                    vox = tuple(int(x) for x in c)
                    d, fl, lb = store.records(np.array([vox], np.int64))
                    observed = bool(fl[0] & 1)
                    occupied = observed and not (d[0] > stop)
                    state = 0 if not observed else 1 if not occupied else 3 if (label != 255 and lb[0] == label) else 2
                    samples += 1
                    seen[vox] = state
                    visited.append((vox, state))
                    if occupied:
                        hit = True
                        break
                hits += hit
                opens += not hit
                rays.append(visited)
    states = list(seen.values())
    return [states.count(0), states.count(1), states.count(2) + states.count(3), states.count(3), hits, opens, samples], rays


def random_poses(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q = (q / np.linalg.norm(q, axis=1)[:, None]).astype(F)
    t = rng.uniform(-0.85, 0.85, (n, 3)).astype(F)
    t[-1] = [3.0, -2.0, 1.0]                                      # outside the field, looking wherever
    return np.concatenate([q, t], axis=1)


@pytest.mark.parametrize("vps", [8, 16])
def test_model_equals_a_scalar_restatement_on_the_random_field(vps):
    store = FC.hand_store(FC.random_voxels(), vps)
    store.label[...] = np.random.default_rng(5).integers(0, 3, store.label.shape)    # (a hand-made store: any label anywhere)
    poses = random_poses(20, 11)
    w, h = 4, 3
    K = C.K_of(w, h, 70.0)
    cfg = dict(min_range_m=0.1, max_range_m=1.3, stop_distance_m=0.0, label=1)
    rec, stats = M.view_gain(store, poses, K, VS, width=w, height=h, **cfg)
    for j, T in enumerate(poses):
        want, _ = scalar_view(store, T, K, w, h, VS, **cfg)
        assert [int(rec[k][j]) for k in M.COUNTERS] == want and rec["flags"][j] == M.VALID, (j, rec[j], want)
    assert stats["rays_hit"] > 50 and stats["rays_open"] > 5 and stats["unknown_voxels"] > 100 and stats["surface_voxels"] > stats["label_voxels"] > 10, stats
    # ... and with a stop distance that makes the voxels beside a wall surfaces, and a coarser step
    cfg = dict(max_range_m=1.0, step_m=0.08, stop_distance_m=VS)
    rec, stats = M.view_gain(store, poses[:6], K, VS, width=w, height=h, **cfg)
    for j, T in enumerate(poses[:6]):
        assert [int(rec[k][j]) for k in M.COUNTERS] == scalar_view(store, T, K, w, h, VS, **cfg)[0], j


def test_empty_space_counts_every_sample_as_a_new_unknown_voxel():
    store = FC.hand_store({(400 + x, 400, 400): FC.FREE for x in range(8)}, 8)
    T = C.pose(C.LOOK["+x"], C.centre(3, -2, 7))
    n = M.n_samples(VS)
    rec, stats = M.view_gain(store, [T], (500.0, 500.0, 0.0, 0.0), VS, width=1, height=1, step_m=VS)
    assert n == 101 and rec[0].tolist() == (n, 0, 0, 0, 0, 1, n, 1), rec
    assert stats["views_valid"] == 1 and stats["unknown_voxels"] == n and stats["box_bits"] == [n]


@pytest.mark.parametrize("vps", [8, 16])
def test_closed_room_shows_no_unknown_voxel_from_inside(vps):
    store = FC.hand_store(FC.room_voxels(False), vps)
    w, h = 9, 7
    poses = [C.pose(C.LOOK[d], C.centre(0, 0, 0)) for d in sorted(C.LOOK)] + [C.pose(C.GENERIC, C.centre(0, 0, 0))]
    rec, stats = M.view_gain(store, poses, C.K_of(w, h, 90.0), VS, width=w, height=h, max_range_m=1.0)
    assert (rec["unknown_voxels"] == 0).all() and (rec["rays_hit"] == w * h).all() and (rec["rays_open"] == 0).all(), rec
    assert (rec["surface_voxels"] > 0).all() and (rec["free_voxels"] > 0).all()


def test_room_with_a_door_shows_unknown_voxels_through_the_door_only():
    store = FC.hand_store(FC.room_voxels(True), 8)
    w, h = 9, 7
    K = C.K_of(w, h, 90.0)
    poses = [C.pose(C.LOOK[d], C.centre(0, 0, 0)) for d in ("+x", "-x", "+y", "-y", "+z", "-z")]
    rec, _ = M.view_gain(store, poses, K, VS, width=w, height=h, max_range_m=1.0)
    assert rec["unknown_voxels"][0] > 0 and (rec["unknown_voxels"][1:] == 0).all() and rec["rays_open"][0] > 0 and (rec["rays_open"][1:] == 0).all(), rec
    values, rays = scalar_view(store, poses[0], K, w, h, VS, max_range_m=1.0)
    assert values == [int(rec[k][0]) for k in M.COUNTERS]
    door = {(5, y, z) for y in (-1, 0) for z in (-1, 0)}
    n_through = 0
    for visited in rays:
        unknown = [v for v, s in visited if s == 0]
        if unknown:
            n_through += 1
            first = [v for v, _ in visited].index(unknown[0])
            assert all(v[0] >= 6 for v in unknown) and any(v in door for v, _ in visited[:first]), visited
    assert n_through == rec["rays_open"][0]


def test_identical_rays_count_their_voxels_once_and_their_samples_twice():
    store = FC.hand_store(FC.room_voxels(True), 8)
    T = C.pose(C.GENERIC, C.centre(1, -1, 0))
    one, _ = M.view_gain(store, [T], (500.0, 500.0, 0.0, 0.0), VS, width=1, height=1, max_range_m=1.0)
    two, _ = M.view_gain(store, [T], (1e30, 500.0, 0.0, 0.0), VS, width=2, height=1, max_range_m=1.0)
    a, b = M.ray_directions(np.array(T, F), (1e30, 500.0, 0.0, 0.0), 2, 1)
    assert (np.array(T, F)[4:7] + F(0.7) * a).tobytes() == (np.array(T, F)[4:7] + F(0.7) * b).tobytes()
    for k in ("unknown_voxels", "free_voxels", "surface_voxels", "label_voxels"):
        assert two[k][0] == one[k][0], k
    assert two["samples"][0] == 2 * one["samples"][0] > 0 and two["rays_hit"][0] + two["rays_open"][0] == 2
    assert one["free_voxels"][0] > 2


def test_a_nan_distance_stops_the_ray():
    vox = {(x, 0, 0): FC.FREE for x in range(0, 12)}
    vox[(6, 0, 0)] = (0, 1.0, float("nan"))
    store = FC.hand_store(vox, 8)
    d, flags, _ = store.records(np.array([(6, 0, 0)], np.int64))
    assert np.isnan(d[0]) and flags[0] == 1
    T = C.pose(C.LOOK["+x"], C.centre(0, 0, 0))
    rec, _ = M.view_gain(store, [T], (500.0, 500.0, 0.0, 0.0), VS, width=1, height=1, max_range_m=1.0)
    assert rec[0].tolist() == (0, 6, 1, 0, 1, 0, 7, 1), rec
    del vox[(6, 0, 0)]                                             # without it the ray runs on: 0 .. 11 free but 6, then unknown
    rec, _ = M.view_gain(FC.hand_store(vox, 8), [T], (500.0, 500.0, 0.0, 0.0), VS, width=1, height=1, max_range_m=1.0)
    assert rec[0].tolist() == (10, 11, 0, 0, 0, 1, 21, 1), rec


def test_sizing_rule_in_numbers():
    assert M.ball_bits(5.0, VS) == 203 ** 3 and M.ball_bits(6.4, VS) == 259 ** 3
    slab = ((203 ** 3 + 31) // 32 + 63) // 64 * 256
    assert M.workspace_bytes(10, 1024, 5.0, VS) == 10 * 256 + 96 + 512 * slab
    assert M.workspace_bytes(10, 3, 5.0, VS) == 10 * 256 + 96 + 3 * slab
    assert M.workspace_bytes(10, 1024, 5.0, VS, max_workspace_bytes=10 * 256 + 96 + 2 * slab + 1) == 10 * 256 + 96 + 2 * slab


# ---- 2. the device code on the functional model: one child per case, started together by test_emu_parity's fixture ----
for _name, _spec in C.SPECS.items():
    EP.JOBS["test_view_gain_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.view_gain_case", json.dumps(_spec)], {}, 900, 40 if _spec["case"] in ("in_flight", "errors", "reads_only") else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(C.SPECS))
def test_view_gain_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "VIEW_GAIN_CASE_OK" in out, out[-3000:] + err[-3000:]
