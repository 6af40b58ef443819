"""CPU tier of the ESDF reads (DESIGN.md, section "ESDF reads"): the yardstick against a scalar restatement of the contract and
against an analytic plane, the DEVICE CODE and the host code of the six entries on the host functional model (tools/emu) against the
yardstick, bit for bit — one child process per case (tests/esdf_read_case.py), started side by side like those of
tests/test_esdf_cpu.py — and the new symbols and struct sizes through the binding."""
import ctypes
import json
import sys

import numpy as np
import pytest

from tests import esdf_read_case
from tests import esdf_read_model as M
from tests import test_emu_parity as EP

F = np.float32
VS = 0.05

for _name, (_spec, _env) in esdf_read_case.SPECS.items():
    EP.JOBS["test_esdf_read_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.esdf_read_case", json.dumps(_spec)], dict(_env), 900, 30 if _spec["case"] == "reads_only" else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(esdf_read_case.SPECS))
def test_esdf_read_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "ESDF_READ_CASE_OK" in out, out[-3000:] + err[-3000:]


def test_esdf_read_symbols_and_struct_sizes():
    from kimera_semantics_amd import binding as B
    for sym in ("ks_esdf_sample", "ks_esdf_sample_device", "ks_esdf_slice", "ks_esdf_slice_device", "ks_esdf_sweep_default_config",
                "ks_esdf_sweep", "ks_esdf_sweep_device"):
        assert sym in B.ABI_SYMBOLS and hasattr(B.lib(), sym), sym
    assert ctypes.sizeof(B.KsEsdfSampleStats) == 24 and ctypes.sizeof(B.KsEsdfSweepConfig) == 16 and ctypes.sizeof(B.KsEsdfSweepStats) == 40
    for name in ("esdf_sample", "esdf_slice", "esdf_sweep", "esdf_sample_device", "esdf_slice_device", "esdf_sweep_device"):
        assert callable(getattr(B.HipIntegrator, name)), name


# ---- the yardstick itself --------------------------------------------------------------------------------------------------------
def _random_store(seed=1, vps=8):
    """3 x 2 x 2 blocks around the origin, one of them absent, a tenth of the voxels unobserved, distances in +-0.4."""
    from kimera_semantics_amd import binding as B
    rng = np.random.default_rng(seed)
    idx = np.array([(x, y, z) for x in (-2, -1, 0) for y in (-1, 0) for z in (-1, 0)], np.int32)
    idx = idx[np.arange(len(idx)) != 5]
    rec = np.zeros((len(idx), vps ** 3), B.ESDF_DTYPE)
    rec["distance"] = rng.uniform(-0.4, 0.4, rec.shape).astype(F)
    rec["flags"] = np.where(rng.random(rec.shape) < 0.1, 0, rng.choice([1, 3], rec.shape)).astype(np.uint8)
    rec["label"] = rng.integers(0, 21, rec.shape).astype(np.uint8)
    hidden = rec["flags"] == 0
    rec["distance"][hidden], rec["label"][hidden] = 0, 255
    return M.Store(idx, rec, vps), {tuple(int(v) for v in b): rec[j] for j, b in enumerate(idx)}, vps


def _scalar_record(blocks, vps, v):
    """The record of voxel v (three Python ints) from the blocks as a dict: (distance, flags, label)."""
    b = tuple(c // vps for c in v)
    if b not in blocks:
        return F(0), 0, 255
    x, y, z = (c % vps for c in v)
    r = blocks[b][x + vps * (y + vps * z)]
    return F(r["distance"]), int(r["flags"]), int(r["label"])


def _scalar_sample(blocks, vps, p, inv):
    """E(p) of one point, rule by rule ("ESDF reads")."""
    unknown = (0, M.NAN, (F(0), F(0), F(0)), 255, 0)
    lim = float((1 << 20) - 1)
    if not all(np.isfinite(c) for c in p):
        return unknown
    with np.errstate(over="ignore", invalid="ignore"):
        g = [F(F(c * inv) - F(0.5)) for c in p]
    i = [F(np.floor(c)) for c in g]
    if not all(abs(float(c)) < lim and abs(float(F(c + F(1)))) < lim for c in i):
        return unknown
    f = [F(a - b) for a, b in zip(g, i)]
    d, observed = [], True
    for j in range(8):
        dist, flags, _ = _scalar_record(blocks, vps, (int(i[0]) + (j & 1), int(i[1]) + ((j >> 1) & 1), int(i[2]) + (j >> 2)))
        d.append(dist)
        observed = observed and bool(flags & 1)
    n = [F(np.floor(F(F(c * inv) + F(1e-6)))) for c in p]
    own = _scalar_record(blocks, vps, tuple(int(c) for c in n)) if all(abs(float(c)) < lim for c in n) else (F(0), 0, 255)
    lerp = lambda a, b, t: F(a + F(t * F(b - a)))
    if observed:
        fx, fy, fz = f
        value = lerp(lerp(lerp(d[0], d[1], fx), lerp(d[2], d[3], fx), fy), lerp(lerp(d[4], d[5], fx), lerp(d[6], d[7], fx), fy), fz)
        gx = F(lerp(lerp(F(d[1] - d[0]), F(d[3] - d[2]), fy), lerp(F(d[5] - d[4]), F(d[7] - d[6]), fy), fz) * inv)
        gy = F(lerp(lerp(F(d[2] - d[0]), F(d[3] - d[1]), fx), lerp(F(d[6] - d[4]), F(d[7] - d[5]), fx), fz) * inv)
        gz = F(lerp(lerp(F(d[4] - d[0]), F(d[5] - d[1]), fx), lerp(F(d[6] - d[2]), F(d[7] - d[3]), fx), fy) * inv)
        return 2, value, (gx, gy, gz), own[2], own[1]
    if own[1] & 1:
        return 1, own[0], (F(0), F(0), F(0)), own[2], own[1]
    return unknown


def _scalar_sweep(blocks, vps, seg, inv, radius, min_step, unknown_is_free, max_samples):
    """One segment -> (status, t_stop, min_clearance, t_min, samples)."""
    a, b = seg[:3], seg[3:]
    invalid = (M.INVALID, F(0), M.INF, F(0))
    with np.errstate(over="ignore", invalid="ignore"):
        d = [F(q - p) for p, q in zip(a, b)]
        L = F(np.sqrt(F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))))
    if not (all(np.isfinite(c) for c in seg) and np.isfinite(L)) or L > F(F(max_samples - 2) * min_step):
        return invalid + (0,)
    u = [F(0)] * 3 if L == 0 else [F(c / L) for c in d]
    t, min_c, t_min, samples = F(0), M.INF, F(0), 0
    for _ in range(max_samples):
        st, dist = _scalar_sample(blocks, vps, [F(p + F(t * q)) for p, q in zip(a, u)], inv)[:2]
        samples += 1
        if st == 0 and not unknown_is_free:
            return M.UNKNOWN, t, min_c, t_min, samples
        c = F(0)
        if st != 0:
            c = F(dist - radius)
            if c < min_c:
                min_c, t_min = c, t
            if c < 0:
                return M.COLLISION, t, min_c, t_min, samples
        if t >= L:
            return M.FREE, L, min_c, t_min, samples
        step = (c if c > min_step else min_step) if st != 0 else min_step
        t = F(min(F(t + step), L))
    return invalid + (samples,)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_vectorised_model_equals_a_scalar_restatement():
    store, blocks, vps = _random_store()
    inv = M.inv_of(VS)
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-0.95, 0.5, (500, 3)).astype(F)
    xyz[:6] = [[0.0, 0.0, 0.0], [-0.0, 0.025, -0.025], [6e4, 0, 0], [np.nan, 0, 0], [0, -np.inf, 0], [52428.75, 0.1, 0.1]]
    got = M.sample(store, xyz, VS)
    assert min(got["stats"].values()) > 25, got["stats"]
    for k, p in enumerate(xyz):
        st, dist, grad, label, flags = _scalar_sample(blocks, vps, p, inv)
        assert (st, label, flags) == (got["status"][k], got["label"][k], got["flags"][k]), (k, p)
        assert _bits(F(dist)) == _bits(got["distance"][k]) and _bits(np.array(grad, F)) == _bits(got["gradient"][k]), (k, p, dist, grad)
    a = rng.uniform(-0.9, 0.45, (100, 3))
    d = rng.normal(size=(100, 3))
    seg = np.concatenate([a, a + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, 0.8, (100, 1))], axis=1).astype(F)
    seg[0, 3:] = seg[0, :3]
    seg[1, 4], seg[2, 0] = np.nan, np.inf
    seg[3, 3:] = seg[3, :3] + F(3.0)
    for cfg in (dict(radius_m=0.05), dict(radius_m=0.05, unknown_is_free=1), dict(radius_m=0.0, min_step_m=0.01, max_samples=40),
                dict(radius_m=0.02, unknown_is_free=1, min_step_m=0.004, max_samples=65)):
        c = dict(M.SWEEP_DEFAULTS, **cfg)
        got = M.sweep(store, seg, VS, **cfg)
        min_step = F(c["min_step_m"]) if c["min_step_m"] > 0 else F(0.5) * F(VS)
        samples = 0
        for k, s in enumerate(seg):
            st, t_stop, min_c, t_min, n = _scalar_sweep(blocks, vps, s, inv, F(c["radius_m"]), min_step, c["unknown_is_free"], c["max_samples"])
            samples += n
            assert st == got["status"][k], (cfg, k, st, got["status"][k])
            assert (_bits(F(t_stop)), _bits(F(min_c)), _bits(F(t_min))) == (_bits(got["t_stop"][k]), _bits(got["min_clearance"][k]), _bits(got["t_min"][k])), (cfg, k)
        assert samples == got["stats"]["samples"]
        assert len(set(got["status"])) >= 3, (cfg, got["stats"])


def test_plane_gives_its_distance_and_a_unit_gradient_within_the_rounding_bound():
    """vs is the context's f32 voxel size.  The store holds d(k_z) = f32((k_z + 0.5) vs - c0): a plane with unit gradient along z.  The corners of a cell hold a = d(i_z) four
    times and b = d(i_z + 1) four times, so every lerp along x and y is a + f * (a - a) = a exactly: gradient.x = gradient.y = +0
    exactly, gradient.z = fl(fl(b - a) * inv) and distance = fl(a + fl(fz * fl(b - a))).  With u = 2^-24, D = max |d| and P = max |p_z|:
      gradient.z  a, b carry u |d| each and b - a = vs before rounding: |fl(b - a) - vs| <= u (2 D + vs); inv = fl(1 / vs) and the
                  product add u each: |gradient.z - 1| <= u (2 D / vs + 3), and one more u for the terms of second order.
      distance    g = fl(fl(p inv) - 0.5) is off its exact value by at most 3 u |p| / vs (inv, the product, the subtraction), which
                  moves the value by 3 u P (the plane is the same line in every cell, so a g that rounds across a cell face costs no
                  more); a: u D; fl(b - a): u (2 D + vs); the product with fz < 1: u vs; the last addition: u D.  In all
                  |distance - (p_z - c0)| <= u (3 P + 4 D + 2 vs), and one more u D for the terms of second order.
    Nothing here is fitted to the model's output."""
    from kimera_semantics_amd import binding as B
    vps, c0, u = 8, 0.1234, 2.0 ** -24
    vs = float(F(VS))
    idx = np.array([(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)], np.int32)
    lin = np.arange(vps ** 3)
    rec = np.zeros((len(idx), vps ** 3), B.ESDF_DTYPE)
    kz = idx[:, 2:3].astype(np.int64) * vps + (lin // (vps * vps))[None]
    rec["distance"] = ((kz + 0.5) * vs - c0).astype(F)
    rec["flags"], rec["label"] = 1, 5
    store = M.Store(idx, rec, vps)
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-0.45, 0.45, (4000, 3)).astype(F)
    got = M.sample(store, xyz, VS)
    inside = got["status"] == 2
    assert inside.sum() > 2000 and (got["status"] == 1).sum() > 100   # (cells inside the box: 0.75^3 / 0.9^3 of the points)
    g = got["gradient"][inside]
    assert (g[:, 0] == 0).all() and (g[:, 1] == 0).all()
    D, P = float(np.abs(rec["distance"]).max()), float(np.abs(xyz[inside, 2]).max())
    bound_g, bound_d = u * (2 * D / vs + 4), u * (3 * P + 5 * D + 2 * vs)
    err_g = np.abs(g[:, 2].astype(np.float64) - 1.0).max()
    err_d = np.abs(got["distance"][inside].astype(np.float64) - (xyz[inside, 2].astype(np.float64) - c0)).max()
    print("gradient.z: %.3g (bound %.3g); distance: %.3g (bound %.3g)" % (err_g, bound_g, err_d, bound_d))
    assert err_g <= bound_g and err_d <= bound_d
    assert (got["label"][inside] == 5).all() and (got["flags"][inside] == 1).all()
