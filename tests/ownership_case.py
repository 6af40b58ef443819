"""Who owns what on the host side of the library (csrc/ks_owned.h), checked against the ledger of the functional model's runtime
stand-in (tools/emu/README.md: live hipMalloc + hipHostMalloc blocks, their bytes, live events, live streams) and its failure
injection (the k-th allocation from now on fails).  One child process per case of tests/test_ownership_emu.py:
KS_HIP_LIB=tools/emu/_build/libks_hip_emu.so python -m tests.ownership_case '<json spec>'.

{"balance": name}: use a context, destroy it, the ledger is what it was before ks_create.
{"sweep": name}:   fail every allocation of a call, one per attempt, every index, no sampling (see the sweep_* functions)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np


def _lib():
    from kimera_semantics_amd import binding as B
    L = B.lib()
    L.ks_emu_ledger.argtypes = [C.POINTER(C.c_longlong)]
    L.ks_emu_ledger.restype = None
    L.ks_emu_fail_alloc.argtypes = [C.c_longlong]
    return L


def ledger():
    """(live blocks, live bytes, live events, live streams), allocations made so far"""
    out = (C.c_longlong * 5)()
    _lib().ks_emu_ledger(out)
    return tuple(out[:4]), int(out[4])


def arm(k):
    _lib().ks_emu_fail_alloc(k)


def disarm():
    """True if the failure armed before has fired."""
    return _lib().ks_emu_fail_alloc(-1) == 0


def frames(count, w=64, h=48, n=None, first=0):
    from kimera_semantics_amd import synth
    sc = synth.make_scene("room")
    out = []
    for i in range(first, first + count):
        f = synth.render_frame(sc, synth.trajectory_pose(5 * i), w, h, seed=40 + i)
        m = len(f.xyz) if n is None else n
        assert len(f.xyz) >= m
        out.append((f.T_G_C, f.xyz[:m].copy(), f.rgba[:m].copy(), f.labels[:m].copy()))
    return out


def config(**kw):
    from kimera_semantics_amd import binding as B
    from tests.util import COMMON
    base = dict(COMMON, method=0, max_tiles=4096, max_points=4096, pipeline_frames=0)
    base.update(kw)
    return B.default_config(**base)


def feed(g, fr):
    for T, xyz, rgba, labels in fr:
        g.integrate(T, xyz, rgba, labels)


# ---- balance ------------------------------------------------------------------------------------------------------------
def _integrate_and_read(cfg, n_frames=3):
    from kimera_semantics_amd import binding as B
    g = B.HipIntegrator(cfg)
    feed(g, frames(n_frames))
    g.flush()
    idx, _, _ = g.download()
    assert len(idx) > 4
    return g


def balance_fast_default():
    return _integrate_and_read(config())


def balance_fast_pipelined():
    return _integrate_and_read(config(pipeline_frames=8), n_frames=10)


def balance_fast_phased():
    return _integrate_and_read(config(early_out_phase_growth=32))


def balance_merged_reference():
    return _integrate_and_read(config(method=1, bundle_order=0))


def balance_merged_anti_grazing():
    return _integrate_and_read(config(method=1, enable_anti_grazing=1))


def balance_grow_points():
    from kimera_semantics_amd import binding as B
    g = B.HipIntegrator(config(max_points=1024))
    feed(g, frames(1, n=1000))
    feed(g, frames(2, first=1))   # ~3000 points each: ensure_points grows
    assert len(g.block_indices()) > 4
    return g


def balance_grow_pool():
    from kimera_semantics_amd import binding as B
    g = B.HipIntegrator(config(max_tiles=1024))
    feed(g, frames(4))            # ~450 tiles, then ~120 more per frame: more than half the pool in use -> grow_pool between frames
    assert len(g.tile_keys()) > 512, len(g.tile_keys())
    idx = np.array([[40 + i, 0, 0] for i in range(40)], np.int32)   # 320 more tiles in one call (grow_pool inside insert_tiles)
    g.upload(idx, tsdf=np.zeros((40, 16 ** 3), B.TSDF_DTYPE))
    assert len(g.tile_keys()) > 1024, len(g.tile_keys())   # more than the pool held when it was created
    return g


def balance_mesh():
    from kimera_semantics_amd import binding as B
    g = B.HipIntegrator(config())
    feed(g, frames(2))
    m = g.mesh()
    assert len(m.xyz) > 0
    feed(g, frames(1, first=2))
    m2 = g.mesh(only_stale=True)
    assert len(m2.xyz) > 0 and m2.stats["blocks_meshed"] > 0
    return g


def balance_block_io():
    from kimera_semantics_amd import binding as B
    g = B.HipIntegrator(config())
    feed(g, frames(2))
    idx, t, s = g.download()
    v = g.download_updated_voxels()
    assert len(v) > 0
    h = B.HipIntegrator(config())
    h.upload(idx, tsdf=t, sem=s)
    idx2, t2, s2 = h.download(idx)
    assert t2.tobytes() == t.tobytes() and s2.tobytes() == s.tobytes()
    h.close()
    return g


def balance_clear_mid_stream():
    from kimera_semantics_amd import binding as B
    g = B.HipIntegrator(config(pipeline_frames=4))
    fr = frames(6)
    feed(g, fr[:3])
    g.clear()                 # frames in flight are dropped with the map
    feed(g, fr[3:5])
    g.clear_voxels()          # frames in flight are completed first
    feed(g, fr[5:])
    g.flush()
    assert len(g.block_indices()) > 0
    return g


def balance_radix_sort():
    from kimera_semantics_amd import binding as B
    g = B.HipIntegrator(config())
    rng = np.random.default_rng(3)
    for dt in (np.uint32, np.uint64):
        k = rng.integers(0, 1 << 30, size=5000).astype(dt)
        v = np.arange(5000, dtype=np.uint32)
        ks, vs = g.debug_radix_sort(k, v)
        assert (ks == np.sort(k)).all() and (k[vs] == ks).all()
        ks, _ = g.debug_radix_sort(k)
        assert (ks == np.sort(k)).all()
    return g


def _balance_round_exact(method):
    from kimera_semantics_amd import binding as B
    marcher, owner = B.HipIntegrator(config(method=method)), B.HipIntegrator(config(method=method))
    for i, (T, xyz, rgba, labels) in enumerate(frames(2)):
        st = owner.integrate_round_exact(marcher, None, 0, 1, i, T, xyz, rgba, labels)
        assert st["updates_applied"] == st["updates_marched"] > 0
    assert len(owner.block_indices()) > 4
    marcher.close()
    return owner


def balance_round_exact_fast():
    return _balance_round_exact(0)


def balance_round_exact_merged():
    return _balance_round_exact(1)


def run_balance(name):
    before, _ = ledger()
    g = globals()["balance_" + name]()
    during, _ = ledger()
    assert during[0] > before[0] and during[3] > before[3], (before, during)   # (the ledger sees the context)
    g.close()
    after, _ = ledger()
    assert after == before, "ledger after ks_destroy %r != before ks_create %r" % (after, before)
    return {"live_during": during}


# ---- failure paths --------------------------------------------------------------------------------------------------------
def sweep_create(cfg):
    """Every allocation of ks_create fails once: an error code, a text, and nothing left behind."""
    from kimera_semantics_amd import binding as B
    L = _lib()
    before, a0 = ledger()
    h = C.c_void_p()
    assert L.ks_create(C.byref(cfg), C.byref(h)) == 0
    n = ledger()[1] - a0
    L.ks_destroy(h)
    assert ledger()[0] == before
    assert n > 20, n
    for k in range(n):
        arm(k)
        h = C.c_void_p()
        rc = L.ks_create(C.byref(cfg), C.byref(h))
        assert disarm(), "allocation %d of %d was never made" % (k, n)
        assert rc != 0, "ks_create succeeded although allocation %d of %d failed" % (k, n)
        assert L.ks_last_error(None), k
        assert ledger()[0] == before, "allocation %d of %d failed: ledger %r, baseline %r" % (k, n, ledger()[0], before)
    return {"allocations": n}


def sweep_create_fast():
    return sweep_create(config(max_tiles=64, max_points=1024))


def sweep_create_merged():
    return sweep_create(config(method=1, max_tiles=64, max_points=1024))


def sweep_create_pipelined():
    return sweep_create(config(max_tiles=64, max_points=1024, pipeline_frames=8))


def _sweep_live(make, call, result, repeat=True, must_fail=True):
    """make() -> a live context; call(g) the call under test; result(g) what it leaves (compared with ==).  Per allocation k of
    the call: a fresh context, the k-th allocation fails, the call returns an error (no crash); repeated without injection it
    succeeds with the result of a context that never failed; ks_destroy balances the ledger."""
    from kimera_semantics_amd import binding as B
    before, _ = ledger()
    g = make()
    a0 = ledger()[1]
    call(g)
    n = ledger()[1] - a0
    want = result(g)
    g.close()
    assert ledger()[0] == before
    assert n > 0
    failed = 0
    for k in range(n):
        g = make()
        arm(k)
        try:
            call(g)
        except B.KsError as e:
            failed += 1
            assert e.code != 0 and str(e)
        else:
            assert not must_fail, "the call succeeded although its allocation %d of %d failed" % (k, n)
        assert disarm(), "allocation %d of %d was never made" % (k, n)
        if repeat:
            call(g)
            got = result(g)
            assert got == want, "allocation %d of %d failed, the call was repeated: another result than on a context that never failed" % (k, n)
        g.close()
        assert ledger()[0] == before, "allocation %d of %d failed: ledger after ks_destroy %r, baseline %r" % (k, n, ledger()[0], before)
    return {"allocations": n, "failed_calls": failed}


def _map_bytes(g):
    idx, t, s = g.download()
    return idx.tobytes(), t.tobytes(), s.tobytes()


def sweep_upload():
    from kimera_semantics_amd import binding as B
    src = B.HipIntegrator(config())
    feed(src, frames(2))
    idx, t, s = src.download()
    src.close()

    def make():
        g = B.HipIntegrator(config())
        feed(g, frames(1, first=3))
        return g
    return _sweep_live(make, lambda g: g.upload(idx, tsdf=t, sem=s), _map_bytes)


def sweep_upload_growing_pool():
    """The same through grow_pool (insert_tiles).  Its FIRST allocation may fail without an error, by design (no room for a
    bigger pool: the map goes on with the one it has); whatever happens, nothing crashes and nothing is left behind."""
    from kimera_semantics_amd import binding as B
    idx = np.array([[40 + i, 0, 0] for i in range(40)], np.int32)
    t = np.zeros((40, 16 ** 3), B.TSDF_DTYPE)
    return _sweep_live(lambda: B.HipIntegrator(config(max_tiles=64)), lambda g: g.upload(idx, tsdf=t), lambda g: None, repeat=False, must_fail=False)


def sweep_mesh():
    from kimera_semantics_amd import binding as B

    def make():
        g = B.HipIntegrator(config())
        feed(g, frames(1))
        g.mesh()                      # (the scratch and an arena exist: the call under test GROWS them)
        feed(g, frames(2, first=1))
        return g

    def result(g):
        m = g.mesh()   # (a full mesh of the same map: what the call under test must have left, too)
        return m.blocks.tobytes(), m.xyz.tobytes(), m.normals.tobytes(), m.rgba.tobytes(), m.labels.tobytes()
    return _sweep_live(make, lambda g: g.mesh(), result)


def sweep_mesh_first():
    """... and of the FIRST call on a map, which allocates all of the scratch and an arena."""
    from kimera_semantics_amd import binding as B

    def make():
        g = B.HipIntegrator(config())
        feed(g, frames(1))
        return g

    def result(g):
        m = g.mesh()
        return m.blocks.tobytes(), m.xyz.tobytes(), m.normals.tobytes(), m.rgba.tobytes(), m.labels.tobytes()
    return _sweep_live(make, lambda g: g.mesh(), result)


def sweep_grow_points():
    """A cloud that outgrows max_points, every allocation of that call: an error, no crash, a clean ks_destroy.  (Not repeated:
    an allocation that fails after the frame's bookkeeping has advanced leaves a context one call further than its twin.)"""
    from kimera_semantics_amd import binding as B
    big = frames(1, first=1)

    def make():
        g = B.HipIntegrator(config(max_points=1024))
        feed(g, frames(1, n=1000))
        return g
    return _sweep_live(make, lambda g: feed(g, big), lambda g: None, repeat=False)


def sweep_radix_sort():
    from kimera_semantics_amd import binding as B
    k = np.random.default_rng(5).integers(0, 1 << 40, size=3000).astype(np.uint64)
    v = np.arange(3000, dtype=np.uint32)
    out = {}

    def call(g):
        ks, vs = g.debug_radix_sort(k, v)
        out["r"] = (ks.tobytes(), vs.tobytes())
    return _sweep_live(lambda: B.HipIntegrator(config(max_tiles=64, max_points=1024)), call, lambda g: out["r"])


def main():
    spec = json.loads(sys.argv[1])
    assert os.environ.get("KS_HIP_LIB", "").endswith("libks_hip_emu.so"), "this script drives the functional model only"
    t0 = time.time()
    rep = run_balance(spec["balance"]) if "balance" in spec else globals()["sweep_" + spec["sweep"]]()
    rep["seconds"] = round(time.time() - t0, 1)
    print("OWNERSHIP_OK", json.dumps(rep))


if __name__ == "__main__":
    main()
