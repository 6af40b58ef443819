"""The view-rendering symbols, struct layouts and default configuration through the binding (no device involved)."""
import ctypes

import numpy as np


def test_render_symbols_and_struct_layouts():
    from kimera_semantics_amd import binding as B
    for sym in ("ks_render_default_config", "ks_render_view", "ks_render_view_device"):
        assert sym in B.ABI_SYMBOLS and hasattr(B.lib(), sym), sym
    assert ctypes.sizeof(B.KsRenderConfig) == 12 and B.KsRenderConfig.min_range_m.offset == 4 and B.KsRenderConfig.max_range_m.offset == 8
    assert ctypes.sizeof(B.KsRenderStats) == 24 and B.KsRenderStats.pixels_missed.offset == 8 and B.KsRenderStats.samples.offset == 16
    cfg = B.KsRenderConfig()
    assert B.lib().ks_render_default_config(ctypes.byref(cfg)) == 0
    assert cfg.min_weight == np.float32(1e-4) and cfg.min_range_m == np.float32(0.1) and cfg.max_range_m == 10.0
    assert B.lib().ks_render_default_config(None) == B.KS_ERR_INVALID_ARG
    assert hasattr(B.HipIntegrator, "render") and hasattr(B.HipIntegrator, "render_device")
