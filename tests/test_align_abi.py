"""The scan-alignment symbols, struct layouts and default configuration through the binding (no device involved)."""
import ctypes

import numpy as np


def test_align_symbols_and_struct_layouts():
    from kimera_semantics_amd import binding as B
    for sym in ("ks_align_default_config", "ks_align_points", "ks_align_points_device"):
        assert sym in B.ABI_SYMBOLS and hasattr(B.lib(), sym), sym
    names = ["min_weight", "max_residual_m", "damping", "eps_rotation_rad", "eps_translation_m", "max_iterations", "point_stride", "min_inliers", "dof_mask"]
    assert [f for f, _ in B.KsAlignConfig._fields_] == names and ctypes.sizeof(B.KsAlignConfig) == 36
    assert [getattr(B.KsAlignConfig, f).offset for f in names] == list(range(0, 36, 4))
    S = B.KsAlignStats
    assert ctypes.sizeof(S) == 48
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 16, 24, 32, 40]
    assert [f for f, _ in S._fields_] == ["status", "iterations", "points_used", "inliers_first", "inliers_last", "rmse_first", "rmse_last"]
    assert (B.KS_ALIGN_CONVERGED, B.KS_ALIGN_ITERATION_LIMIT, B.KS_ALIGN_TOO_FEW_INLIERS, B.KS_ALIGN_DEGENERATE) == (0, 1, 2, 3)
    assert hasattr(B.HipIntegrator, "align") and hasattr(B.HipIntegrator, "align_device")


def test_align_defaults_and_null_config():
    from kimera_semantics_amd import binding as B
    cfg = B.KsAlignConfig()
    assert B.lib().ks_align_default_config(ctypes.byref(cfg)) == 0
    assert cfg.min_weight == np.float32(1e-4) and cfg.max_residual_m == 0.0 and cfg.damping == np.float32(1e-6)
    assert cfg.eps_rotation_rad == np.float32(1e-4) and cfg.eps_translation_m == np.float32(1e-4)
    assert (cfg.max_iterations, cfg.point_stride, cfg.min_inliers, cfg.dof_mask) == (10, 1, 64, 0x3f)
    assert B.lib().ks_align_default_config(None) == B.KS_ERR_INVALID_ARG


def test_align_structs_match_the_c_header(tmp_path):
    """sizeof / offsetof of the two structs as gcc sees include/ks_hip.h == the ctypes mirrors."""
    import os
    import shutil
    import subprocess
    import pytest
    from kimera_semantics_amd import binding as B
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ks_hip.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %d\\n", sizeof(ks_align_config), sizeof(ks_align_stats), offsetof(ks_align_config, dof_mask),'
                   ' offsetof(ks_align_stats, points_used), offsetof(ks_align_stats, rmse_last), KS_ALIGN_DEGENERATE); return 0;}\n')
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.check_call(["gcc", "-I", inc, "-o", str(tmp_path / "sz"), str(src)])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert got == [ctypes.sizeof(B.KsAlignConfig), 48, B.KsAlignConfig.dof_mask.offset, B.KsAlignStats.points_used.offset, B.KsAlignStats.rmse_last.offset, 3]
