"""The C-ABI library loads and exports every symbol include/limap_amd.h declares (no compute: runs
without a GPU), and the Python binding agrees with the C layout."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "limap_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lt_[a-zA-Z0-9_]+)\s*\(", text)))


def test_header_declares_expected_surface():
    syms = declared_symbols()
    for must in ("lt_create", "lt_init", "lt_triangulate_image", "lt_triangulate_image_exhaustive",
                 "lt_compute_tracks", "lt_get_tracks", "lt_set_ranges", "lt_get_best", "lt_vp_detect",
                 "lt_fn_vp_cluster_host", "lt_vp_cluster_sets", "lt_bpt_junctions", "lt_fn_bpt_grid_keys",
                 "lt_fn_bpt_close_pairs_host", "lt_fn_track_connect", "lt_fn_gate_outcomes"):
        assert must in syms


def test_library_exports_every_declared_symbol(gpu_lib):
    for name in declared_symbols():
        assert hasattr(gpu_lib, name), f"{name} declared in include/limap_amd.h but not exported"


def test_binding_covers_every_symbol():
    from limap_amd import _capi
    assert sorted(_capi.EXPORTED_SYMBOLS) == declared_symbols()


def test_config_layout_and_defaults(gpu_lib):
    from limap_amd import _capi
    assert gpu_lib.lt_sizeof_config() == C.sizeof(_capi.LtConfig)
    assert gpu_lib.lt_abi_version() == 2
    cfg = _capi.config_from_dict(None)
    # C++ defaults of the reference (base_line_triangulator.h:27-42, global_line_triangulator.h:16-23,
    # line_linker.h:24-45,94-112)
    assert (cfg.min_length_2d, cfg.line_tri_angle_threshold, cfg.IoU_threshold) == (20.0, 5.0, 0.1)
    assert (cfg.sensitivity_threshold, cfg.var2d, cfg.fullscore_th) == (70.0, 2.0, 1.0)
    assert (cfg.max_valid_conns, cfg.min_num_outer_edges, cfg.num_outliers_aggregator) == (1000, 1, 2)
    assert (cfg.l2_th_angle, cfg.l2_th_perp, cfg.l2_th_overlap, cfg.l2_use_innerseg) == (8.0, 5.0, 0.1, 0)
    assert (cfg.l3_th_angle, cfg.l3_th_innerseg, cfg.l3_th_scaleinv, cfg.l3_use_scaleinv) == (10.0, 0.02, 0.01, 0)


def test_config_from_dict_semantics():
    """ASSIGN_PYDICT_ITEM semantics (internal/helpers.h:25-27): present keys override, unknown keys
    are ignored, nested linker dicts are honoured."""
    from limap_amd import _capi, synthetic as syn
    d = syn.default_triangulation_cfg()
    d["unknown_key"] = 7
    d["remerging"] = {"disable": False}
    cfg = _capi.config_from_dict(d)
    assert cfg.min_length_2d == 0.0 and cfg.line_tri_angle_threshold == 1.0 and cfg.min_num_outer_edges == 0
    assert cfg.l2_th_angle == 5.0 and cfg.l2_th_perp == 2.0 and cfg.l2_th_overlap == 0.05
    assert cfg.l3_th_scaleinv == 0.015 and cfg.l3_th_smartangle == 2.0 and cfg.l3_th_innerseg == 1.0
    assert cfg.l2_th_smartoverlap == 0.2  # not in the yaml: keeps the C++ default
    assert cfg.merging_strategy == 0
    assert _capi.config_from_dict({"merging_strategy": "nope"}).merging_strategy == 99


def test_no_gpu_means_loud_failure(gpu_lib):
    """Without a HIP device lt_create returns NULL and the Python layer raises: no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from limap_amd import _capi
    with pytest.raises(RuntimeError, match="no usable HIP device"):
        _capi.Context()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "limap_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in text.replace("no oracle", ""), f"{f} mentions the oracle"


def test_python_surface_lists_every_free_function_of_the_reference_bindings():
    """limap/triangulation/__init__.py does `from _limap._triangulation import *`: the mirror's __all__ must carry the ten
    free functions of triangulation/bindings.cc:22-31 and the two classes (read from the reference tree where it exists)."""
    import os
    import re
    from limap_amd import triangulation as tri
    names = ["get_normal_direction", "get_direction_from_VP", "compute_essential_matrix", "compute_fundamental_matrix",
             "compute_epipolar_IoU", "triangulate_point", "triangulate_line_by_endpoints", "triangulate_line",
             "triangulate_line_with_one_point", "triangulate_line_with_direction"]
    src = "/root/reference/src/limap/triangulation/bindings.cc"
    if os.path.exists(src):
        found = re.findall(r'm\.def\("(\w+)"', open(src).read())
        assert sorted(found) == sorted(names)
    for n in names + ["GlobalLineTriangulator", "GlobalLineTriangulatorConfig"]:
        assert n in tri.__all__ and callable(getattr(tri, n)), n
