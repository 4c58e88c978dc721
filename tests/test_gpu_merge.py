"""limap_amd.merging.merging (MergeToLineTracks on the GPU) against the reference's own merging code: the golden files
of tests/golden/make_merge_golden.py (scenes a-d in full, scene e as digests), and the fit-and-merge chain after it
(runners/line_fitnmerge.py:229-258)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from merge_fixtures import (FILTER2D, GOLDEN, REMERGE_L3, SCENES, STAGES, assert_stage, bits, call_args, generator,
                            load, tracks_to_arrays)

pytestmark = pytest.mark.gpu


def _labels_from_tracks(a, n_nodes):
    lab = -np.ones(n_nodes, np.int32)
    for t in range(len(a["off"]) - 1):
        lab[a["node_ids"][a["off"][t]:a["off"][t + 1]]] = t
    return lab


def _check_graph(graph, g):
    assert np.array_equal(graph.node_image_ids, g["node_img"])
    assert np.array_equal(graph.node_line_ids, g["node_line"])
    assert np.array_equal(graph.edge_idx1, g["edge_n1"])
    assert np.array_equal(graph.edge_idx2, g["edge_n2"])
    assert np.array_equal(bits(graph.edge_sim), bits(g["edge_sim"]))


@pytest.mark.parametrize("name", SCENES)
def test_merge_matches_reference(gpu_lib, name):
    from limap_amd import merging
    g = load(name)
    graph, tracks = merging.merging(*call_args(g))
    _check_graph(graph, g)
    a = tracks_to_arrays(tracks)
    assert np.array_equal(_labels_from_tracks(a, len(g["node_img"])), g["labels"])
    assert_stage(a, g, "merge")


@pytest.mark.parametrize("name", SCENES)
def test_fitnmerge_chain_trackset(gpu_lib, name):
    from limap_amd import merging
    g = load(name)
    ts = merging.TrackSet.from_merge(*call_args(g))
    _check_graph(ts.graph, g)
    assert_stage(ts.arrays(), g, "merge")
    ts.filter_by_reprojection(*FILTER2D, num_outliers=0)
    assert_stage(ts.arrays(), g, "filter1")
    ts.remerge(REMERGE_L3, num_outliers=0)
    assert_stage(ts.arrays(), g, "remerge")
    ts.filter_by_reprojection(*FILTER2D, num_outliers=0)
    assert_stage(ts.arrays(), g, "filter2")


@pytest.mark.parametrize("name", SCENES)
def test_fitnmerge_chain_module_functions(gpu_lib, name):
    from limap_amd import merging
    g = load(name)
    args = call_args(g)
    imagecols = args[2]
    _, tracks = merging.merging(*args)
    tracks = merging.filter_tracks_by_reprojection(tracks, imagecols, *FILTER2D, num_outliers=0)
    assert_stage(tracks_to_arrays(tracks), g, "filter1")
    tracks = merging.remerge(REMERGE_L3, tracks, num_outliers=0)
    assert_stage(tracks_to_arrays(tracks), g, "remerge")
    tracks = merging.filter_tracks_by_reprojection(tracks, imagecols, *FILTER2D, num_outliers=0)
    assert_stage(tracks_to_arrays(tracks), g, "filter2")


def test_scene_e_digests(gpu_lib):
    from limap_amd import merging
    gen = generator()
    with open(os.path.join(GOLDEN, "merge_e_digests.json")) as f:
        d = json.load(f)
    a = gen.scene_e_inputs()
    assert gen.digest(a["img_ids"], a["kvec"], a["qvec"], a["tvec"], a["seg_off"], a["segs2"], a["segs3"], a["nb_off"],
                      a["nb"]) == d["inputs"], "the synthetic inputs of scene (e) changed"
    ts = merging.TrackSet.from_merge(*call_args(a))
    gr = ts.graph
    assert gr.num_nodes() == d["n_nodes"] and gr.num_edges() == d["n_edges"]
    assert gen.digest(gr.node_image_ids, gr.node_line_ids) == d["nodes"]
    assert gen.digest(gr.edge_idx1, gr.edge_idx2, gr.edge_sim) == d["edges"]
    arr = ts.arrays()
    assert gen.digest(_labels_from_tracks(arr, gr.num_nodes())) == d["labels"]
    for stage in STAGES:
        if stage == "filter1" or stage == "filter2":
            ts.filter_by_reprojection(*FILTER2D, num_outliers=0)
        elif stage == "remerge":
            ts.remerge(REMERGE_L3, num_outliers=0)
        arr = ts.arrays()
        assert len(arr["off"]) - 1 == d[f"{stage}_tracks"], stage
        assert gen.digest(arr["off"], arr["image_ids"], arr["line_ids"], arr["node_ids"]) == d[f"{stage}_members"], stage


def test_edge_buffer_overflow_runs_again(gpu_lib, monkeypatch):
    """an edge buffer far too small: the kernels count every accepted pair, the host runs them again with room for all"""
    from limap_amd import merging
    g = load("c")
    ref = merging.TrackSet.from_merge(*call_args(g))
    assert ref.merge_timers["attempts"] == 1
    monkeypatch.setenv("LT_TEST_MERGE_EDGE_CAP", "16")
    ts = merging.TrackSet.from_merge(*call_args(g))
    assert ts.merge_timers["attempts"] == 2
    assert ts.merge_timers["edges"] == ref.merge_timers["edges"] > 16
    _check_graph(ts.graph, g)
    a, b = ts.arrays(), ref.arrays()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_c_abi_rejects_bad_arguments(gpu_lib):
    """lt_merge_to_tracks itself: 2D / 3D count mismatch and an unknown neighbour id are errors, not faults"""
    from limap_amd import _capi
    g = load("a")
    ctx = _capi.Context()
    ctx.init(g["img_ids"], g["kvec"], g["qvec"], g["tvec"], g["seg_off"], g["segs2"])
    cfg = _capi.config_from_dict(None)
    p = _capi.ptr
    out = C.c_void_p()
    segs3 = np.ascontiguousarray(g["segs3"])
    bad_off = g["seg_off"].copy()
    bad_off[1:] -= 1
    bad_off[0] = 0
    nb_off, nb = np.ascontiguousarray(g["nb_off"]), np.ascontiguousarray(g["nb"]).copy()
    with pytest.raises(ValueError):
        ctx.chk(ctx.L.lt_merge_to_tracks(ctx.h, p(bad_off, C.c_int64), p(segs3, C.c_double), p(nb_off, C.c_int64),
                                         p(nb, C.c_int32), C.byref(cfg), 5.0, C.byref(out)))
    assert not out.value
    nb[0] = 12345
    seg_off = np.ascontiguousarray(g["seg_off"])
    with pytest.raises(IndexError):
        ctx.chk(ctx.L.lt_merge_to_tracks(ctx.h, p(seg_off, C.c_int64), p(segs3, C.c_double), p(nb_off, C.c_int64),
                                         p(nb, C.c_int32), C.byref(cfg), 5.0, C.byref(out)))
    assert not out.value
