"""limap_amd.merging.merging (k_merge_pairs + lt_merge.cpp) against the CPU oracle's MergeToLineTracks
(oracle/lt_oracle.cpp ora_merge_to_tracks, pinned to the reference by tests/test_oracle_vs_ref.py) on the scenes of
tests/merge_fixtures.py: random scenes, line counts on both sides of the 256-row tiles and the 1024-line LDS chunks,
negative / large / wrapping image ids, 3D angles at and around th_angle and the guard's cut, degenerate geometry, the C
ABI's init paths and an overflowing edge buffer.  Each scene is also run with the device's shortcuts off
(LT_TEST_MERGE_PARITY_SLOW, LT_TEST_MERGE_NO_GUARD): the result must not change by a bit."""
import ctypes as C
import json

import numpy as np
import pytest

import merge_fixtures as mf
from merge_fixtures import FILTER2D, REMERGE_L3, STAGES, assert_stage, bits, call_args

pytestmark = pytest.mark.gpu

SWITCHES = ("LT_TEST_MERGE_PARITY_SLOW", "LT_TEST_MERGE_NO_GUARD")


def _device(g, monkeypatch=None, switch=None):
    from limap_amd import merging
    if switch:
        monkeypatch.setenv(switch, "1")
    try:
        return merging.TrackSet.from_merge(*call_args(g))
    finally:
        if switch:
            monkeypatch.delenv(switch)


def _labels(a, n_nodes):
    lab = -np.ones(n_nodes, np.int32)
    for t in range(len(a["off"]) - 1):
        lab[a["node_ids"][a["off"][t]:a["off"][t + 1]]] = t
    return lab


def _check_graph(graph, o, where):
    assert np.array_equal(graph.node_image_ids, o["node_img"]), where
    assert np.array_equal(graph.node_line_ids, o["node_line"]), where
    assert len(graph.edge_idx1) == len(o["edge_n1"]), f"{where}: {len(graph.edge_idx1)} edges, oracle {len(o['edge_n1'])}"
    assert np.array_equal(graph.edge_idx1, o["edge_n1"]), where
    assert np.array_equal(graph.edge_idx2, o["edge_n2"]), where
    assert np.array_equal(bits(graph.edge_sim), bits(o["edge_sim"])), where


def _check_chain(ts, o, where):
    """the merge, then filter / remerge / filter of the fit-and-merge runner, each against the oracle's"""
    _check_graph(ts.graph, o, where)
    a = ts.arrays()
    assert np.array_equal(_labels(a, len(o["node_img"])), o["labels"]), where
    assert_stage(a, o, "merge")
    ts.filter_by_reprojection(*FILTER2D, num_outliers=0)
    assert_stage(ts.arrays(), o, "filter1")
    ts.remerge(REMERGE_L3, num_outliers=0)
    assert_stage(ts.arrays(), o, "remerge")
    ts.filter_by_reprojection(*FILTER2D, num_outliers=0)
    assert_stage(ts.arrays(), o, "filter2")


def _same_device_result(a, b, where):
    """two device runs of one scene: graph and tracks identical to the bit"""
    for k in ("node_image_ids", "node_line_ids", "edge_idx1", "edge_idx2"):
        assert np.array_equal(getattr(a.graph, k), getattr(b.graph, k)), f"{where}: {k}"
    assert np.array_equal(bits(a.graph.edge_sim), bits(b.graph.edge_sim)), where
    x, y = a.arrays(), b.arrays()
    for k in x:
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), f"{where}: {k}"


def _against_oracle(oracle, monkeypatch, g, where, switches=SWITCHES):
    o = mf.oracle_chain(oracle, g)
    ts = _device(g)
    ref = _device(g)  # (a second run, kept unfiltered for the switch comparisons)
    _check_chain(ts, o, where)
    for sw in switches:
        _same_device_result(_device(g, monkeypatch, sw), ref, f"{where} {sw}")
    return o, ref


@pytest.mark.parametrize("k", range(16))
def test_random_scene(gpu_lib, oracle, monkeypatch, k):
    seed = 6000 + k
    _against_oracle(oracle, monkeypatch, mf.random_scene(seed), f"seed {seed}")


SHAPES = {
    "small_tiles": ((1, 63, 64, 65, 255, 256), 51),
    "chunks": ((257, 1023, 1024, 1025), 52),
    "two_chunks_self": ((2049, 1025, 255), 53),
    "mixed": ((1024, 1023, 256, 64, 1), 54),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_tile_and_chunk_shapes(gpu_lib, oracle, monkeypatch, name):
    """line counts on both sides of the 256-row tiles and of the 1024-line LDS chunks, in the self and the cross pass;
    lines at every index have partners (merge_fixtures.shaped_scene), so a wrong chunk offset loses or invents edges"""
    counts, seed = SHAPES[name]
    o, _ = _against_oracle(oracle, monkeypatch, mf.shaped_scene(counts, seed), name)
    assert len(o["edge_n1"]) > sum(counts) // 4, "the scene must have edges at every size"
    if max(counts) > 1024:  # edges to neighbour lines past the first chunk
        assert (np.asarray(o["node_line"])[o["edge_n2"]] >= 1024).any()


def test_zero_length_image_and_empty_neighbour(gpu_lib, oracle, monkeypatch):
    g = mf.shaped_scene((300, 257, 1025), 55, zero_image=1, empty_neighbour=True)
    o, _ = _against_oracle(oracle, monkeypatch, g, "zero / empty")
    ids = [int(i) for i in g["img_ids"]]
    assert ids[1] not in set(o["node_img"].tolist())


@pytest.mark.parametrize("name", sorted(mf.edge_scenes()))
def test_edge_scene(gpu_lib, oracle, monkeypatch, name):
    """angles th_angle (1 +- delta) and guard cut (1 +- delta) for th_angle in merge_fixtures.ANGLES, identical /
    parallel / tied / very short lines, depth 0 and negative depth in the neighbour view, negative ids, ids above 2^29
    (generic parity rule) and near INT_MAX (the int key wraps), self-listed neighbours"""
    _against_oracle(oracle, monkeypatch, mf.edge_scenes()[name](), name)


def _abi_merge(ctx, g):
    from limap_amd import _capi, merging
    cfg = merging._merge_linker_cfg(json.loads(str(g["linker"])))
    p = _capi.ptr
    out = C.c_void_p()
    so, s3 = np.ascontiguousarray(g["seg_off"], np.int64), np.ascontiguousarray(g["segs3"], np.float64)
    no, nb = np.ascontiguousarray(g["nb_off"], np.int64), np.ascontiguousarray(g["nb"], np.int32)
    nb = nb if nb.size else np.zeros(1, np.int32)
    ctx.chk(ctx.L.lt_merge_to_tracks(ctx.h, p(so, C.c_int64), p(s3, C.c_double), p(no, C.c_int64), p(nb, C.c_int32),
                                     C.byref(cfg), float(g["var2d"]), C.byref(out)))
    ts = merging.TrackSet(ctx, out.value)
    ts.graph = merging.MergeGraph.from_ctx(ctx)
    return ts


def test_c_abi_unsorted_init(gpu_lib):
    """lt_init with the images in another order than ascending id, then lt_merge_to_tracks with its arrays in ascending
    id order (include/limap_amd.h): the same result as the Python path"""
    from limap_amd import _capi
    g = mf.id_scene("wide", self_listed=True)
    ref = _device(g)
    perm = np.array([2, 0, 3, 1])
    so = g["seg_off"]
    segs = [g["segs2"][so[n]:so[n + 1]] for n in perm]
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    ctx = _capi.Context()
    ctx.init(g["img_ids"][perm], g["kvec"][perm], g["qvec"][perm], g["tvec"][perm], off, np.concatenate(segs, 0))
    _same_device_result(_abi_merge(ctx, g), ref, "unsorted lt_init")


def test_c_abi_add_halfpix_context(gpu_lib, oracle):
    """a context created with add_halfpix = 1 (lt_init and lt_init_device): the merge reads the 2D segments as given,
    like the reference's MergeToLineTracks, and equals the oracle and the Python path"""
    import torch
    from limap_amd import _capi
    g = mf.shaped_scene((300, 257, 120), 56)
    o = mf.oracle_chain(oracle, g)
    ref = _device(g)
    ctx = _capi.Context({"add_halfpix": True})
    ctx.init(g["img_ids"], g["kvec"], g["qvec"], g["tvec"], g["seg_off"], g["segs2"])
    _same_device_result(_abi_merge(ctx, g), ref, "add_halfpix lt_init")
    _check_chain(_abi_merge(ctx, g), o, "add_halfpix lt_init")
    d = [torch.tensor(np.ascontiguousarray(g[k], np.float64), device="cuda") for k in ("kvec", "qvec", "tvec", "segs2")]
    torch.cuda.synchronize()
    ctx2 = _capi.Context({"add_halfpix": True})
    ctx2.init_device(g["img_ids"], *(x.data_ptr() for x in d[:3]), g["seg_off"], d[3].data_ptr())
    _same_device_result(_abi_merge(ctx2, g), ref, "add_halfpix lt_init_device")


def test_edge_buffer_overflow_on_chunked_scene(gpu_lib, monkeypatch):
    """the 1025-line shape with an edge buffer below its edge count: counted, run again, the same result"""
    g = mf.shaped_scene((257, 1023, 1024, 1025), 52)
    ref = _device(g)
    n = ref.merge_timers["edges"]
    assert ref.merge_timers["attempts"] == 1 and n > 1000
    monkeypatch.setenv("LT_TEST_MERGE_EDGE_CAP", str(n // 3))
    ts = _device(g)
    assert ts.merge_timers["attempts"] == 2 and ts.merge_timers["edges"] == n
    _same_device_result(ts, ref, "edge cap")
