"""-m gpu: k_track_connect, the device half of RemergeLineTracks, on its own -- lt_fn_track_connect against the restated
pair loop of tests/connect_cases.py over the CPU oracle's check_connection, on the cases of that module (tile and grid
edges, orientation, the cosine pre-test at its threshold, a full survivor queue, a workgroup without an active track, edge
counts around the first copy, a first launch without room).  Edges and partitions are discrete: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import connect_cases as cc

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in cc.all_cases()]


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    """one context for the module, as a remerge to its fixed point uses one: the device buffers are reused"""
    from limap_amd import _capi
    c = _capi.Context()
    c.init([0], np.array([[1.0, 1, 0, 0]]), np.array([[1.0, 0, 0, 0]]), np.zeros((1, 3)), np.zeros(2, np.int64),
           np.zeros((0, 4)))
    return c


def run(ctx, case):
    from limap_amd import merging
    name, line7, active, linker, capacity0, _ = case
    return merging.track_connect_edges(ctx, line7, active, linker, capacity0)


def explain(case, got, want):
    """the first few missing and spurious pairs with what decides them"""
    _, line7, active, _, _, _ = case
    g, w = set(map(tuple, got.tolist())), set(map(tuple, want.tolist()))
    all_active = bool(active.all())
    rows = []
    for kind, pairs in (("missing", sorted(w - g)), ("spurious", sorted(g - w))):
        for i, j in pairs[:6]:
            side = "-" if not all_active else ("i tests" if (i + j) & 1 else "j tests")
            rows.append(f"{kind} ({i}, {j}): active {int(active[i])}/{int(active[j])}, parity {(i + j) & 1} ({side}), "
                        f"wave {i // 64}/{j // 64}, lines {line7[i].tolist()} {line7[j].tolist()}")
    return f"{len(w - g)} missing, {len(g - w)} spurious of {len(w)}\n" + "\n".join(rows)


@pytest.mark.parametrize("name", NAMES)
def test_edge_set(ctx, name):
    case = cc.case_by_name(name)
    facts, want = case[5], cc.expected(case)
    r = run(ctx, case)
    got = r["edges"]
    print(f"{name}: T {len(case[1])}, edges {len(got)} (expected {len(want['edges'])}), n_raw {r['n_raw']} "
          f"(expected {want['n_raw']}), attempts {r['attempts']}")
    assert np.array_equal(got, want["edges"]), explain(case, got, want["edges"])
    assert r["n_raw"] >= len(got)
    assert r["n_raw"] == want["n_raw"]                       # one count per accepted (i, j) of the directed loop
    if facts["all_active"]:
        assert r["n_raw"] == len(got)
    assert r["attempts"] == facts.get("attempts", 1)


def test_too_small_output_reports_the_count(ctx):
    case = cc.case_by_name("count_below")
    _, line7, active, linker, _, facts = case
    from limap_amd import _capi, merging
    cfg = merging._linker_cfg(linker)
    p = _capi.ptr
    l7, act = np.ascontiguousarray(line7), np.ascontiguousarray(active, np.uint8)
    n, raw, att = C.c_int64(), C.c_int64(), C.c_int32()
    out = np.zeros(8, np.uint64)
    rc = ctx.L.lt_fn_track_connect(ctx.h, len(l7), p(l7, C.c_double), p(act, C.c_uint8), C.byref(cfg), 0, p(out, C.c_uint64),
                                   len(out), C.byref(n), C.byref(raw), C.byref(att))
    assert rc == -2 and n.value == facts["n_unique"] and not out.any()


def test_determinism_and_buffer_reuse(ctx):
    """twice the same set; and the same again after a larger case (more tracks, more edges) went through the buffers"""
    small, large = cc.case_by_name("tile_65_mixed"), cc.case_by_name("count_above")
    a, b = run(ctx, small), run(ctx, small)
    assert np.array_equal(a["edges"], b["edges"]) and a["n_raw"] == b["n_raw"]
    big = run(ctx, large)
    assert np.array_equal(big["edges"], cc.expected(large)["edges"])
    c = run(ctx, small)
    assert np.array_equal(a["edges"], c["edges"]) and a["n_raw"] == c["n_raw"]
    assert np.array_equal(c["edges"], cc.expected(small)["edges"])


@pytest.mark.parametrize("name", ["tile_257_mixed", "orientation_all", "orientation_mixed", "capacity_N"])
def test_one_remerge_pass(ctx, name):
    """lt_ts_remerge_once on a track set with one support per track (line3d = the track line): the partition of the input
    tracks into output tracks and the output order are the union / label rule (merging.cc:557-600) on the expected
    edges; groups of one come out inactive, the others active"""
    from limap_amd import _capi, merging
    case = cc.case_by_name(name)
    _, line7, active, linker, _, _ = case
    T = len(line7)
    off = np.arange(T + 1, dtype=np.int64)
    img = np.zeros(T, np.int32); lid = np.arange(T, dtype=np.int32); nid = np.arange(T, dtype=np.int32)
    score = np.ones(T); l2 = np.zeros((T, 4))
    l3 = np.zeros((T, 10))
    l3[:, :6] = line7[:, :6]; l3[:, 6:8] = 1.0; l3[:, 9] = 1.0
    l3[:, 8] = np.where(np.isnan(line7[:, 6]), 1.0, line7[:, 6])   # (the support's own uncertainty: the aggregator's input)
    p = _capi.ptr
    act = np.ascontiguousarray(active, np.uint8)
    ts = merging.TrackSet(ctx, ctx.L.lt_ts_create(T, p(np.ascontiguousarray(line7), C.c_double), p(act, C.c_uint8),
                                                  p(off, C.c_int64), p(img, C.c_int32), p(lid, C.c_int32), p(nid, C.c_int32),
                                                  p(score, C.c_double), p(l2, C.c_double), p(l3, C.c_double)))
    cfg = merging._linker_cfg(linker)
    ctx.chk(ctx.L.lt_ts_remerge_once(ctx.h, ts.h, C.byref(cfg), 0))
    a = ts.arrays()
    got = [a["line_ids"][a["off"][g]:a["off"][g + 1]].tolist() for g in range(len(a["off"]) - 1)]
    want = cc.groups_as_lists(cc.groups_from_edges(T, cc.expected(case)["edges"]))
    assert got == want
    assert len(want) < T
    assert a["active"].tolist() == [len(g) > 1 for g in want]
