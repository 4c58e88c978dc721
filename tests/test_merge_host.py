"""MergeToLineTracks without a GPU: the C ABI surface, synthetic.make_fit_segs, the golden files' own consistency, the
CPU oracle's merge (oracle/lt_oracle.cpp ora_merge_to_tracks, the checker of tests/test_gpu_merge_oracle.py) against
the golden files, and the argument errors of limap_amd.merging.merging (raised before any device work)."""
import json
import os
import re

import numpy as np
import pytest

from merge_fixtures import (ANGLES, STAGES, SCENES, angle_scene, assert_stage, bits, call_args, generator, load,
                            oracle_chain, pair_angles)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGE_ABI = ("lt_merge_to_tracks", "lt_merge_graph_size", "lt_merge_graph_get", "lt_merge_get_timers")


def test_abi_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "limap_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    from limap_amd import _capi
    for name in MERGE_ABI:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _capi.EXPORTED_SYMBOLS, name
    L = _capi.load_library()  # (loads without a device)
    for name in MERGE_ABI:
        assert getattr(L, name).argtypes, f"{name} has no prototype in _capi"


def _point_line_dist(p, a, b):
    u = (b - a) / np.linalg.norm(b - a)
    v = p - a
    return np.linalg.norm(v - (v @ u) * u)


def test_make_fit_segs():
    from limap_amd import synthetic as syn
    sc = syn.make_scene(n_views=6, n_segs=60, n_neighbors=3, seed=4)
    f1 = syn.make_fit_segs(sc, seed=2, depth_noise=0.0, fail_frac=0.2)
    f2 = syn.make_fit_segs(sc, seed=2, depth_noise=0.0, fail_frac=0.2)
    assert sorted(f1) == [int(i) for i in sc.img_ids]
    n_zero = n_fit = 0
    for n, i in enumerate(sc.img_ids):
        a = f1[int(i)]
        assert a.shape == (sc.seg_off[n + 1] - sc.seg_off[n], 2, 3)
        assert np.array_equal(a, f2[int(i)])
        gids = sc.gt_ids[sc.seg_off[n]:sc.seg_off[n + 1]]
        zero = np.all(a.reshape(len(a), -1) == 0, axis=1)
        assert np.all(zero[gids < 0]), "clutter must be zeros"
        n_zero += int(zero[gids >= 0].sum())
        for m in np.nonzero(~zero)[0]:
            gt = sc.gt_lines[gids[m]]
            for p in a[m]:
                assert _point_line_dist(p, gt[:3], gt[3:]) < 1e-8
            n_fit += 1
    assert n_fit > 0 and n_zero > 0  # the failed fraction is zeros too
    f3 = syn.make_fit_segs(sc, seed=2, depth_noise=0.01, fail_frac=0.2)
    assert not np.array_equal(f3[int(sc.img_ids[0])], f1[int(sc.img_ids[0])])


def _greedy_labels(n_nodes, node_img, e1, e2, sim):
    """ComputeLineTrackLabelsGreedy (merging/merging.cc:18-103), restated"""
    order = sorted(zip(sim.tolist(), e1.tolist(), e2.tolist()), reverse=True)
    parent = [-1] * n_nodes
    images = [{int(node_img[i])} for i in range(n_nodes)]

    def root(i):
        r = i
        while parent[r] != -1:
            r = parent[r]
        while parent[i] != -1:
            nx = parent[i]
            if nx != r:
                parent[i] = r
            i = nx
        return r

    for _, a, b in order:
        r1, r2 = root(a), root(b)
        if r1 == r2:
            continue
        if len(images[r1]) < len(images[r2]):
            parent[r1] = r2
            images[r2] |= images[r1]
            images[r1] = set()
        else:
            parent[r2] = r1
            images[r1] |= images[r2]
            images[r2] = set()
    labels = [-1] * n_nodes
    n = 0
    for i in range(n_nodes):
        if parent[i] != -1 and parent[parent[i]] == -1 and labels[parent[i]] == -1:
            labels[parent[i]] = n
            n += 1
    for i in range(n_nodes):
        if parent[i] != -1:
            labels[i] = labels[root(i)]
    return np.array(labels, np.int32)


@pytest.mark.parametrize("name", SCENES)
def test_golden_self_consistent(name):
    g = load(name)
    N = len(g["node_img"])
    ids = [int(i) for i in g["img_ids"]]
    # nodes: images in ascending id order, lines in order, exactly the lines of non-zero length
    so = g["seg_off"]
    want = [(i, l) for n, i in enumerate(ids) for l in range(so[n + 1] - so[n])
            if np.linalg.norm(g["segs3"][so[n] + l, :3] - g["segs3"][so[n] + l, 3:]) != 0]
    assert list(zip(g["node_img"].tolist(), g["node_line"].tolist())) == want
    assert np.all((g["edge_n1"] >= 0) & (g["edge_n1"] < N) & (g["edge_n2"] >= 0) & (g["edge_n2"] < N))
    assert np.array_equal(_greedy_labels(N, g["node_img"], g["edge_n1"], g["edge_n2"], g["edge_sim"]), g["labels"])
    # tracks of the merge: one per label, members in node order
    off, nid = g["merge_off"], g["merge_nid"]
    assert len(off) - 1 == (g["labels"].max() + 1 if N else 0)
    for t in range(len(off) - 1):
        m = nid[off[t]:off[t + 1]]
        assert np.all(np.diff(m) > 0) and np.all(g["labels"][m] == t)


def _stage_arrays(o, stage):
    p = stage + "_"
    return dict(off=o[p + "off"], image_ids=o[p + "img"], line_ids=o[p + "lid"], node_ids=o[p + "nid"],
                scores=o[p + "score"], line2d=o[p + "line2d"], line3d=o[p + "line3d"], line=o[p + "line"])


@pytest.mark.parametrize("name", SCENES)
def test_oracle_merge_reproduces_golden(oracle, name):
    """the oracle's MergeToLineTracks and the fit-and-merge chain after it are what the reference's own code wrote"""
    g = load(name)
    o = oracle_chain(oracle, g)
    for k in ("node_img", "node_line", "edge_n1", "edge_n2", "labels"):
        assert np.array_equal(o[k], g[k]), k
    assert np.array_equal(bits(o["edge_sim"]), bits(g["edge_sim"]))
    for stage in STAGES:
        assert_stage(_stage_arrays(o, stage), g, stage)


def test_oracle_merge_reproduces_scene_e_digests(oracle):
    gen = generator()
    with open(os.path.join(ROOT, "tests", "golden", "merge", "merge_e_digests.json")) as f:
        d = json.load(f)
    o = oracle_chain(oracle, gen.scene_e_inputs())
    assert len(o["node_img"]) == d["n_nodes"] and len(o["edge_n1"]) == d["n_edges"]
    assert gen.digest(o["node_img"], o["node_line"]) == d["nodes"]
    assert gen.digest(o["edge_n1"], o["edge_n2"], o["edge_sim"]) == d["edges"]
    assert gen.digest(o["labels"]) == d["labels"]
    for s in STAGES:
        assert len(o[s + "_off"]) - 1 == d[f"{s}_tracks"], s
        assert gen.digest(o[s + "_off"], o[s + "_img"], o[s + "_lid"], o[s + "_nid"]) == d[f"{s}_members"], s
        assert gen.digest(o[s + "_line"]) == d[f"{s}_line"], s


@pytest.mark.parametrize("th", [a for a in ANGLES if 0 < a < 90])
def test_angle_scenes_decide_at_the_threshold(oracle, th):
    """the pairs of merge_fixtures.angle_scene sit on both sides of th_angle, and the exact test decides them there:
    a pair is linked in the self pass iff its angle is at most th_angle"""
    o = oracle_chain(oracle, angle_scene(th))
    linked = {(int(o["node_line"][i]), int(o["node_line"][j])) for i, j in zip(o["edge_n1"], o["edge_n2"])
              if o["node_img"][i] == o["node_img"][j] == 0}
    angles = pair_angles(th)
    want = [n for n, a in enumerate(angles) if a <= th]
    assert 0 < len(want) < len(angles)
    assert sorted(n for n in range(len(angles)) if (2 * n, 2 * n + 1) in linked) == want


def test_golden_covers_the_quirks():
    b, c = load("b"), load("c")
    ids_b = b["img_ids"].tolist()
    assert ids_b != list(range(ids_b[0], ids_b[0] + len(ids_b)))  # non-contiguous ids
    counts = np.diff(b["nb_off"])
    assert (counts == 0).any() and (np.diff(b["seg_off"]) == 0).any()
    lists = {i: b["nb"][b["nb_off"][n]:b["nb_off"][n + 1]].tolist() for n, i in enumerate(ids_b)}
    assert any(lst != sorted(lst) for lst in lists.values())
    assert any(i not in lists[j] for i in ids_b for j in lists[i])  # asymmetric
    lists = {i: c["nb"][c["nb_off"][n]:c["nb_off"][n + 1]].tolist() for n, i in enumerate(c["img_ids"].tolist())}
    assert any(len(set(v)) < len(v) for v in lists.values())
    assert any(i in v for i, v in lists.items())


def _args():
    return list(call_args(load("a")))


def test_error_image_counts():
    from limap_amd import merging
    linker, all_2d, imagecols, seg3d, nbs, var2d = _args()
    nbs2 = dict(nbs)
    nbs2.pop(next(iter(nbs2)))
    with pytest.raises(ValueError):
        merging.merging(linker, all_2d, imagecols, seg3d, nbs2, var2d)
    seg3d2 = dict(seg3d)
    seg3d2.pop(next(iter(seg3d2)))
    with pytest.raises((ValueError, KeyError)):
        merging.merging(linker, all_2d, imagecols, seg3d2, nbs, var2d)


def test_error_segment_counts():
    from limap_amd import merging
    linker, all_2d, imagecols, seg3d, nbs, var2d = _args()
    k = next(iter(seg3d))
    seg3d = dict(seg3d)
    seg3d[k] = seg3d[k][:-1]
    with pytest.raises(ValueError):
        merging.merging(linker, all_2d, imagecols, seg3d, nbs, var2d)


def test_error_unknown_neighbour():
    from limap_amd import merging
    linker, all_2d, imagecols, seg3d, nbs, var2d = _args()
    k = next(iter(nbs))
    nbs = dict(nbs)
    nbs[k] = nbs[k] + [987654]
    with pytest.raises(IndexError):
        merging.merging(linker, all_2d, imagecols, seg3d, nbs, var2d)


def test_seg3d_forms_and_bad_shape():
    from limap_amd.merging import _seg3d_array
    a = np.arange(24, dtype=float).reshape(4, 2, 3)
    assert np.array_equal(_seg3d_array(a), a.reshape(4, 6))
    assert np.array_equal(_seg3d_array(a.reshape(4, 6)), a.reshape(4, 6))
    assert np.array_equal(_seg3d_array([x for x in a]), a.reshape(4, 6))
    assert _seg3d_array([]).shape == (0, 6)
    with pytest.raises(ValueError):
        _seg3d_array(np.zeros((4, 5)))
