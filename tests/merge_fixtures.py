"""Shared helpers of the MergeToLineTracks tests: the golden files of tests/golden/make_merge_golden.py as the
arguments of limap_amd.merging.merging, and the track arrays to compare."""
import importlib.util
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge")
SCENES = ("a", "b", "c", "d")
STAGES = ("merge", "filter1", "remerge", "filter2")
REMERGE_L3 = dict(score_th=0.5, th_angle=5.0, th_overlap=0.001, th_smartoverlap=0.1, th_smartangle=1.0, th_perp=0.5,
                  th_innerseg=0.5)  # cfgs/fitnmerge/default.yaml:77-86
FILTER2D = (8.0, 5.0)


def load(name):
    with np.load(os.path.join(GOLDEN, f"merge_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def generator():
    path = os.path.join(os.path.dirname(GOLDEN), "make_merge_golden.py")
    spec = importlib.util.spec_from_file_location("make_merge_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def call_args(g):
    """(linker, all_2d_segs, imagecols, seg3d_list, neighbors, var2d) of a golden input set"""
    from limap_amd.base import ImageCollection
    ids = [int(i) for i in g["img_ids"]]
    so, no = g["seg_off"], g["nb_off"]
    all_2d = {i: g["segs2"][so[n]:so[n + 1]] for n, i in enumerate(ids)}
    seg3d = {i: g["segs3"][so[n]:so[n + 1]].reshape(-1, 2, 3) for n, i in enumerate(ids)}
    nbs = {i: [int(j) for j in g["nb"][no[n]:no[n + 1]]] for n, i in enumerate(ids)}
    imagecols = ImageCollection.from_arrays(ids, g["kvec"], g["qvec"], g["tvec"])
    return json.loads(str(g["linker"])), all_2d, imagecols, seg3d, nbs, float(g["var2d"])


def tracks_to_arrays(tracks):
    off = np.zeros(len(tracks) + 1, np.int64)
    off[1:] = np.cumsum([len(t.image_id_list) for t in tracks])
    cat = lambda xs, shape, dt: np.array(xs, dt).reshape(shape)  # noqa: E731
    return dict(
        line=cat([list(t.line.start) + list(t.line.end) + [t.line.uncertainty] for t in tracks], (-1, 7), float),
        off=off,
        image_ids=cat([i for t in tracks for i in t.image_id_list], (-1,), np.int32),
        line_ids=cat([i for t in tracks for i in t.line_id_list], (-1,), np.int32),
        node_ids=cat([i for t in tracks for i in t.node_id_list], (-1,), np.int32),
        scores=cat([s for t in tracks for s in t.score_list], (-1,), float),
        line2d=cat([list(l.start) + list(l.end) for t in tracks for l in t.line2d_list], (-1, 4), float),
        line3d=cat([list(l.start) + list(l.end) + list(l.depths) + [l.uncertainty, l.score] for t in tracks
                    for l in t.line3d_list], (-1, 10), float))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def assert_stage(a, g, stage):
    """track arrays `a` (TrackSet.arrays() form) against stage `stage` of golden set `g`"""
    p = stage + "_"
    assert len(a["off"]) == len(g[p + "off"]), f"{stage}: {len(a['off']) - 1} tracks, reference {len(g[p + 'off']) - 1}"
    assert np.array_equal(a["off"], g[p + "off"]), stage
    assert np.array_equal(a["image_ids"], g[p + "img"]), stage
    assert np.array_equal(a["line_ids"], g[p + "lid"]), stage
    assert np.array_equal(a["node_ids"], g[p + "nid"]), stage
    assert np.array_equal(bits(a["scores"]), bits(g[p + "score"])), stage
    assert np.array_equal(bits(a["line2d"]), bits(g[p + "line2d"])), stage
    assert np.array_equal(bits(a["line3d"]), bits(g[p + "line3d"])), stage
    ref = g[p + "line"]
    got = a["line"][:len(ref)]
    # track lines: within 1e-9 relative, start and end not swapped
    tol = 1e-9 * np.maximum(1.0, np.abs(ref[:, :6]))
    assert np.all(np.abs(got[:, :6] - ref[:, :6]) <= tol), stage
    assert np.array_equal(bits(got[:, 6]), bits(ref[:, 6])), stage
