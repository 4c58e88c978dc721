"""The fit-and-merge runner's chain on the GPU -- depth maps -> fit_3d_segs_arrays -> merging.TrackSet.from_merge ->
filter / remerge / filter (runners/line_fitnmerge.py:201-258) -- against tests/fit_oracle.py followed by the CPU
oracle's MergeToLineTracks and the same chain: graph, labels and members bit for bit, track lines within 1e-9."""
import numpy as np
import pytest

import merge_fixtures as mf
from fit_scenes import oracle_scene
from merge_fixtures import FILTER2D, REMERGE_L3, assert_stage, bits

pytestmark = pytest.mark.gpu


def _labels(a, n_nodes):
    lab = -np.ones(n_nodes, np.int32)
    for t in range(len(a["off"]) - 1):
        lab[a["node_ids"][a["off"][t]:a["off"][t + 1]]] = t
    return lab


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_depth_fit_then_merge_chain(oracle, dtype):
    from limap_amd import fitting, merging, synthetic as syn
    base_sc = syn.make_scene(n_views=5, n_segs=30, n_neighbors=3, seed=4)
    h, w = 150, 200
    sc = syn.resize_scene(base_sc, h, w)
    depths = syn.render_depths(base_sc, h, w, noise=0.002, hole_frac=0.03, outlier_frac=0.03, dtype=dtype, seed=4)
    all_2d = sc.all_2d_segs()
    imagecols = syn.imagecols_of(sc)
    cfg = syn.default_merging_cfg(var2d=5.0)
    linker = dict(linker2d=cfg["linker2d"], linker3d=cfg["linker3d"])
    seg3d, info, _ = fitting.fit_3d_segs_arrays(all_2d, imagecols, depths, dict(ransac_th=0.75,
                                                                                min_percentage_inliers=0.6, var2d=5.0))
    ref = oracle_scene(all_2d, sc, depths)
    ids = [int(i) for i in sc.img_ids]
    ref3d = {i: np.stack([r["seg"] for r in ref[i]]) if ref[i] else np.zeros((0, 2, 3)) for i in ids}
    for i in ids:
        assert np.array_equal(bits(seg3d[i]), bits(ref3d[i])), f"image {i}: fitted segments differ from the oracle"
    assert sum(int((info[i]["status"] == 0).sum()) for i in ids) > len(ids) * 5
    g = mf._pack(ids, sc.kvec, sc.qvec, sc.tvec, [all_2d[i] for i in ids], [ref3d[i] for i in ids],
                 [sc.neighbors[i] for i in ids], linker, 5.0)
    o = mf.oracle_chain(oracle, g)
    ts = merging.TrackSet.from_merge(linker, all_2d, imagecols, seg3d, sc.neighbors, 5.0)
    gr = ts.graph
    assert np.array_equal(gr.node_image_ids, o["node_img"]) and np.array_equal(gr.node_line_ids, o["node_line"])
    assert np.array_equal(gr.edge_idx1, o["edge_n1"]) and np.array_equal(gr.edge_idx2, o["edge_n2"])
    assert np.array_equal(bits(gr.edge_sim), bits(o["edge_sim"]))
    assert len(gr.edge_idx1) > 0
    a = ts.arrays()
    assert np.array_equal(_labels(a, len(o["node_img"])), o["labels"])
    assert_stage(a, o, "merge")
    ts.filter_by_reprojection(*FILTER2D, num_outliers=0)
    assert_stage(ts.arrays(), o, "filter1")
    ts.remerge(REMERGE_L3, num_outliers=0)
    assert_stage(ts.arrays(), o, "remerge")
    ts.filter_by_reprojection(*FILTER2D, num_outliers=0)
    assert_stage(ts.arrays(), o, "filter2")
