"""limap_amd.matching, host side (no GPU): the host restatement lt_fn_match_pair_host against the rows limap's own
matchers returned for every fixture of tests/golden/match (written by tests/golden/make_match_golden.py).

Reference and restatement each sum an FP32 dot product in SOME order, so they may rank two columns differently only
where the exact scores are closer than the two error bounds (exact_scores / row_analysis of the generator, DESIGN
section 17).  A row whose best k columns are separated from every other column by more than the bounds is DECIDED and
must equal the reference's row exactly; every other row must be admissible; at most 10 % of a fixture's rows may be
undecided, so the second clause cannot carry the test."""
import glob
import importlib.util
import os

import numpy as np
import pytest

from limap_amd import matching

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_match_golden", os.path.join(HERE, "golden", "make_match_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(gen.OUT, "*.npz")))
EXPECTED = ["endpoints_m2_below_topk", "endpoints_synthetic", "endpoints_top10", "l2d2_empty", "l2d2_mutual",
            "l2d2_one_vs_many", "l2d2_ragged", "l2d2_synthetic", "l2d2_top1", "l2d2_top10"]


def test_every_fixture_is_there():
    assert FIXTURES == EXPECTED


def _lines(kind, d):
    return d.shape[0] if kind == "l2d2" else d.shape[1] // 2


@pytest.mark.parametrize("name", EXPECTED)
def test_restatement_against_reference_rows(name):
    kind, topk, descs, pairs, ref = gen.load_fixture(os.path.join(gen.OUT, name + ".npz"))
    n_rows = n_undecided = 0
    for p, (a, b) in enumerate(pairs):
        m1, m2 = _lines(kind, descs[a]), _lines(kind, descs[b])
        ours, scores = matching.match_pair_host(descs[a], descs[b], kind, topk, return_scores=True)
        assert ours.dtype == np.int32 and ours.shape[1:] == (2,)
        if m1 == 0 or m2 == 0:
            assert ours.shape == (0, 2) and ref[p].shape == (0, 2)
            continue
        E, B = gen.exact_scores(kind, descs[a], descs[b])
        # the reported score is within the bound of the exact one
        assert (np.abs(scores.astype(np.float64) - E[ours[:, 0], ours[:, 1]]) <= B[ours[:, 0], ours[:, 1]]).all()
        if topk == 0:
            dec = gen.mutual_decided(E, B)
            n_rows += m1
            n_undecided += int((~dec).sum())
            ref_of = {int(i): int(j) for i, j in ref[p]}
            our_of = {int(i): int(j) for i, j in ours}
            assert (np.diff(ours[:, 0]) > 0).all()
            for i in range(m1):
                if dec[i]:
                    assert our_of.get(i) == ref_of.get(i), (name, p, i)
            _, _, mand_r = gen.row_analysis(E, B, 1)
            _, _, mand_c = gen.row_analysis(E.T.copy(), B.T.copy(), 1)
            for i, j in ours:  # admissible: j can be the best column of i, i the best line of j
                assert not gen.forbidden_order(E, B, i, np.array([j, int(np.argmax(E[i]))]))
                assert not gen.forbidden_order(E.T, B.T, j, np.array([i, int(np.argmax(E[:, j]))]))
            continue
        k = min(topk, m2)
        assert ours.shape == (m1 * k, 2) == ref[p].shape
        assert np.array_equal(ours[:, 0], np.repeat(np.arange(m1), k))
        oc, rc = ours[:, 1].reshape(m1, k), ref[p][:, 1].reshape(m1, k)
        order, dec, mandatory = gen.row_analysis(E, B, k)
        n_rows += m1
        n_undecided += int((~dec).sum())
        assert np.array_equal(oc[dec], rc[dec]), (name, p)
        assert np.array_equal(oc[dec], order[dec, :k])
        for i in np.nonzero(~dec)[0]:
            cols = oc[i]
            assert len(set(cols.tolist())) == k and cols.min() >= 0 and cols.max() < m2
            assert set(mandatory[i].tolist()) <= set(cols.tolist()), (name, p, i)
            assert not gen.forbidden_order(E, B, i, cols), (name, p, i)
    assert n_undecided <= gen.MAX_UNDECIDED * max(n_rows, 1), (name, n_undecided, n_rows)


def test_equal_scores_rank_by_ascending_column():
    """exact ties (duplicate descriptors in image 2): ascending column index.  The reference leaves this open."""
    rng = np.random.default_rng(3)
    d1 = rng.standard_normal((20, 128)).astype(np.float32)
    base = rng.standard_normal((6, 128)).astype(np.float32)
    d2 = base[[0, 1, 0, 2, 1, 0, 3, 4, 5, 0]]  # column 0 = 2 = 5 = 9, 1 = 4
    rows, scores = matching.match_pair_host(d1, d2, "l2d2", 10, return_scores=True)
    cols, sc = rows[:, 1].reshape(20, 10), scores.reshape(20, 10)
    assert (np.diff(sc, axis=1) <= 0).all()
    for i in range(20):
        for t in range(9):
            if sc[i, t] == sc[i, t + 1]:
                assert cols[i, t] < cols[i, t + 1]
        pos = {int(c): t for t, c in enumerate(cols[i])}
        assert pos[0] + 1 == pos[2] and pos[2] + 1 == pos[5] and pos[5] + 1 == pos[9] and pos[1] + 1 == pos[4]
    # mutual NN: arg-max = first maximum, on both sides
    d = np.concatenate([base, base[:2]], 0)  # lines 6, 7 repeat lines 0, 1
    rows = matching.match_pair_host(d, d, "l2d2", 0)
    assert rows.tolist() == [[i, i] for i in range(6)]


def test_scores_are_the_fmaf_chain():
    rng = np.random.default_rng(4)
    a = rng.standard_normal((3, 16)).astype(np.float32)
    b = rng.standard_normal((4, 16)).astype(np.float32)
    rows, scores = matching.match_pair_host(a, b, "l2d2", 4, return_scores=True)
    for (i, j), s in zip(rows, scores):
        acc = np.float32(0.0)
        for k in range(16):  # fmaf: the product and the sum exact in float64 (24 + 24 + 24 bits fit), one rounding
            acc = np.float32(np.float64(a[i, k]) * np.float64(b[j, k]) + np.float64(acc))
        assert acc == s


def test_rejections_of_the_host_function():
    ok = np.ones((4, 128), np.float32)
    for bad in (np.full((4, 128), np.nan, np.float32), np.full((4, 128), np.inf, np.float32),
                np.full((4, 128), 2.0 ** 58, np.float32)):
        with pytest.raises(ValueError):
            matching.match_pair_host(bad, ok, "l2d2", 10)
    with pytest.raises(ValueError):
        matching.match_pair_host(ok, ok, "l2d2", -1)
    with pytest.raises(ValueError):
        matching.match_pair_host(ok, ok, "l2d2", matching.MAX_TOPK + 1)
    with pytest.raises(ValueError):
        matching.match_pair_host(np.ones((4, 12), np.float32), np.ones((4, 12), np.float32), "l2d2", 1)
    with pytest.raises(ValueError):
        matching.match_pair_host(np.ones((64, 3), np.float32), np.ones((64, 4), np.float32), "endpoints", 1)
    with pytest.raises(ValueError):
        matching.match_pair_host(ok, np.ones((4, 64), np.float32), "l2d2", 1)
    with pytest.raises(ValueError):
        matching.match_pair_host(np.ones((64, 4), np.float32), np.ones((64, 4), np.float32), "endpoints", 0)


def test_mirror_names_and_folder():
    m = matching.L2D2Matcher(None, matching.BaseMatcherOptions(topk=10, n_neighbors=20))
    assert m.get_module_name() == "l2d2" and m.get_matches_folder("out") == os.path.join("out", "l2d2_n20_top10")
    e = matching.NNEndpointsMatcher(None)
    assert e.get_module_name() == "nn_endpoints"
    for name in ("match_pair", "match_segs_with_descinfo", "match_segs_with_descinfo_topk", "match_all_neighbors",
                 "match_all_exhaustive_pairs", "get_matches_folder"):
        assert callable(getattr(m, name)) and callable(getattr(e, name))


def test_make_descriptors_shapes_and_correspondence():
    from limap_amd import synthetic as syn
    sc = syn.make_scene(n_views=4, n_segs=40, n_neighbors=2, seed=2)
    d = syn.make_descriptors(sc, "l2d2", noise=0.01, seed=1)
    e = syn.make_descriptors(sc, "endpoints", noise=0.01, seed=1)
    for k, i in enumerate(sc.img_ids):
        m = int(sc.seg_off[k + 1] - sc.seg_off[k])
        assert d[int(i)]["line_descriptors"].shape == (m, 128) and d[int(i)]["line_descriptors"].dtype == np.float32
        assert e[int(i)]["endpoints_desc"].shape == (256, 2 * m)
    # a GT segment seen in an image and in one of its neighbours: its line is the best match at low noise
    n_shared = 0
    for k0, i0 in enumerate(sc.img_ids):
        for i1 in sc.neighbors[int(i0)]:
            k1 = int(np.searchsorted(sc.img_ids, i1))
            g0, g1 = sc.gt_ids[sc.seg_off[k0]:sc.seg_off[k0 + 1]], sc.gt_ids[sc.seg_off[k1]:sc.seg_off[k1 + 1]]
            shared = [(i, int(np.nonzero(g1 == g)[0][0])) for i, g in enumerate(g0) if g >= 0 and (g1 == g).any()]
            n_shared += len(shared)
            for kind, di, key in (("l2d2", d, "line_descriptors"), ("endpoints", e, "endpoints_desc")):
                rows = matching.match_pair_host(di[int(i0)][key], di[int(i1)][key], kind, 1)
                assert all(rows[i, 1] == j for i, j in shared)
    assert n_shared > 0
