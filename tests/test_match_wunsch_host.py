"""The SOLD2 kind of limap_amd.matching, host side (no GPU): the restatement lt_fn_match_wunsch_pair_host against what
limap's own WunschLineMatcher returned for every fixture of tests/golden/match_wunsch (written by
tests/golden/make_match_wunsch_golden.py), against NumPy restatements of its pieces written here, and on the cases that
pin what DESIGN section 17 ("SOLD2") defines where upstream leaves it open.

Reference and restatement each sum an FP32 dot product in SOME order.  A top-k row whose best k line scores are
separated from every other by more than the two bounds is DECIDED and must equal the reference's row set exactly; a
line of the mutual form is decided when its candidate set is and its best Needleman-Wunsch value leads by more than the
bounds carried through the recurrence.  At most 10 % of a fixture's rows may be undecided."""
import glob
import importlib.util
import os

import numpy as np
import pytest

import wunsch_cases as wc
from limap_amd import io as limapio, matching

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_match_wunsch_golden",
                                               os.path.join(HERE, "golden", "make_match_wunsch_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(gen.OUT, "*.npz")))
EXPECTED = ["mutual_130_97", "mutual_33_47_64", "mutual_40_9", "mutual_empty", "top10_130_97", "top10_33_47",
            "top10_40_9", "top10_64_65", "top10_empty", "top1_17_16"]
F32 = np.float32


def test_every_fixture_is_there():
    assert FIXTURES == EXPECTED


# ---- (a) top-k against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in EXPECTED if not n.startswith("mutual")])
def test_topk_restatement_against_reference_rows(name):
    topk, S, kc, descs, pairs, ref = gen.load_fixture(os.path.join(gen.OUT, name + ".npz"))
    n_rows = n_undecided = 0
    for p, (a, b) in enumerate(pairs):
        m1, m2 = descs[a][1].shape[0], descs[b][1].shape[0]
        ours, scores = matching.match_pair_host(descs[a], descs[b], "sold2", topk, return_scores=True, num_samples=S)
        assert ours.dtype == np.int32 and ours.shape[1:] == (2,)
        if m1 == 0 or m2 == 0:
            assert ours.shape == (0, 2) and ref[p].shape == (0, 2)
            continue
        E, B = gen.exact_line_scores(*gen.exact_point_scores(descs[a], descs[b], S))
        # the reported score is within the bound of the exact one
        assert (np.abs(scores.astype(np.float64) - E[ours[:, 0], ours[:, 1]]) <= B[ours[:, 0], ours[:, 1]]).all()
        k = min(topk, m2)
        assert ours.shape == (m1 * k, 2) == ref[p].shape
        assert np.array_equal(ours[:, 0], np.repeat(np.arange(m1), k))  # lines ascending, best first within a line
        oc = ours[:, 1].reshape(m1, k)
        rc = ref[p][:, 1].reshape(k, m1).T[:, ::-1]  # upstream: rank blocks, ascending -> (line, best first)
        assert np.array_equal(ref[p][:, 0], np.tile(np.arange(m1), k))
        order, dec, mandatory = gen.base.row_analysis(E, B, k)
        n_rows += m1
        n_undecided += int((~dec).sum())
        assert np.array_equal(oc[dec], rc[dec]), (name, p)
        assert np.array_equal(oc[dec], order[dec, :k])
        for i in np.nonzero(~dec)[0]:
            cols = oc[i]
            assert len(set(cols.tolist())) == k and cols.min() >= 0 and cols.max() < m2
            assert set(mandatory[i].tolist()) <= set(cols.tolist()), (name, p, i)
            assert not gen.base.forbidden_order(E, B, i, cols), (name, p, i)
    assert n_undecided <= gen.MAX_UNDECIDED * max(n_rows, 1), (name, n_undecided, n_rows)


# ---- (c) the mutual form against the reference -----------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in EXPECTED if n.startswith("mutual")])
def test_mutual_restatement_against_reference_matches(name):
    topk, S, kc, descs, pairs, ref = gen.load_fixture(os.path.join(gen.OUT, name + ".npz"))
    assert topk == 0
    n_rows = n_undecided = 0
    for p, (a, b) in enumerate(pairs):
        m1, m2 = descs[a][1].shape[0], descs[b][1].shape[0]
        ours = matching.match_pair_host(descs[a], descs[b], "sold2", 0, num_samples=S, top_k_candidates=kc)
        assert ours.dtype == np.int32 and ours.shape[1:] == (2,)
        if m1 == 0 or m2 == 0:
            assert ours.shape == (0, 2) and ref[p].shape == (0, 2)
            continue
        assert (np.diff(ours[:, 0]) > 0).all() and ours[:, 1].min() >= 0 and ours[:, 1].max() < m2
        assert len(set(ours[:, 1].tolist())) == len(ours)  # a cross-checked match is one to one
        exact, dec = gen.mutual_analysis(descs[a], descs[b], S, kc)
        ref_of = {int(i): int(j) for i, j in ref[p]}
        our_of = {int(i): int(j) for i, j in ours}
        n_rows += m1
        n_undecided += int((~dec).sum())
        for i in np.nonzero(dec)[0]:
            assert our_of.get(int(i), -1) == ref_of.get(int(i), -1) == int(exact[i]), (name, p, i)
    assert n_undecided <= gen.MAX_UNDECIDED * max(n_rows, 1), (name, n_undecided, n_rows)


# ---- NumPy restatements of the pieces -------------------------------------------------------------------------------
def np_point_scores(d1, d2, S):
    """P (N1, N2, S, S): the fmaf chain in ascending k from +0.0f -- product and sum exact in float64 (24 + 24 + 24 bits
    fit), one rounding to FP32 per step -- and -1 where either sample is masked"""
    a, b = np.asarray(d1[0], F32).T, np.asarray(d2[0], F32).T  # (S N, K)
    acc = np.zeros((a.shape[0], b.shape[0]), F32)
    for k in range(a.shape[1]):
        acc = (a[:, k, None].astype(np.float64) * b[None, :, k].astype(np.float64) + acc.astype(np.float64)).astype(F32)
    ok = np.asarray(d1[1], bool).reshape(-1)[:, None] & np.asarray(d2[1], bool).reshape(-1)[None, :]
    acc[~ok] = F32(-1.0)
    n1, n2 = d1[1].shape[0], d2[1].shape[0]
    return np.ascontiguousarray(acc.reshape(n1, S, n2, S).transpose(0, 2, 1, 3))


def np_line_scores(P):
    """L (N1, N2) from P (N1, N2, S, S) in FP32: the maxima, the means of those that are not -1 with the sum as the
    fixed tree over 8 slots (absent terms +0.0f), -1 for a mean without terms, the sum of the two, the halving"""
    def pool(m):  # (N1, N2, S)
        S = m.shape[2]
        t = np.zeros(m.shape[:2] + (8,), F32)
        t[..., :S] = np.where(m != F32(-1.0), m, F32(0.0))
        cnt = (m != F32(-1.0)).sum(2)
        tree = ((t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])) + ((t[..., 4] + t[..., 5]) + (t[..., 6] + t[..., 7]))
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = tree / cnt.astype(F32)
        return np.where(cnt > 0, mean, F32(-1.0)).astype(F32)
    return ((pool(P.max(3)) + pool(P.max(2))) * F32(0.5)).astype(F32)


def np_mutual(P, L, kc):
    """filter_and_match_lines + the cross check in NumPy under the total order: candidates ascending in (L, -column),
    forward blocks before reversed ones, first maximum"""
    def one_side(P, L):
        n1, n2 = L.shape
        k = min(kc, n2)
        out = np.zeros(n1, np.int64)
        for i in range(n1):
            best_first = sorted(range(n2), key=lambda j: (-float(L[i, j]), j))[:k]
            cand = best_first[::-1]
            blocks = [P[i, j] for j in cand] + [P[i, j][:, ::-1] for j in cand]
            nw = np.array([gen.nw_value((blk - F32(0.1)).astype(np.float64)) for blk in blocks])
            out[i] = cand[int(np.argmax(nw)) % k]
        return out
    f = one_side(P, L)
    b = one_side(np.ascontiguousarray(P.transpose(1, 0, 3, 2)), np.ascontiguousarray(L.T))
    keep = b[f] == np.arange(len(f))
    return np.stack([np.arange(len(f))[keep], f[keep]], 1).astype(np.int32)


def _small_pairs():
    rng = np.random.default_rng(5)
    yield wc.rand_descinfo(rng, 9, 5, 32), wc.rand_descinfo(rng, 14, 5, 32), 5
    yield wc.rand_descinfo(rng, 7, 2, 8, prefix=False), wc.rand_descinfo(rng, 5, 2, 8, prefix=False), 2
    yield wc.rand_descinfo(rng, 6, 8, 16, prefix=False), wc.rand_descinfo(rng, 13, 8, 16, prefix=False), 8
    for name in ("antipodal", "masks_S5"):
        a, b, S, _, _ = wc.definition_case(name)
        yield a, b, S


def test_point_and_line_scores_are_the_defined_bits():
    for a, b, S in _small_pairs():
        P, L = matching.wunsch_scores_host(a, b, S)
        Pn = np_point_scores(a, b, S)
        assert np.array_equal(wc.bits(P), wc.bits(Pn))
        assert np.array_equal(wc.bits(L), wc.bits(np_line_scores(Pn)))
        # the swapped pair sees the same bits: products commute, and both pooled sides use the same tree
        Pt, Lt = matching.wunsch_scores_host(b, a, S)
        assert np.array_equal(wc.bits(Pt), wc.bits(P.transpose(1, 0, 3, 2))) and np.array_equal(wc.bits(Lt), wc.bits(L.T))


# ---- (b) NW on the restatement's own score bits ------------------------------------------------------------------------
def test_nw_values_argmax_and_cross_check_equal_numpy():
    for a, b, S in _small_pairs():
        P, L = matching.wunsch_scores_host(a, b, S)
        for blk in P.reshape(-1, S, S)[::3]:
            got = matching.wunsch_nw_host(blk)
            w = (blk - F32(0.1)).astype(np.float64)  # the subtraction in FP32, widened exactly
            want = np.array([gen.nw_value(w), gen.nw_value(w[:, ::-1])])
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        for kc in (1, 3, 10):
            ours = matching.match_pair_host(a, b, "sold2", 0, num_samples=S, top_k_candidates=kc)
            assert np.array_equal(ours, np_mutual(P, L, kc)), (S, kc)
        for topk in (1, 4, 64):  # and the top-k rows are the order of the key on the same bits
            rows, sc = matching.match_pair_host(a, b, "sold2", topk, return_scores=True, num_samples=S)
            k = min(topk, L.shape[1])
            want = np.array([sorted(range(L.shape[1]), key=lambda j: (-float(L[i, j]), j))[:k] for i in range(L.shape[0])])
            assert np.array_equal(rows[:, 1].reshape(-1, k), want)
            assert np.array_equal(wc.bits(sc).reshape(-1, k), wc.bits(np.take_along_axis(L, want, 1)))


# ---- (d) the definitions -----------------------------------------------------------------------------------------------
def test_equal_scores_rank_by_ascending_line():
    a, b, S, topk, kc = wc.definition_case("ties")
    rows, sc = matching.match_pair_host(a, b, "sold2", topk, return_scores=True)
    cols, s = rows[:, 1].reshape(-1, topk), sc.reshape(-1, topk)
    assert (np.diff(s, axis=1) <= 0).all()
    eq = s[:, :-1] == s[:, 1:]
    assert eq.sum() > 20 and (cols[:, :-1][eq] < cols[:, 1:][eq]).all()
    P, L = matching.wunsch_scores_host(a, b, S)
    assert np.array_equal(matching.match_pair_host(a, b, "sold2", 0), np_mutual(P, L, kc))
    # identical images: every line is its own first maximum although its duplicates tie with it
    d = [np.concatenate([b[0], b[0][:, :10]], 1), np.concatenate([b[1], b[1][:2]], 0)]
    P, L = matching.wunsch_scores_host(d, d, S)
    assert np.array_equal(matching.match_pair_host(d, d, "sold2", 0), np_mutual(P, L, kc))


def test_a_valid_score_of_minus_one_is_dropped_and_an_all_minus_one_block_scores_minus_one():
    a, b, S, topk, kc = wc.definition_case("antipodal")
    P, L = matching.wunsch_scores_host(a, b, S)
    assert P[0, 0].tolist() == [[-1.0, -1.0], [0.0, -1.0]]  # (e0, e1) against (-e0, padded): -1 valid, -1 masked
    assert P[1, 0].tolist() == [[-1.0, -1.0], [-1.0, -1.0]]  # (e0, padded) against (-e0, padded)
    # line 0 / line 0: max over t = (-1 dropped, 0) -> 0 / 1; max over s = (0, -1 dropped) -> 0 / 1; L = 0, where a
    # counted -1 would give (-1 + 0) / 2
    assert L[0, 0] == 0.0 and L[1, 0] == -1.0
    assert P[0, 1].tolist() == [[0.0, 1.0], [1.0, 0.0]] and L[0, 1] == 1.0
    rows, sc = matching.match_pair_host(a, b, "sold2", topk, return_scores=True, num_samples=S)
    assert rows.tolist() == [[0, 1], [0, 0], [1, 1], [1, 0]] and sc.tolist() == [1.0, 0.0, 0.75, -1.0]
    assert matching.match_pair_host(a, b, "sold2", 0, num_samples=S).tolist() == np_mutual(P, L, kc).tolist()


@pytest.mark.parametrize("name", [n for n in wc.DEFINITION_CASES if n.startswith("below")])
def test_real_scores_below_minus_one_are_terms_of_the_means(name):
    """descriptors that are not unit vectors: only a maximum EQUAL to -1.0f is dropped; one below it counts, and the
    maxima run over the S real samples only (on the device no padded slot's -1.0f may take its place)"""
    a, b, S, topk, kc = wc.definition_case(name)
    P, L = matching.wunsch_scores_host(a, b, S)
    Pn = np_point_scores(a, b, S)
    assert np.array_equal(wc.bits(P), wc.bits(Pn)) and np.array_equal(wc.bits(L), wc.bits(np_line_scores(Pn)))
    assert (P[0, 0] == -2.0).all() and L[0, 0] == -2.0  # 2 e0 in every sample against -e0 in every sample
    low = P[1:, 1:8]  # behind the example: every real score against lines 1 .. 7 is far below -1
    assert (low[low != -1.0] < -1.5).all()
    if not name.endswith("masked"):  # ... and so is every maximum and every line score; the last lines score high
        assert (P != -1.0).all() and (L[1:, 1:8] < -1.5).all() and (L[1:, 8:] > 1.5).all()
    else:  # a masked -1.0f beats a real score below it in a maximum, as upstream: such a maximum is dropped
        assert (L[1:, 1:8] <= -1.0).all()
    assert np.array_equal(matching.match_pair_host(a, b, "sold2", 0, num_samples=S), np_mutual(P, L, kc))
    rows, sc = matching.match_pair_host(a, b, "sold2", topk, return_scores=True, num_samples=S)
    want = np.array([sorted(range(L.shape[1]), key=lambda j: (-float(L[i, j]), j))[:topk] for i in range(L.shape[0])])
    assert np.array_equal(rows[:, 1].reshape(-1, topk), want)
    assert np.array_equal(wc.bits(sc).reshape(-1, topk), wc.bits(np.take_along_axis(L, want, 1)))


def test_fewer_lines_than_topk_and_than_candidates():
    a, b, S, topk, kc = wc.definition_case("few_lines")
    rows = matching.match_pair_host(a, b, "sold2", topk)
    assert rows.shape == (19 * 3, 2) and np.array_equal(rows[:, 0], np.repeat(np.arange(19), 3))
    assert all(sorted(r) == [0, 1, 2] for r in rows[:, 1].reshape(19, 3).tolist())
    P, L = matching.wunsch_scores_host(a, b, S)
    assert np.array_equal(matching.match_pair_host(a, b, "sold2", 0), np_mutual(P, L, kc))
    assert np.array_equal(matching.match_pair_host(b, a, "sold2", 0),
                          np_mutual(np.ascontiguousarray(P.transpose(1, 0, 3, 2)), np.ascontiguousarray(L.T), kc))
    empty = wc.rand_descinfo(np.random.default_rng(1), 0)
    for topk in (0, 10):
        assert matching.match_pair_host(a, empty, "sold2", topk).shape == (0, 2)
        assert matching.match_pair_host(empty, a, "sold2", topk).shape == (0, 2)
        assert matching.match_pair_host([], a, "sold2", topk).shape == (0, 2)


@pytest.mark.parametrize("name", ["masks_S2", "masks_S5", "masks_S8"])
def test_arbitrary_masks_and_sample_counts(name):
    a, b, S, topk, kc = wc.definition_case(name)
    assert not all((np.diff(v.astype(int), axis=1) <= 0).all() for v in (a[1], b[1]))  # not prefixes
    P, L = matching.wunsch_scores_host(a, b, S)
    Pn = np_point_scores(a, b, S)
    assert np.array_equal(wc.bits(P), wc.bits(Pn)) and np.array_equal(wc.bits(L), wc.bits(np_line_scores(Pn)))
    masked = ~(a[1][:, None, :, None] & b[1][None, :, None, :])
    assert (P[masked] == -1.0).all() and (P[~masked] != -1.0).all()
    assert np.array_equal(matching.match_pair_host(a, b, "sold2", 0, num_samples=S), np_mutual(P, L, kc))
    # the padded samples' descriptors do not matter
    a2 = [a[0].copy(), a[1]]
    a2[0][:, ~a[1].reshape(-1)] = 7.0
    for topk in (0, 10):
        assert np.array_equal(matching.match_pair_host(a, b, "sold2", topk, num_samples=S),
                              matching.match_pair_host(a2, b, "sold2", topk, num_samples=S))


def test_rejections_of_the_host_function():
    rng = np.random.default_rng(2)
    ok = wc.rand_descinfo(rng, 4)
    for v in (np.nan, np.inf, 2.0 ** 58):
        bad = [ok[0].copy(), ok[1]]
        bad[0][3, 7] = v
        with pytest.raises(ValueError):
            matching.match_pair_host(bad, ok, "sold2", 10)
    for kw in (dict(topk=-1), dict(topk=matching.MAX_TOPK + 1), dict(topk=0, top_k_candidates=0),
               dict(topk=0, top_k_candidates=matching.MAX_TOPK + 1)):
        with pytest.raises(ValueError):
            matching.match_pair_host(ok, ok, "sold2", **kw)
    for S in (1, 9):
        w = [np.ones((128, 4 * S), np.float32), np.ones((4, S), bool)]
        with pytest.raises(ValueError):
            matching.match_pair_host(w, w, "sold2", 10, num_samples=S)
    w = [np.ones((12, 20), np.float32), np.ones((4, 5), bool)]
    with pytest.raises(ValueError):
        matching.match_pair_host(w, w, "sold2", 10)
    none_valid = [ok[0], ok[1].copy()]
    none_valid[1][1, :] = False
    with pytest.raises(ValueError):
        matching.match_pair_host(ok, none_valid, "sold2", 10)
    with pytest.raises(ValueError, match="columns per line"):
        matching.match_pair_host(ok, [ok[0][:, :19], ok[1]], "sold2", 10)
    with pytest.raises(ValueError, match="num_samples"):
        matching.match_pair_host(ok, ok, "sold2", 10, num_samples=4)
    with pytest.raises(ValueError, match="widths differ"):
        matching.match_pair_host(ok, wc.rand_descinfo(rng, 4, 5, 64), "sold2", 10)


# ---- (e) the Python surface ---------------------------------------------------------------------------------------------
def test_mirror_names_folder_and_what_is_not_built():
    m = matching.SOLD2Matcher(None, matching.BaseMatcherOptions(topk=10, n_neighbors=20))
    assert m.get_module_name() == "sold2" and m.get_matches_folder("out") == os.path.join("out", "sold2_n20_top10")
    assert m.num_samples == 5 and m.top_k_candidates == 10 and matching.KINDS["sold2"] == matching.SOLD2Matcher.KIND
    for name in ("match_pair", "match_segs_with_descinfo", "match_segs_with_descinfo_topk", "match_all_neighbors",
                 "match_all_exhaustive_pairs", "match_scene", "get_matches_folder"):
        assert callable(getattr(m, name))
    with pytest.raises(NotImplementedError, match="cross_check"):
        matching.SOLD2Matcher(None, cross_check=False)
    for sampling in ("d2_net", "asl_feat"):
        with pytest.raises(NotImplementedError, match=sampling):
            matching.SOLD2Matcher(None, sampling=sampling)
    with pytest.raises(ValueError, match="Wrong sampling mode"):
        matching.SOLD2Matcher(None, sampling="other")
    with pytest.raises(NotImplementedError, match="compute_descriptors"):
        m.compute_descriptors(None, None)
    with pytest.raises(NotImplementedError, match="get_pairwise_distance"):
        m.get_pairwise_distance(None, None, None, None)
    with pytest.raises(ValueError, match="positive"):
        m.match_segs_with_descinfo_topk([], [], topk=0)


def test_descinfo_forms_and_the_object_array_round_trip(tmp_path):
    """list, tuple, and what SOLD2Detector.save_descinfo writes: an object array with a leading axis on valid"""
    rng = np.random.default_rng(8)
    a, b = wc.rand_descinfo(rng, 11), wc.rand_descinfo(rng, 6)
    want = matching.match_pair_host(a, b, "sold2", 10)
    assert np.array_equal(matching.match_pair_host(tuple(a), tuple(b), "sold2", 10), want)
    for k, d in enumerate((a, b)):
        limapio.save_npy(str(tmp_path / f"descinfo_{k}.npy"), [d[0], d[1][None, :]])
    ra, rb = (limapio.read_npy(str(tmp_path / f"descinfo_{k}.npy")) for k in range(2))
    assert ra.dtype == object and ra[1].shape == (1, 11, 5)
    assert np.array_equal(matching.match_pair_host(ra, rb, "sold2", 10), want)
    ra[1] = ra[1][0]  # what read_descinfo hands to the matcher
    assert np.array_equal(matching.match_pair_host(ra, rb, "sold2", 10), want)
    limapio.save_npy(str(tmp_path / "descinfo_2.npy"), [])  # an image without lines
    assert matching.match_pair_host(limapio.read_npy(str(tmp_path / "descinfo_2.npy")), rb, "sold2", 10).shape == (0, 2)


def test_make_descriptors_sold2_shapes_and_correspondence():
    from limap_amd import synthetic as syn
    sc = syn.make_scene(n_views=4, n_segs=30, n_neighbors=2, seed=6)
    di = syn.make_descriptors(sc, "sold2", noise=0.01, seed=1)
    for k, i in enumerate(sc.img_ids):
        d, v = di[int(i)]
        n = int(sc.seg_off[k + 1] - sc.seg_off[k])
        assert d.shape == (128, 5 * n) and d.dtype == np.float32 and v.shape == (n, 5) and v.dtype == bool
        assert (v.sum(1) >= 2).all() and (np.diff(v.astype(int), axis=1) <= 0).all()
        assert np.allclose(np.linalg.norm(d, axis=0), 1.0, atol=1e-5)
