"""The dense kind of limap_amd.matching without a device ("Dense"): the host restatement
lt_fn_match_dense_pair_host / lt_fn_match_dense_dists_host against what limap's own BaseDenseLineMatcher returned for
the fixtures of tests/golden/match_dense -- rows on the decided entries, distances and overlaps within the rounding
bound -- the values exactly on the thresholds, the rejections, the Python surface and the sanitizer program."""
import ctypes as C
import glob
import importlib.util
import os

import numpy as np
import pytest

import dense_cases as dc
from limap_amd import _capi, matching

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "match_dense")
_spec = importlib.util.spec_from_file_location("make_match_dense_golden",
                                               os.path.join(HERE, "golden", "make_match_dense_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "*.npz")))
CONSTRUCTED = {"zero_length_12_12", "tie_10_12", "empty_0_9", "empty_9_0"}


def _inputs(fx, one_to_many=False):
    a = dc.descinfo(fx["lines1"], fx["shape1"])
    b = dc.descinfo(fx["lines2"], fx["shape2"])
    opts = matching.BaseDenseLineMatcherOptions(n_samples=fx["n_samples"], pixel_th=fx["pixel_th"],
                                                segment_percentage_th=fx["segment_percentage_th"],
                                                one_to_many=one_to_many)
    return a, b, (fx["warp12"], fx["cert12"], fx["warp21"], fx["cert21"]), opts, fx["sample_thresh"]


def test_the_fixtures_are_there():
    assert len(FIXTURES) == 8 and CONSTRUCTED <= set(FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("one_to_many", [False, True])
def test_rows_equal_upstream_on_decided_entries(name, one_to_many):
    fx = gen.load_fixture(os.path.join(GOLD, name + ".npz"))
    n1, n2 = fx["lines1"].shape[0], fx["lines2"].shape[0]
    match, dec, _ = gen.pair_analysis(fx, one_to_many)
    share = float((~dec).mean()) if dec.size else 0.0
    assert share <= gen.MAX_UNDECIDED
    if name in CONSTRUCTED:
        assert share == 0.0
    ref = gen.rows_to_mask(fx["ref_many" if one_to_many else "ref_one"], n1, n2)
    rows = matching.match_dense_pair_host(*_inputs(fx, one_to_many))
    assert rows.dtype == np.int32 and rows.shape[1:] == (2,)
    assert np.array_equal(rows, rows[np.lexsort((rows[:, 1], rows[:, 0]))])  # torch.nonzero's order
    got = gen.rows_to_mask(rows, n1, n2)
    assert np.array_equal(got[dec], ref[dec])
    assert np.array_equal(got[dec], match[dec])
    if share == 0.0:
        assert np.array_equal(rows, fx["ref_many" if one_to_many else "ref_one"])
    if name == "tie_10_12" and not one_to_many:  # both identical target lines are kept
        assert got[2, 2] and got[2, 10] and got[7, 7] and got[7, 11]


@pytest.mark.parametrize("name", FIXTURES)
def test_distances_and_overlaps_within_the_bound_of_upstream(name):
    fx = gen.load_fixture(os.path.join(GOLD, name + ".npz"))
    _, _, r = gen.pair_analysis(fx, True)
    d12, o12, d21, o21, dists = matching.match_dense_dists_host(*_inputs(fx))
    for mine_d, mine_o, ref_d, ref_o, e, f, k, ex_d, ex_o in (
            (d12, o12, fx["ref_d12"], fx["ref_o12"], r["e12"], r["f12"], r["k12"], r["d12"], r["o12"]),
            (d21, o21, fx["ref_d21"], fx["ref_o21"], r["e21"], r["f21"], r["k21"], r["d21"], r["o21"])):
        assert mine_d.shape == ref_d.shape == ex_d.shape
        # the overlap is a count over S: exactly equal wherever every sample flag of the entry is decided
        assert np.array_equal(dc.bits(mine_o[f]), dc.bits(ref_o[f]))
        assert np.array_equal(mine_o[f], ex_o[f].astype(np.float32))
        # the distance: within the bound of the float64 value, upstream's and the restatement's alike (decided
        # entries: the jump to 10000 is on the same side for all three)
        assert np.all(np.abs(mine_d[k] - ex_d[k]) <= e[k] + 1e-6 * np.abs(ex_d[k]))
        assert np.all(np.abs(ref_d[k] - ex_d[k]) <= e[k] + 1e-6 * np.abs(ex_d[k]))
        assert np.all(np.abs(mine_d[k] - ref_d[k]) <= 2 * e[k] + 2e-6 * np.abs(ex_d[k]))


@pytest.mark.parametrize("name", dc.THRESHOLD_CASES)
def test_values_on_the_thresholds(name):
    a, b, warps, o, thresh, want = dc.threshold_case(name)
    opts = matching.BaseDenseLineMatcherOptions(**o)
    rows, sc = matching.match_dense_pair_host(a, b, warps, opts, thresh, return_scores=True)
    assert np.array_equal(rows, want), name
    d12, o12, d21, o21, dists = matching.match_dense_dists_host(a, b, warps, opts, thresh)
    if name.startswith("overlap"):
        assert dc.bits(o12)[0, 0] == dc.bits(np.float32(0.2))
    if name == "dists_equal":
        assert dists[0, 0] == 10.0 and sc[0] == 10.0
    if name == "dmax_equal":
        assert d12[0, 0] == 10.0 and dists[0, 0] == 0.5


def _raw_call(n_samples=21, dims12=(2, 2, 2, 2), shape1=(48, 64), pixel_th=10.0):
    L = _capi.load_library()
    l = np.array([[1, 2, 30, 20]], np.float32)
    w, c = np.zeros((2, 2, 2), np.float32), np.zeros((2, 2), np.float32)
    cfg = _capi.LtMatchDenseConfig(n_samples, 0, 0.2, pixel_th, 0.5, 0, 0, 0)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    f = lambda a: a.ctypes.data_as(fp)
    i = lambda v: np.array(v, np.int32).ctypes.data_as(ip)
    n = C.c_int64(-1)
    return L.lt_fn_match_dense_pair_host(f(l), 1, i(shape1), f(l), 1, i((48, 64)), f(w), f(c), i(dims12), f(w), f(c),
                                         i((2, 2, 2, 2)), C.byref(cfg), None, None, C.byref(n)), n.value


def test_rejections():
    assert _raw_call() == (0, 0)
    assert _raw_call(n_samples=1)[0] != 0
    assert _raw_call(n_samples=65)[0] != 0
    assert _raw_call(n_samples=64)[0] == 0 and _raw_call(n_samples=2)[0] == 0
    assert _raw_call(dims12=(0, 2, 0, 2))[0] != 0
    assert _raw_call(dims12=(2, 2, 2, 3))[0] != 0
    assert _raw_call(shape1=(0, 64))[0] != 0
    assert _raw_call(shape1=(48, -1))[0] != 0
    assert _raw_call(pixel_th=float("nan"))[0] != 0
    a, b, warps, o, thresh, _ = dc.threshold_case("plain")
    with pytest.raises(ValueError):
        matching.match_dense_pair_host(a, b, warps, matching.BaseDenseLineMatcherOptions(n_samples=65), thresh)
    with pytest.raises(ValueError):
        matching.match_dense_pair_host(a, b, (warps[0], warps[1][:3], warps[2], warps[3]),
                                       matching.BaseDenseLineMatcherOptions(), thresh)
    with pytest.raises(ValueError):
        matching.match_dense_pair_host(a, b, warps[:3], matching.BaseDenseLineMatcherOptions(), thresh)


def test_python_surface(tmp_path):
    o = matching.DefaultDenseLineMatcherOptions
    assert (o.n_samples, o.segment_percentage_th, o.device, o.pixel_th, o.one_to_many) == (21, 0.2, "cuda", 10.0, False)
    assert matching.BaseDenseLineMatcherOptions(device="cpu").device == "cpu"
    assert matching.KINDS["dense"] == matching.KINDS["dense_roma"] == matching.DENSE

    class Cam:
        def read_image(self):
            return np.zeros((48, 64, 3), np.uint8)

    ex = matching.DenseNaiveExtractor()
    assert ex.get_module_name() == "dense_naive"
    segs = np.array([[1.0, 2.0, 4.0, 6.0, 0.5], [0.0, 0.0, 0.0, 9.0, 2.0]])
    d = ex.extract(Cam(), segs)
    assert d["image_shape"] == (48, 64, 3) and d["lines"].shape == (2, 2, 2)
    assert np.allclose(d["scores"], [0.5 * np.sqrt(5.0), 2.0 * 3.0])
    ex.save_descinfo(str(tmp_path), 7, d)
    assert os.path.exists(os.path.join(str(tmp_path), "descinfo_7.npz"))
    back = ex.read_descinfo(str(tmp_path), 7)
    assert sorted(back) == ["image", "image_shape", "lines", "scores"]
    assert np.array_equal(back["lines"], d["lines"]) and tuple(back["image_shape"]) == (48, 64, 3)

    bm = matching.BaseDenseMatcher()
    xy = np.array([[0.0, 0.0], [64.0, 48.0], [32.0, 12.0]])
    nrm = bm.to_normalized_coordinates(xy, 48, 64)
    assert np.allclose(nrm, [[-1, -1], [1, 1], [0, -0.5]])
    assert np.allclose(bm.to_unnormalized_coordinates(nrm, 48, 64), xy)
    with pytest.raises(NotImplementedError):
        bm.get_sample_thresh()
    with pytest.raises(NotImplementedError):
        bm.get_warping_symmetric(None, None)

    with pytest.raises(ImportError, match="romatch"):
        matching.RoMaLineMatcher(ex)
    with pytest.raises(ValueError, match="match_scene_dense"):
        matching.match_scene({}, {}, kind="dense")
    with pytest.raises(ValueError, match="match_scene_dense"):
        matching.match_scene({}, {}, kind="dense_roma")
    with pytest.raises(TypeError):
        matching.DenseLineMatcher(ex, object())
    with pytest.raises(ValueError):
        matching.match_scene_dense({}, {}, lambda i, j: None)  # no threshold and nobody to ask
    m = matching.DenseLineMatcher(ex, bm)
    assert m.get_module_name() == "dense" and m.check_compatibility(ex)
    for name in ("match_pair", "match_segs_with_descinfo", "match_segs_with_descinfo_topk",
                 "compute_distance_one_direction", "match_all_neighbors", "match_all_exhaustive_pairs"):
        assert callable(getattr(m, name))


def test_sanitizer_program_of_the_host_restatement():
    """tools/dense_host_asan.cpp + lt_match_dense.cpp under AddressSanitizer and UBSan, a program of its own"""
    from helpers import run_host_asan
    run_host_asan("dense_asan", "dense_host_asan")
