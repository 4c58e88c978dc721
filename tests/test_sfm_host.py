"""limap_amd.pointsfm without a GPU: the library's host path (lt_fn_sfm_neighbors_host, lt_fn_sfm_ranges) equals
tests/sfm_oracle.py -- a NumPy restatement of DESIGN.md section 21 -- on every case family of tests/sfm_cases.py:
exactly on neighbour lists, shared points, ComputeNumPoints and ranges; angles equal as float32 or one ulp apart
(the library evaluates its own arccosine, the oracle NumPy's).  Known answers worked out by hand; the Python surface."""
import os

import numpy as np
import pytest

import sfm_cases as sc
import sfm_oracle as so

KINDS = ("overlap", "iou", "dice")
CASES = {
    "no_points": sc.no_points, "degenerate": sc.degenerate, "single_image": sc.single_image,
    "all_skipped": sc.all_skipped, "percentile": sc.percentile, "landmark": sc.landmark,
    "slot_below": lambda: sc.slot_boundary(-1), "slot_on": lambda: sc.slot_boundary(0),
    "slot_above": lambda: sc.slot_boundary(1), "tie_ring": sc.tie_ring, "star64": lambda: sc.star(64),
    "star65": lambda: sc.star(65), "star200": lambda: sc.star(200), "all_gated": sc.all_gated,
    "star_mixed": lambda: sc.star(100, coincident=37),
    "repeated_negative": sc.repeated_negative, "repeated_infinite": sc.repeated_infinite,
}
CASES.update({f"random{s}": (lambda s=s: sc.random_model(s)) for s in range(20)})
NUM_IMAGES = {"tie_ring": (0, 1, 3, 4, 100), "star64": (20, 150), "star65": (20, 150), "star200": (20, 150),
              "star_mixed": (150,), "landmark": (20,)}


def build(case):
    from limap_amd import pointsfm
    return pointsfm.SfmModel.from_arrays(*sc.to_arrays(case))


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_path_equals_the_oracle(gpu_lib, name):
    from limap_amd import pointsfm
    case = CASES[name]()
    mod = build(case)
    table = case["table"]
    assert mod.ComputeNumPoints() == so.num_points(case)
    ij, shared, angle = mod.pair_records(host=True)
    assert np.array_equal(ij, table[0]) and np.array_equal(shared, table[1])
    assert angle.dtype == np.float32 and (ulps(angle, table[2]) <= 1).all()
    if len(case["img_ids"]) <= 64:
        assert mod.ComputeSharedPoints(host=True) == so.shared_points(case, table)
    for num_images in NUM_IMAGES.get(name, (1 + len(name) % 7,)):
        for kind in KINDS:
            got = pointsfm.compute_neighbors(mod, num_images, sc.GATE_DEG, kind, host=True)
            want = so.neighbors(case, num_images, sc.GATE_DEG, kind, table)
            assert got == want and list(got) == list(want), (kind, num_images)


def test_hand_built_known_answer(gpu_lib):
    from limap_amd import pointsfm
    case, expect = sc.hand_built()
    mod = build(case)
    assert mod.ComputeNumPoints() == expect["num_points"]
    assert mod.ComputeSharedPoints(host=True) == expect["shared"]
    ij, shared, angle = mod.pair_records(host=True)
    th = float(so.gate_threshold(1.0))
    gated = [tuple(p) for p, a in zip(ij.tolist(), angle.tolist()) if a < th]
    assert gated == [(0, 3)] and angle[ij.tolist().index([0, 3])] < 0.00025  # 1 mm at 5 m
    for kind in KINDS:
        assert pointsfm.compute_neighbors(mod, 20, 1.0, kind, host=True) == expect[kind]
        assert so.neighbors(case, 20, 1.0, kind) == expect[kind]
    assert mod.GetMaxIoUImages(2, 1.0, host=True) == {1: [3], 3: [8, 5], 5: [3, 8], 8: [3, 5]}
    assert mod.GetMaxOverlapImages(1, 1.0, host=True) == {1: [3], 3: [5], 5: [3], 8: [3]}
    assert mod.GetMaxDiceCoeffImages(0, 1.0, host=True) == {1: [], 3: [], 5: [], 8: []}


def test_repeated_images_give_negative_and_infinite_iou(gpu_lib):
    """[0, 0, 0, 1, 1, 2]: shared (0,1) 6, (0,2) 3, (1,2) 2 and n = 3, 2, 1.  IoU (0,1) = 6 / -1, (0,2) = 3 / 1,
    (1,2) = 2 / 1: image 0 ranks 2 before 1, image 1 ranks 2 before 0.  [0, 0, 1, 1, 2]: IoU (0,1) = 4 / 0 = +inf"""
    from limap_amd import pointsfm
    mod = build(sc.repeated_negative())
    assert mod.ComputeSharedPoints(host=True)[:3] == [{1: 6, 2: 3}, {0: 6, 2: 2}, {0: 3, 1: 2}]
    assert pointsfm.compute_neighbors(mod, 5, 1.0, "iou", host=True) == {0: [2, 1], 1: [2, 0], 2: [0, 1], 3: [4], 4: [3]}
    assert pointsfm.compute_neighbors(mod, 1, 1.0, "overlap", host=True) == {0: [1], 1: [0], 2: [0], 3: [4], 4: [3]}
    mod = build(sc.repeated_infinite())
    assert pointsfm.compute_neighbors(mod, 1, 1.0, "iou", host=True) == {0: [1], 1: [0], 2: [0], 3: [4], 4: [3]}


def test_non_finite_projection_centre_is_refused(gpu_lib):
    from limap_amd import pointsfm
    big = 3e38  # finite in float32, R^T T is not
    mod = pointsfm.SfmModel.from_arrays([0, 1], np.stack([np.full((3, 3), 2.0), np.eye(3)]), [[big, big, big], [0, 0, 0]],
                                        [[0, 0, 5.0]], [0, 2], [0, 1])
    with pytest.raises(ValueError, match="non-finite pose"):
        mod.GetMaxIoUImages(5, 1.0, host=True)


def test_sanitizer_program_of_the_host_unit():
    """tools/sfm_host_asan.cpp + lt_sfm_host.cpp under AddressSanitizer and UBSan, a program of its own"""
    from helpers import run_host_asan
    run_host_asan("sfm_asan", "sfm_host_asan")


def test_percentile_picks_round_half_away_from_zero(gpu_lib):
    case = sc.percentile()
    ij, shared, angle = build(case).pair_records(host=True)
    lists = case["table"][3]
    assert [so.percentile_index(n) for n in sc.PERCENTILE_COUNTS] == [0, 1, 2, 2, 5, 11, 11]
    for k, n in enumerate(sc.PERCENTILE_COUNTS):
        assert shared[k] == n and ulps(angle[k:k + 1], lists[(2 * k, 2 * k + 1)][so.percentile_index(n)][None])[0] <= 1


def model_with_points(xyz):
    from limap_amd import pointsfm
    xyz = np.asarray(xyz, float).reshape(-1, 3)
    return pointsfm.SfmModel.from_arrays([0], np.eye(3)[None], np.zeros((1, 3)), xyz, np.arange(len(xyz) + 1),
                                         np.zeros(len(xyz), np.int32))


def test_ranges_known_answer_20_points(gpu_lib):
    """sorted x = 0 .. 19: float(20) * float(0.05) = 1.0 -> 1; float(20) * float(0.95) = 19.0 -> 19; diff 18, stretched
    by 1.25 * 18 = 22.5.  y = 2 x, z = -x (sorted -19 .. 0: elements 1 and 19 are -18 and 0)"""
    x = np.random.default_rng(0).permutation(20).astype(float)
    lo, hi = model_with_points(np.stack([x, 2 * x, -x], 1)).ComputeRanges([0.05, 0.95], 1.25)
    assert lo.dtype == np.float64 and hi.dtype == np.float64
    assert lo.tolist() == [-21.5, -43.0, -40.5] and hi.tolist() == [41.5, 83.0, 22.5]


def test_ranges_index_is_a_float32_product(gpu_lib):
    """size 100, p = 0.29: float(100) * float(0.29) = 29.0 exactly (element 29), the double product 100 * 0.29 =
    28.999999999999996 truncates to 28"""
    assert int(100 * 0.29) == 28 and so.robust_index(100, 0.29) == 29 and so.robust_index(100, 0.5) == 50
    x = np.random.default_rng(1).permutation(100).astype(float)
    lo, hi = model_with_points(np.stack([x, x, x], 1)).ComputeRanges([0.29, 0.5], 0.0)
    assert lo.tolist() == [29.0] * 3 and hi.tolist() == [50.0] * 3


@pytest.mark.parametrize("seed", range(6))
def test_ranges_equal_the_oracle(gpu_lib, seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    xyz = rng.normal(size=(n, 3)) * rng.uniform(0.1, 50)
    if seed == 0:
        xyz[:, 1] = 0.0  # -0.0 == 0.0 under ==
    p = sorted(rng.uniform(0, 0.999, 2).tolist())
    k = float(rng.uniform(0, 2))
    case = {"xyz": xyz}
    lo, hi = model_with_points(xyz).ComputeRanges(p, k)
    olo, ohi = so.ranges(case, p, k)
    assert (lo == olo).all() and (hi == ohi).all()


def test_ranges_raise_where_upstream_is_undefined(gpu_lib):
    from limap_amd import pointsfm
    with pytest.raises(ValueError, match="no points"):
        pointsfm.SfmModel().ComputeRanges([0.05, 0.95], 1.25)
    m = model_with_points(np.arange(30.0).reshape(10, 3))
    with pytest.raises(ValueError, match="outside"):
        m.ComputeRanges([0.05, 1.0], 1.25)
    with pytest.raises(ValueError, match="outside"):
        m.ComputeRanges([-0.2, 0.9], 1.25)
    bad = np.arange(30.0).reshape(10, 3)
    bad[4, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        model_with_points(bad).ComputeRanges([0.05, 0.95], 1.25)
    for args in (([0.05, 1.0], 1.25), ([-0.2, 0.9], 1.25)):
        with pytest.raises(ValueError):
            so.ranges({"xyz": np.arange(30.0).reshape(10, 3)}, *args)


# ---- the Python surface ----
def image(k):
    from limap_amd import pointsfm
    return pointsfm.SfmImage(f"im{k}.png", 640, 480, np.eye(3), np.eye(3), [-float(k), 0.0, 0.0])


def test_add_image_id_rule():
    from limap_amd import pointsfm
    m = pointsfm.SfmModel()
    m.addImage(image(0))
    m.addImage(image(1))
    assert m.reg_image_ids == [0, 1] and m.GetImageNames() == ["im0.png", "im1.png"]
    m.addImage(image(2), 7)
    with pytest.raises(ValueError, match="reg_image_ids"):
        m.addImage(image(3))  # the previous id is not count - 1
    m.addImage(image(3), 3)
    m.addImage(image(4))      # 3 == 4 - 1: accepted, id 4
    assert m.reg_image_ids == [0, 1, 7, 3, 4]
    im = image(2)
    assert im.GetT().dtype == np.float32 and im.GetR().shape == (3, 3) and im.GetK().dtype == np.float32


def test_bad_track_index_is_an_index_error(gpu_lib):
    from limap_amd import pointsfm
    m = pointsfm.SfmModel()
    for k in range(3):
        m.addImage(image(k))
    m.addPoint(0.0, 0.0, 5.0, [0, 3])
    with pytest.raises(IndexError):
        m.ComputeNumPoints()
    with pytest.raises(IndexError, match="unknown image index 3"):
        m.GetMaxIoUImages(5, 1.0, host=True)
    m2 = pointsfm.SfmModel()
    m2.addImage(image(0))
    m2.addPoint(0.0, 0.0, 5.0, [-1])
    with pytest.raises(IndexError):
        pointsfm.compute_neighbors(m2, 5, host=True)


def test_not_implemented():
    from limap_amd import pointsfm
    with pytest.raises(NotImplementedError):
        pointsfm.compute_neighbors(pointsfm.SfmModel(), 5, neighbor_type="cosine", host=True)
    with pytest.raises(NotImplementedError):
        pointsfm.SfmModel().ReadFromCOLMAP("/nowhere")


def test_from_arrays_equals_the_add_loop_and_keys_ascend(gpu_lib):
    from limap_amd import pointsfm
    case = sc.random_model(2, n=9, p=60)
    ids, R, T, xyz, off, img = sc.to_arrays(case)
    flat = pointsfm.SfmModel.from_arrays(ids, R, T, xyz, off, img)
    loop = pointsfm.SfmModel()
    for k, i in enumerate(ids):
        loop.addImage(pointsfm.SfmImage(f"image{i}", 0, 0, np.eye(3), R[k], T[k]), i)
    for p in range(len(xyz)):
        loop.addPoint(*xyz[p], img[off[p]:off[p + 1]].tolist())
    assert loop.GetImageNames() == flat.GetImageNames() and loop.ComputeNumPoints() == flat.ComputeNumPoints()
    for kind in KINDS:
        a = pointsfm.compute_neighbors(flat, 4, 1.0, kind, host=True)
        b = pointsfm.compute_neighbors(loop, 4, 1.0, kind, host=True)
        assert a == b and list(a) == sorted(ids) and list(b) == sorted(ids)
    assert all(np.array_equal(u, v) for u, v in zip(flat.ComputeRanges([0.05, 0.95], 1.25), loop.ComputeRanges([0.05, 0.95], 1.25)))
    flat.addPoint(0.0, 0.0, 5.0, [0, 1])  # a bulk model can still grow
    assert sum(flat.ComputeNumPoints()) == sum(loop.ComputeNumPoints()) + 2
    grown = pointsfm.SfmModel.from_arrays(ids, R, T, xyz, off, img)
    grown.addImage(pointsfm.SfmImage("late", 0, 0, np.eye(3), np.eye(3), [0.0, 0.0, 0.0]), 999)
    assert grown.ComputeNumPoints() == loop.ComputeNumPoints() + [0]
    assert list(pointsfm.compute_neighbors(grown, 4, 1.0, "iou", host=True)) == sorted(ids + [999])


def test_metainfos_round_trip_through_io(gpu_lib, tmp_path):
    from limap_amd import io, pointsfm
    case = sc.random_model(4, n=12, p=200)
    mod = build(case)
    cfg = {"min_triangulation_angle": 1.0, "neighbor_type": "iou", "ranges": {"range_robust": [0.05, 0.95], "k_stretch": 1.25}}
    neighbors, ranges = pointsfm.compute_metainfos(cfg, mod, n_neighbors=5, host=True)
    assert neighbors == so.neighbors(case, 5, 1.0, "iou", case["table"])
    olo, ohi = so.ranges(case, [0.05, 0.95], 1.25)
    assert (ranges[0] == olo).all() and (ranges[1] == ohi).all()
    fname = os.path.join(str(tmp_path), "metainfos.txt")
    io.save_txt_metainfos(fname, neighbors, ranges)
    nb2, (lo2, hi2) = io.read_txt_metainfos(fname)
    assert nb2 == neighbors and list(nb2) == list(neighbors)
    assert np.array_equal(lo2, ranges[0]) and np.array_equal(hi2, ranges[1])
