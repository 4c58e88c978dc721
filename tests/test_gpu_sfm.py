"""limap_amd.pointsfm on the device: lt_sfm_neighbors equals the library's host path bit for bit -- neighbour lists, pair
records (the bits of the angles included) and counts -- on the smallest shapes at which each stage can go wrong
(tests/sfm_cases.py); the counted output and the key budget through their test switches; timers; buffer reuse.  The
host path itself is pinned to tests/sfm_oracle.py by test_sfm_host.py."""
import numpy as np
import pytest

import sfm_cases as sc

pytestmark = pytest.mark.gpu

KINDS = {"overlap": 0, "iou": 1, "dice": 2}
_models = {}


def built(name, make):
    """(case, SfmModel) by name, generated once"""
    from limap_amd import pointsfm
    if name not in _models:
        case = make()
        _models[name] = (case, pointsfm.SfmModel.from_arrays(*sc.to_arrays(case)))
    return _models[name]


def assert_same(mod, num_images, kinds=("overlap", "iou", "dice"), angle=sc.GATE_DEG):
    for kind in kinds:
        dev = mod._call(KINDS[kind], num_images, angle, host=False, pairs=True)
        ref = mod._call(KINDS[kind], num_images, angle, host=True, pairs=True)
        assert np.array_equal(dev[0], ref[0]), (kind, num_images, "offsets")
        assert np.array_equal(dev[1], ref[1]), (kind, num_images, "neighbours")
        assert np.array_equal(dev[2], ref[2]) and np.array_equal(dev[3], ref[3]), (kind, "pairs")
        assert np.array_equal(dev[4].view(np.uint32), ref[4].view(np.uint32)), (kind, "angles")
    return ref


@pytest.mark.parametrize("name", ["repeated_negative", "repeated_infinite"])
def test_repeated_images_in_a_track(gpu_lib, name):
    """shared exceeds n_i + n_j: an IoU is negative or +inf, and the partner is still kept and ranked"""
    case, mod = built(name, getattr(sc, name))
    ref = assert_same(mod, 5)
    assert (np.diff(ref[0]) == [2, 2, 2, 1, 1]).all()
    assert_same(mod, 1)


@pytest.mark.parametrize("name", ["no_points", "degenerate", "single_image", "all_skipped"])
def test_empty_and_degenerate(gpu_lib, name):
    case, mod = built(name, getattr(sc, name))
    ref = assert_same(mod, 5)
    if name != "degenerate":
        assert ref[1].size == 0 and ref[2].shape[0] == 0
    else:
        assert ref[2].tolist() == [[0, 1], [0, 3], [1, 2], [1, 3], [2, 3]] and ref[0][5] == ref[0][4]  # image 4: no track


def test_percentile_rounding(gpu_lib):
    case, mod = built("percentile", sc.percentile)
    ref = assert_same(mod, 5)
    assert ref[3].tolist() == list(sc.PERCENTILE_COUNTS)
    lists = case["table"][3]
    for k, pick, rint in ((4, 5, 4), (5, 11, 10)):  # n = 7 -> element 5, n = 15 -> element 11; rint: 4 and 10
        a = lists[(2 * k, 2 * k + 1)]  # the oracle's angles: the library's own arccosine may differ in the last bit
        ulp = lambda x, y: abs(int(np.float32(x).view(np.int32)) - int(np.float32(y).view(np.int32)))
        assert ulp(ref[4][k], a[pick]) <= 1 < ulp(ref[4][k], a[rint])


def test_triangular_decode_of_a_landmark_track(gpu_lib):
    case, mod = built("landmark", sc.landmark)
    assert len(case["tracks"][0]) == 2100
    assert_same(mod, 20, kinds=("iou",))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_slot_count_at_a_workgroup_boundary(gpu_lib, delta):
    case, mod = built(f"slot{delta}", lambda: sc.slot_boundary(delta))
    assert_same(mod, 30)


@pytest.mark.parametrize("num_images", [0, 1, 3, 4, 100])
def test_ties_rank_by_ascending_index(gpu_lib, num_images):
    case, mod = built("tie_ring", sc.tie_ring)
    ref = assert_same(mod, num_images)
    n = 12
    for k in range(n):  # four partners of one score: the smallest indices first
        assert ref[1][ref[0][k]:ref[0][k + 1]].tolist() == sorted((k + d) % n for d in (-2, -1, 1, 2))[:num_images]


@pytest.mark.parametrize("partners", [64, 65, 200])
@pytest.mark.parametrize("num_images", [20, 150])
def test_select_rounds(gpu_lib, partners, num_images):
    case, mod = built(f"star{partners}", lambda: sc.star(partners))
    ref = assert_same(mod, num_images)
    assert ref[0][1] == min(partners, num_images)


def test_gate(gpu_lib):
    case, mod = built("all_gated", sc.all_gated)
    ref = assert_same(mod, 10)
    assert ref[0][1] == 0 and ref[1].size > 0  # image 0 keeps nobody, the others do
    case, mod = built("star_mixed", lambda: sc.star(100, coincident=37))
    ref = assert_same(mod, 150)
    assert ref[0][1] == 63


def test_counted_output_relaunch(gpu_lib, monkeypatch):
    from limap_amd import pointsfm
    case, mod = built("random3", lambda: sc.random_model(3))
    plain = mod._call(1, 20, sc.GATE_DEG, pairs=True)
    assert pointsfm.timers()[7] == 1
    monkeypatch.setenv("LT_TEST_SFM_PAIR_CAP", "1")
    again = mod._call(1, 20, sc.GATE_DEG, pairs=True)
    assert pointsfm.timers()[7] == 2 and plain[2].shape[0] > 1
    for a, b in zip(plain, again):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    assert_same(mod, 20, kinds=("iou",))


def test_key_budget_is_refused_by_name_and_the_context_lives(gpu_lib, monkeypatch):
    case, mod = built("random5", lambda: sc.random_model(5))
    slots = sum(len(t) * (len(t) - 1) // 2 for t in case["tracks"])
    monkeypatch.setenv("LT_TEST_SFM_KEY_BUDGET", str(16 * slots - 1))
    with pytest.raises(ValueError, match=f"E = {slots} pair instances.*budget is {16 * slots - 1}"):
        mod._call(1, 20, sc.GATE_DEG)
    monkeypatch.delenv("LT_TEST_SFM_KEY_BUDGET")
    assert_same(mod, 20)


@pytest.mark.parametrize("seed", range(20))
def test_randomised(gpu_lib, seed):
    case, mod = built(f"random{seed}", lambda: sc.random_model(seed))
    assert_same(mod, 1 + seed % 7)


def test_timers_and_a_smaller_second_call(gpu_lib):
    from limap_amd import pointsfm
    case, big = built("random17", lambda: sc.random_model(17))
    big._call(1, 20, sc.GATE_DEG)
    t = pointsfm.timers()
    assert t.shape == (8,) and np.isfinite(t).all() and (t >= 0).all() and t[3] > 0 and t[4] > 0
    case, small = built("degenerate", sc.degenerate)
    assert_same(small, 5)  # nothing of the larger model's buffers shows
    assert small.ComputeSharedPoints() == small.ComputeSharedPoints(host=True)


def test_public_calls_route_to_the_device(gpu_lib):
    from limap_amd import pointsfm
    case, mod = built("random9", lambda: sc.random_model(9))
    cfg = {"min_triangulation_angle": sc.GATE_DEG, "neighbor_type": "dice",
           "ranges": {"range_robust": [0.05, 0.95], "k_stretch": 1.25}}
    nb, rg = pointsfm.compute_metainfos(cfg, mod, n_neighbors=6)
    nb_h, rg_h = pointsfm.compute_metainfos(cfg, mod, n_neighbors=6, host=True)
    assert nb == nb_h and list(nb) == sorted(case["img_ids"])
    assert np.array_equal(rg[0], rg_h[0]) and np.array_equal(rg[1], rg_h[1])
    assert mod.GetMaxOverlapImages(4, sc.GATE_DEG) == mod.GetMaxOverlapImages(4, sc.GATE_DEG, host=True)
