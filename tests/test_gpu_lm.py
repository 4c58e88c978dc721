"""-m gpu: the minimisers' shared loop (lt_lm.h) on the device.  Every named case of tests/lm_cases.py through its kernel
(k_refine_lm, k_refine_lm_terms, k_loc_lm, k_ba_point_lm) equals the host twin bit for bit and ends with its declared code -- the codes 1 to
4 asked of the device by name; tracks that leave the loop with different codes at different iterations side by side in
one wave (four 16-lane groups), in a wave that is not full and one that spills over, in three orders, each equal to its
result alone; pose problems with seven different ends in one call of 5 and of 257 problems; four ends in one workgroup
of k_refine_lm_feat; the free-pose bundle adjustment's decisions against the twin."""
import numpy as np
import pytest

import ba_scenes as bs
import lm_cases as lc
from limap_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    return _capi.Context()


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.name)
def test_every_case_on_the_device(gpu_lib, ctx, case):
    dev, host = lc.run_device(case, ctx), lc.run_host(case)
    assert len(dev) == len(host) == 1
    assert lc.same(dev[0], host[0]), (case.name, {k: (dev[0][k], host[0][k]) for k in lc.FIELDS})
    assert dev[0]["code"] == case.code


def orders(n):
    """the given order, reversed, rotated by one"""
    idx = list(range(n))
    return [idx, idx[::-1], idx[1:] + idx[:1]]


# exits of k_refine_lm under one configuration (200 iterations): constant (5), the cap after 200 iterations (0), zero
# gradient at iteration 0 (2), a bad pivot after 7 iterations on 26 supports (3), a bad model after 14 rejections (4),
# the radius after 62 iterations (1)
LINE_MIX = [lambda o: lc.line_track(3, id_offset=o), lambda o: lc.line_track(8, 1e44, id_offset=o),
            lambda o: lc.line_track(0, 1e-100, id_offset=o), lambda o: lc.line_track(6, 1e44, id_offset=o),
            lambda o: lc.line_track(0, 1e-40, id_offset=o), lambda o: lc.line_track(2, id_offset=o)]
LINE_MIX_CODES = [5, 0, 2, 3, 4, 1]


@pytest.fixture(scope="module")
def lines_alone():
    scenes = [b(1000 * (j + 1)) for j, b in enumerate(LINE_MIX)]
    alone = [lc._refine_run(s, lc.IT(200), host_threads=1)[0] for s in scenes]
    assert [a["code"] for a in alone] == LINE_MIX_CODES
    assert alone[1]["iterations"] == 200 and sorted(a["iterations"] for a in alone) == [0, 0, 7, 14, 62, 200]
    return scenes, alone


@pytest.mark.parametrize("n", [3, 4, 5, 6])
def test_mixed_exits_in_one_wave_of_k_refine_lm(gpu_lib, ctx, lines_alone, n):
    scenes, alone = lines_alone
    for order in orders(n):
        dev = lc._refine_run(lc.concat_lines([scenes[j] for j in order]), lc.IT(200), ctx=ctx)
        for d, j in zip(dev, order):
            assert lc.same(d, alone[j]), (n, order, j, {k: (d[k], alone[j][k]) for k in lc.FIELDS})


# ends of k_refine_lm_terms under one configuration (the geometric and the heatmap term, min_num_images 2): a start that
# cannot be evaluated (6), a bad pivot after steps into infinite texels on 33 supports (3, 7 iterations), a constant track
# of one support (5), the radius after 82 iterations with such steps rejected on the way (1), an ordinary track (1)
TERMS_CFG = dict(lc.EDGE, min_num_images=2)


def terms_mix():
    """the five one-track scenes, every one with image ids and heatmaps of its own"""
    import refine_terms_scenes as ts

    def own(s, off):
        s = dict(s, img_ids=np.ascontiguousarray(s["img_ids"] + off, np.int32), img=np.ascontiguousarray(s["img"] + off, np.int32))
        s["heatmaps"] = {int(i) + off: a for i, a in s["heatmaps"].items()}
        return s
    terms = dict(use_heatmap=1)
    return [own(b, 10000 * (k + 1)) for k, b in enumerate((lc.terms_track(7, terms=terms), lc.terms_band_track(6),
                                                          lc.terms_track(0, terms=terms), lc.terms_band_track(5),
                                                          lc.terms_track(6, terms=terms)))]


@pytest.mark.parametrize("n", [3, 4, 5])
def test_mixed_exits_in_one_wave_of_k_refine_lm_terms(gpu_lib, ctx, n):
    import refine_terms_scenes as ts
    scenes = terms_mix()
    alone = [lc._terms_run(s, TERMS_CFG)[0] for s in scenes]
    assert [a["code"] for a in alone] == [6, 3, 5, 1, 1]
    assert [a["iterations"] for a in alone[:4]] == [0, 7, 0, 82] and alone[4]["iterations"] not in (0, 7, 82)
    for order in orders(n):
        mixed = scenes[order[0]]
        for j in order[1:]:
            mixed = ts.merge(mixed, scenes[j])
        mixed["_terms"] = dict(use_heatmap=1)
        dev = lc._terms_run(mixed, TERMS_CFG, ctx=ctx)
        for d, j in zip(dev, order):
            assert lc.same(d, alone[j]), (n, order, j, {k: (d[k], alone[j][k]) for k in lc.FIELDS})


# exits of k_ba_point_lm under one configuration: zero gradient after 4 iterations (2), the radius after 24 (1), a bad model
# at iteration 0 (4), a bad pivot at iteration 0 (3), a start that is not finite (6), the radius on 33 blocks
POINT_MIX = [lambda o: lc.point_track(0, id_offset=o), lambda o: lc.point_track(5, id_offset=o),
             lambda o: lc.point_track(0, 1e-100, id_offset=o), lambda o: lc.point_track(0, 1e44, id_offset=o),
             lambda o: lc.point_track(1, 1e160, id_offset=o), lambda o: lc.point_track(4, id_offset=o)]
POINT_MIX_CODES = [2, 1, 4, 3, 6, 1]


@pytest.fixture(scope="module")
def points_alone():
    scenes = [b(1000 * (j + 1)) for j, b in enumerate(POINT_MIX)]
    alone = []
    for s in scenes:
        rc, o = bs.run_host(s, lc.point_cfg(lc.IT(200)), 1)
        assert rc == 0
        alone.append(lc._point_out(o)[0])
    assert [a["code"] for a in alone] == POINT_MIX_CODES
    return scenes, alone


@pytest.mark.parametrize("n", [3, 4, 5, 6])
def test_mixed_exits_in_one_wave_of_k_ba_point_lm(gpu_lib, ctx, points_alone, n):
    """the separated solve reports the points per track and a summary: the costs summed in ascending order, the largest
    iteration count and the largest code"""
    scenes, alone = points_alone
    for order in orders(n):
        s = lc.concat_points([scenes[j] for j in order])
        rc, dev = bs.run_device(ctx, s, lc.point_cfg(lc.IT(200)))
        assert rc == 0
        rc, host = bs.run_host(s, lc.point_cfg(lc.IT(200)), 1)
        assert rc == 0 and bs.same_bits(dev, host), (n, order)
        cost0 = cost1 = 0.0
        for row, j in enumerate(order):
            assert np.array_equal(dev["points"][row], alone[j]["p"], equal_nan=True), (n, order, j)
            cost0, cost1 = cost0 + alone[j]["cost0"], cost1 + alone[j]["cost1"]
        assert np.array_equal(dev["cost"], [cost0, cost1], equal_nan=True)
        assert dev["iterations"][0] == max(alone[j]["iterations"] for j in order)
        assert dev["code"][0] == max(alone[j]["code"] for j in order)


# ends of k_loc_lm under one configuration (20 iterations): the cap (0), the radius after 15 rejections (1), zero gradient
# (2), a bad pivot (3), a bad model (4), a start that is not finite (6), no residuals (7)
POSE_MIX = [lambda: lc.pose_problem(), lambda: lc.pose_problem(scale=1e-60), lambda: lc.points_only(1e-170),
            lambda: lc.pose_problem(scale=1e151), lambda: lc.pose_problem(scale=1e-100), lambda: lc.pose_problem(scale=1e153),
            lambda: lc.empty_problem()]
POSE_MIX_CODES = [0, 1, 2, 3, 4, 6, 7]


@pytest.mark.parametrize("n", [5, 257])
def test_mixed_ends_in_one_call_of_k_loc_lm(gpu_lib, ctx, n):
    problems = [b() for b in POSE_MIX]
    alone = [lc._loc_run([pr], lc.IT(20), host_threads=1)[0] for pr in problems]
    assert [a["code"] for a in alone] == POSE_MIX_CODES
    for start, stride in ((0, 1), (6, -1)):
        order = [(start + stride * i) % 7 for i in range(n)]
        dev = lc._loc_run([problems[j] for j in order], lc.IT(20), ctx=ctx)
        assert {d["code"] for d in dev} >= ({0, 1, 2, 3, 4} if n == 5 and stride == 1 else {2, 3, 4, 6, 7})
        for d, j in zip(dev, order):
            assert lc.same(d, alone[j]), (n, order[:8], j, {k: (d[k], alone[j][k]) for k in lc.FIELDS})


def test_four_ends_in_one_workgroup_of_k_refine_lm_feat(gpu_lib, ctx):
    """k_refine_lm_feat runs four tracks per workgroup, one wave each: a start that fails (6), a constant track (5), an
    ordinary solve and a track whose every sample is dropped end side by side; each equals the twin's result alone"""
    import refine_feature_scenes as fs
    maps, scenes, codes = lc.feat_mix()
    rf = fs.refine_cfg(max_num_iterations=lc.FEAT_ITERATIONS)
    alone = [fs.run(s, rf, "map", maps, host_threads=1) for s in scenes]
    assert [int(a["codes"][0]) for a in alone[:2]] == codes[:2] and all(a["iterations"][0] > 0 for a in alone[2:])
    assert alone[2]["iterations"][0] != alone[3]["iterations"][0]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 2, 3, 0]):
        mixed = fs.merge(*[scenes[j] for j in order])
        dev = fs.run(mixed, rf, "map", maps, ctx=ctx)
        fs.same_bits(dev, fs.run(mixed, rf, "map", maps, host_threads=2), order)
        for row, j in enumerate(order):
            for k in fs.RESULT_KEYS:
                assert np.ascontiguousarray(dev[k][row]).tobytes() == np.ascontiguousarray(alone[j][k][0]).tobytes(), (order, j, k)


@pytest.mark.parametrize("name", sorted(lc.BA_SCENES))
def test_free_pose_ba_on_the_device(gpu_lib, ctx, name):
    """the scenes of test_lm_host.py whose attempts fail their factorisation before the radius ends the solve, and
    whose gradient is zero: the kernels' k_ba_decide against the twin, every output bit for bit"""
    scale, code = lc.BA_SCENES[name]
    s, cfg = lc.ba_scene(scale), bs.cfg_of(**lc.BA_CFG)
    rc, dev = bs.run_device(ctx, s, cfg)
    assert rc == 0
    rc, host = bs.run_host(s, cfg, 2)
    assert rc == 0 and bs.same_bits(dev, host), {k: (dev[k], host[k]) for k in ("cost", "iterations", "code")}
    assert dev["code"][0] == code
