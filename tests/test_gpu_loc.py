"""-m gpu: the point-line pose refinement on the device (lt_kernels_loc.hip) equals the host path (lt_fn_loc_host) bit
for bit -- pose, both costs, iterations, termination codes -- over batch sizes, block counts around the wave width,
every cost function, weight and loss; the engines equal the batch call; two runs and a permuted problem order give
identical per-problem results."""
import glob
import os

import numpy as np
import pytest

import loc_scenes as ls
from limap_amd import _capi
from limap_amd import hybrid_localization as hl
from test_loc_host import GOLDEN, load_golden, ocfg, struct_of

pytestmark = pytest.mark.gpu
KEYS = ("qvec", "tvec", "cost", "num_residuals", "iterations", "codes")


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    return _capi.Context()


def both(ctx, probs, cfg):
    csr = hl._problem_arrays(probs)
    return hl.loc_arrays(csr, struct_of(cfg), ctx=ctx), hl.loc_arrays(csr, struct_of(cfg), 8)


def same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, np.flatnonzero(np.any(np.atleast_2d(a[k].T != b[k].T), 0))[:5])


def sized(n_blocks, seed, lines_share=0.4):
    """a problem with exactly n_blocks residual blocks (one 2D segment per 3D line)"""
    nl = int(round(n_blocks * lines_share))
    return ls.make_problem(nl, n_blocks - nl, seed=seed, multi=0.0)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))))
def test_device_reproduces_the_goldens(ctx, path):
    """against the recorded bytes, not against the twin"""
    csr, s, want = load_golden(path)
    same(hl.loc_arrays(csr, s, ctx=ctx), want, os.path.basename(path))


@pytest.mark.parametrize("n_prob", [1, 4, 5, 257])
def test_batches(ctx, n_prob):
    probs = [ls.make_problem(3 + n % 5, 4 + n % 7, seed=500 + n) for n in range(n_prob)]
    d, h = both(ctx, probs, ocfg(2, 1, 3, loss_a=2.0, weight_line=0.6))
    same(d, h, n_prob)
    assert np.all(np.isin(d["codes"], (0, 1, 2))) and np.all(d["cost"][:, 1] <= d["cost"][:, 0])


@pytest.mark.parametrize("n_blocks", [1, 2, 63, 64, 65, 129, 1000])
def test_block_counts_around_the_wave_width(ctx, n_blocks):
    """1 block: two residuals for six unknowns, the damping carries the rank-deficient step"""
    probs = [sized(n_blocks, 600 + n_blocks, share) for share in ((0.0, 1.0) if n_blocks == 1 else (0.4,))]
    d, h = both(ctx, probs, ocfg(2, 0, 1, loss_a=2.0))
    same(d, h, n_blocks)
    assert np.all(d["num_residuals"] == 2 * n_blocks)
    assert np.all(d["cost"][:, 1] <= d["cost"][:, 0]) and np.all(d["iterations"] >= 1)


@pytest.mark.parametrize("cost", range(6))
def test_every_cost_function_weight_and_loss(ctx, cost):
    probs = [ls.make_problem(20, 30, seed=700 + n) for n in range(3)]
    for weight, loss in ((0, 0), (1, 1), (3, 2), (4, 3), (1, 3)):
        cfg = ocfg(cost, weight, loss, loss_a=0.05 if cost in (4, 5) else 1.5, weight_line=0.7, weight_point=1.3)
        d, h = both(ctx, probs, cfg)
        same(d, h, (cost, weight, loss))
        assert np.all(d["cost"][:, 1] <= d["cost"][:, 0])


def test_points_only_lines_only_and_three_segments(ctx):
    a = ls.make_problem(0, 40, seed=801)
    b = ls.make_problem(30, 0, seed=802)
    c = ls.make_problem(10, 5, seed=803, multi=1.0)
    assert max(len(g) for g in c["l2ds"]) == 3
    for cost in (2, 4):
        d, h = both(ctx, [a, b, c], ocfg(cost, 0, 0))
        same(d, h, cost)


@pytest.mark.parametrize("max_iter", [0, 1])
def test_iteration_caps(ctx, max_iter):
    probs = [ls.make_problem(12, 20, seed=810 + n) for n in range(4)]
    csr = hl._problem_arrays(probs)
    s = struct_of(ocfg(2, 0, 0))
    s.max_num_iterations = max_iter
    d, h = hl.loc_arrays(csr, s, ctx=ctx), hl.loc_arrays(csr, s, 4)
    same(d, h, max_iter)
    assert np.all(d["iterations"] == max_iter) and np.all(d["codes"] == 0)
    if max_iter == 0:
        assert np.array_equal(d["cost"][:, 0], d["cost"][:, 1])


def test_mixed_empty_problems_repeat_and_permutation(ctx):
    empty = dict(ls.make_problem(1, 1, seed=1), l3ds=np.zeros((0, 2, 3)), l2ds=[], p3ds=[], p2ds=[])
    probs = []
    for n in range(9):
        probs.append(ls.make_problem(4 + 9 * n, 6 + 17 * n, seed=820 + n))
        if n % 3 == 0:
            probs.append(empty)
    cfg = ocfg(3, 1, 3, loss_a=1.0)
    d, h = both(ctx, probs, cfg)
    same(d, h, "mixed")
    is_empty = np.array([len(p["p3ds"]) == 0 and len(p["l2ds"]) == 0 for p in probs])
    assert np.all(d["codes"][is_empty] == 7) and np.all(d["codes"][~is_empty] != 7)
    assert np.array_equal(d["tvec"][is_empty], np.array([p["tvec"] for p, e in zip(probs, is_empty) if e]))
    d2, _ = both(ctx, probs, cfg)
    same(d, d2, "second run")
    perm = np.random.default_rng(0).permutation(len(probs))
    d3 = hl.loc_arrays(hl._problem_arrays([probs[i] for i in perm]), struct_of(cfg), ctx=ctx)
    for k in KEYS:
        assert np.array_equal(d3[k], d[k][perm]), k


def test_engine_equals_the_batch_call(ctx):
    pr = ls.make_problem(15, 25, seed=830)
    cfg = dict(weight_line=0.8, loss_function=hl.CauchyLoss(2.0))
    batch = hl.solve_jointloc_batch("PerpendicularDist", cfg, [pr], "cosine")
    e = hl.solve_jointloc_merged("PerpendicularDist", cfg, (pr["l2ds"], pr["l3ds"]), (pr["p2ds"], pr["p3ds"]), pr["kvec"],
                                 pr["qvec"], pr["tvec"], "cosine")
    assert np.array_equal(e.GetFinalQ(), batch["qvec"][0]) and np.array_equal(e.GetFinalT(), batch["tvec"][0])
    r = e.result()
    for k in KEYS:
        assert np.array_equal(r[k], batch[k]), k
    assert e.IsSolutionUsable() and e.GetFinalCost() < e.GetInitialCost()
    assert batch["timers"]["lm_device_ms"] > 0
    host = hl.solve_jointloc_batch("PerpendicularDist", cfg, [pr], "cosine", host=True)
    same(batch, host, "engine")


# ---- pose scoring ----
@pytest.fixture(scope="module")
def score_pool():
    """500 points, 500 2D segments over 382 3D lines and 300 poses: the host test's fixture at a larger size"""
    rng = np.random.default_rng(9)
    fx = ls.score_fixture(380, 500, 294, seed=78)
    ids = np.array(fx["l3d_ids"])
    assert len(ids) >= 500
    take = rng.permutation(len(ids))[:500]
    return dict(fx, l3d_ids=ids[take], l2ds=np.array([fx["l2ds"][i] for i in take]), poses=fx["poses"][:300])


def score_both(ctx, name, fx, n_pts, n_seg, H, **kw):
    a = (name, fx["l3ds"], fx["l3d_ids"][:n_seg], fx["l2ds"][:n_seg], fx["p3ds"][:n_pts], fx["p2ds"][:n_pts], fx["kvec"],
         fx["poses"][-H:] if H else fx["poses"][:0])
    return hl.score_poses(*a, ctx=ctx, **kw), hl.score_poses(*a, host_threads=8, **kw)


@pytest.mark.parametrize("H", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("shape", [(0, 40), (40, 0), (1, 0), (0, 1), (30, 34), (33, 32), (500, 500)])
def test_scoring_equals_the_host_twin(ctx, score_pool, H, shape):
    n_pts, n_seg = shape
    assert len(score_pool["poses"]) == 300 and np.isnan(score_pool["poses"][-1]).any()
    for name in ("PerpendicularDist", "3DPlaneLineDist"):
        d, h = score_both(ctx, name, score_pool, n_pts, n_seg, H, thresholds=(4.0, 9.0), weights=(1.0, 0.5))
        assert d["residuals"].shape == (H, n_pts + n_seg)
        for k in ("residuals", "scores", "inliers"):
            assert np.array_equal(d[k], h[k]), (name, k)
        assert np.array_equal(d["residuals"] == np.finfo(float).max, h["residuals"] == np.finfo(float).max)


def test_scoring_threshold_fixture_and_table_only(ctx):
    fx = ls.score_fixture()
    for name in ("MidpointDist", "PerpendicularDist", "PerpendicularDist4", "3DLineLineDist", "3DPlaneLineDist"):
        a = (name, fx["l3ds"], fx["l3d_ids"], fx["l2ds"], fx["p3ds"], fx["p2ds"], fx["kvec"], fx["poses"])
        d = hl.score_poses(*a, ctx=ctx, thresholds=(4.0, 9.0), cheirality_min_depth=0.5, cheirality_overlap_pixels=5.0)
        h = hl.score_poses(*a, host=True, thresholds=(4.0, 9.0), cheirality_min_depth=0.5, cheirality_overlap_pixels=5.0)
        for k in ("residuals", "scores", "inliers"):
            assert np.array_equal(d[k], h[k]), (name, k)
        mx = np.finfo(float).max
        assert 0.1 < (d["residuals"] == mx).mean() < 0.9 and np.all(d["residuals"][-1] == mx)
        t = hl.score_poses(*a, ctx=ctx, cheirality_min_depth=0.5, cheirality_overlap_pixels=5.0)
        assert np.array_equal(t["residuals"], d["residuals"]) and t["scores"] is None
        assert t["timers"]["score_device_ms"] > 0
