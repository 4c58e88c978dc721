"""-m gpu: the bundle adjustment with free poses on the device (lt_kernels_ba.hip) equals the host path (lt_fn_ba_host)
bit for bit -- poses, points, line parameters, segments, both costs, iterations and code -- on the smallest shapes at
which each kernel can go wrong.  Iteration caps of 30 or less."""
import glob
import os

import numpy as np
import pytest

import ba_scenes as bs
from limap_amd import _capi
from test_ba_host import GOLDEN, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    return _capi.Context()


@pytest.fixture(scope="module")
def hybrid():
    return bs.make_scene(n_cams=4, n_points=24, n_lines=6, seed=0)  # the scene of the CPU tests


def both(ctx, s, what="", **kw):
    cfg = bs.cfg_of(**kw)
    rc_d, d = bs.run_device(ctx, s, cfg)
    rc_h, h = bs.run_host(s, cfg, 8)
    assert rc_d == 0 and rc_h == 0, (what, rc_d, rc_h)
    for k in h:
        assert np.array_equal(d[k].view(np.uint8), h[k].view(np.uint8)), (what, k, d[k], h[k])
    return d


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))))
def test_device_reproduces_the_goldens(ctx, path):
    """against the recorded bytes, not against the twin"""
    s, cfg, want = load_golden(path)
    rc, d = bs.run_device(ctx, s, bs.cfg_of(**cfg))
    assert rc == 0 and set(d) == set(want)
    for k in d:
        assert np.array_equal(d[k], want[k]), (os.path.basename(path), k)


# degenerate-but-legal sizes
def test_two_cameras_one_point(ctx):
    s = bs.make_scene(n_cams=2, n_points=1, n_lines=0, seed=11)
    d = both(ctx, s, max_num_iterations=20)
    assert d["iterations"][0] > 0


def test_three_cameras_five_points_no_lines(ctx):
    d = both(ctx, bs.make_scene(n_cams=3, n_points=5, n_lines=0, seed=12), max_num_iterations=25)
    assert d["cost"][1] < d["cost"][0]


def test_lines_only(ctx):
    d = both(ctx, bs.make_scene(n_cams=5, n_points=0, n_lines=7, seed=13), max_num_iterations=25)
    assert d["cost"][1] < d["cost"][0]


def test_hybrid_scene_of_the_cpu_tests(ctx, hybrid):
    d = both(ctx, hybrid, max_num_iterations=30)
    assert d["cost"][1] < 0.05 * d["cost"][0]


# the 16-lane group of k_ba_blocks and its loop; a track twice (and more often) in one image
def test_structure_tracks_around_the_group_width(ctx):
    s = bs.make_scene(n_cams=6, n_points=10, n_lines=8, seed=14, point_obs=[1, 15, 16, 17, 33, 2, 12], line_obs=[1, 15, 16, 17, 33, 7])
    both(ctx, s, max_num_iterations=12, min_num_images=1, num_outliers_aggregator=0)


@pytest.mark.parametrize("n_img", [6, 7, 8])
def test_tracks_seen_by_six_to_eight_images(ctx, n_img):
    s = bs.make_scene(n_cams=8, n_points=6, n_lines=3, seed=15, point_obs=[n_img] * 6, line_obs=[n_img] * 3)
    both(ctx, s, n_img, max_num_iterations=10)


def test_image_without_observations_in_the_middle_of_the_ids(ctx):
    s = bs.make_scene(n_cams=4, n_points=12, n_lines=4, seed=4, extra_images=(9,))
    row = int(np.where(s["img_ids"] == 9)[0][0])
    d = both(ctx, s, max_num_iterations=15)
    assert np.array_equal(d["qvec"][row], s["q"][row]) and np.array_equal(d["tvec"][row], s["t"][row])


# camera counts around the edges of k_ba_schur and k_ba_chol as built.  k_ba_schur has one wave per image pair and no
# strip, so its only edge is the grid (C x C blocks, the upper half idle).  k_ba_chol's one workgroup has 1024 lanes, more
# than 6 C can reach (768 at LT_BA_MAX_IMAGES), so every row has a lane of its own and no count makes 6 C pass the
# lane count; its edges are the 64-entry chunks of the back substitution (6 C = 60, 66: one chunk and two; 126, 132: two
# and three), the 16-step batches of the column loop (every count above 3 passes several), whole waves of rows
# (6 C = 252, 258; 510, 516) and the cap itself (127, 128; 129 is an argument error)
@pytest.mark.parametrize("n_cams", [10, 11, 21, 22, 42, 43, 85, 86, 127, 128])
def test_camera_counts_at_the_workgroup_edges(ctx, n_cams):
    d = both(ctx, bs.chain_scene(n_cams, seed=20 + n_cams), n_cams, max_num_iterations=4)
    assert d["cost"][1] < d["cost"][0]


def test_above_the_image_cap_is_an_argument_error(ctx):
    rc, _ = bs.run_device(ctx, bs.chain_scene(129, seed=6), bs.cfg_of())
    assert rc != 0 and "LT_BA_MAX_IMAGES" in ctx.L.lt_last_error(ctx.h).decode()


# block counts around the chunk of the cost reduction (256) and around the wave of k_ba_images (64 blocks per image)
@pytest.mark.parametrize("n_blocks", [126, 128, 130, 255, 256, 257])
def test_block_counts_around_the_chunk(ctx, n_blocks):
    n_pts = n_blocks // 2
    obs = [2] * n_pts
    if n_blocks % 2:
        obs[0] = 3
    s = bs.make_scene(n_cams=3 if n_blocks % 2 else 2, n_points=n_pts, n_lines=0, seed=30 + n_blocks, point_obs=obs)
    assert len(s["pimg"]) == n_blocks
    both(ctx, s, n_blocks, max_num_iterations=8)


def test_more_chunks_than_the_second_level_has_lanes(ctx):
    s = bs.make_scene(n_cams=6, n_points=2731, n_lines=0, seed=40)  # 16386 blocks: 65 chunks
    assert len(s["pimg"]) > 256 * 64
    both(ctx, s, max_num_iterations=3)


# the switches of the CPU tests, code 6 and code 7
@pytest.mark.parametrize("sw", [dict(constant_point=1), dict(constant_line=1), dict(min_num_images=5), dict(lw_point=0.0),
                                dict(constant_point=1, constant_line=1)])
def test_switches(ctx, hybrid, sw):
    d = both(ctx, hybrid, sw, max_num_iterations=12, **sw)
    if sw.get("constant_point"):
        assert np.array_equal(d["points"], hybrid["p3"])
    assert not np.array_equal(d["tvec"], hybrid["t"])


# constant_pose: the separated point solves of k_ba_point_lm, group width and its loop, more than one workgroup, a point
# in a camera's plane (code 6 of its track alone)
@pytest.mark.parametrize("n_points", [1, 3, 4, 5, 40])
def test_constant_pose_point_tracks(ctx, n_points):
    s = bs.make_scene(n_cams=6, n_points=n_points, n_lines=0, seed=50 + n_points, point_obs=[33, 1, 15, 16, 17][:n_points])
    d = both(ctx, s, n_points, constant_pose=1, max_num_iterations=30)
    assert np.array_equal(d["qvec"], s["q"]) and np.array_equal(d["tvec"], s["t"]) and d["cost"][1] < d["cost"][0]


def test_constant_pose_switches_and_a_failing_track(ctx, hybrid):
    s = bs.without_lines(hybrid, [])
    d = both(ctx, s, constant_pose=1, constant_point=1)
    assert d["code"][0] == 7
    d = both(ctx, s, constant_pose=1, lw_point=0.0)
    assert d["code"][0] == 7
    rc, _ = bs.run_device(ctx, hybrid, bs.cfg_of(constant_pose=1))
    assert rc != 0 and "constant_pose" in ctx.L.lt_last_error(ctx.h).decode()
    s = bs.make_scene(n_cams=3, n_points=5, n_lines=0, seed=5)
    s["q"][0] = [1.0, 0.0, 0.0, 0.0]
    s["t"][0] = [0.0, 0.0, 5.0]
    s["p3"][2] = [0.3, 0.2, -5.0]
    d = both(ctx, s, constant_pose=1, max_num_iterations=20)
    assert d["code"][0] == 6 and np.array_equal(d["points"][2], s["p3"][2]) and not np.array_equal(d["points"][1], s["p3"][1])


def test_code_6_and_code_7(ctx, hybrid):
    s = bs.make_scene(n_cams=3, n_points=5, n_lines=0, seed=5)
    s["q"][0] = [1.0, 0.0, 0.0, 0.0]
    s["t"][0] = [0.0, 0.0, 5.0]
    s["p3"][2] = [0.3, 0.2, -5.0]
    d = both(ctx, s)
    assert d["code"][0] == 6 and np.array_equal(d["points"], s["p3"])
    d = both(ctx, bs.without_lines(hybrid, []), lw_point=0.0)
    assert d["code"][0] == 7 and np.array_equal(d["tvec"], hybrid["t"])


def test_radius_end_past_the_iteration_cap_of_the_poll(ctx):
    """the solve ends (radius) between two polls: the attempts enqueued behind its end change nothing"""
    s = bs.make_scene(n_cams=3, n_points=6, n_lines=0, seed=16, noise_px=0.0, pose_sigma=0.0, struct_sigma=0.0)
    both(ctx, s, max_num_iterations=30)


def test_two_runs_identical(ctx, hybrid):
    cfg = bs.cfg_of(max_num_iterations=20)
    _, a = bs.run_device(ctx, hybrid, cfg)
    _, b = bs.run_device(ctx, hybrid, cfg)
    assert bs.same_bits(a, b)


def test_poll_interval_does_not_reach_the_result(ctx, hybrid):
    _, a = bs.run_device(ctx, hybrid, bs.cfg_of(max_num_iterations=21, poll_interval=1))
    _, b = bs.run_device(ctx, hybrid, bs.cfg_of(max_num_iterations=21))
    _, c = bs.run_device(ctx, hybrid, bs.cfg_of(max_num_iterations=21, kernel_timers=1))
    assert bs.same_bits(a, b) and bs.same_bits(a, c) and a["iterations"][0] == 21
    assert ctx.L.lt_ba_poll_default() > 1


def test_python_surface_on_the_device(ctx, hybrid):
    from limap_amd import optimize
    from test_ba_host import _py_scene
    imagecols, pts, lines = _py_scene(hybrid)
    cfg_ba = optimize.HybridBAConfig(dict(min_num_images=4))
    cfg_ba.constant_intrinsics = True
    dev = optimize.solve_hybrid_bundle_adjustment(cfg_ba, imagecols, pts, lines, max_num_iterations=10).result()
    host = optimize.solve_hybrid_bundle_adjustment(cfg_ba, imagecols, pts, lines, max_num_iterations=10, host_threads=4).result()
    for k in ("qvec", "tvec", "points", "params", "segments", "cost_ba"):
        assert np.array_equal(dev[k], host[k]), k
    assert dev["timers"]["attempts_enqueued"] >= 10
    cfg_ba.set_constant_camera()  # constant poses: the lines through the refinement, the points through their own solves
    dev = optimize.solve_hybrid_bundle_adjustment(cfg_ba, imagecols, pts, lines, max_num_iterations=10).result()
    host = optimize.solve_hybrid_bundle_adjustment(cfg_ba, imagecols, pts, lines, max_num_iterations=10, host_threads=4).result()
    for k in ("points", "params", "segments", "cost", "cost_ba"):
        assert np.array_equal(dev[k], host[k]), k
