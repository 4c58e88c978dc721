"""limap_amd.undistortion without a GPU: the library's host path (lt_fn_undist_warp_host, lt_fn_undist_points_host,
lt_fn_undist_scale) equals tests/undist_oracle.py -- a NumPy restatement of DESIGN.md section 22 -- exactly, on every
case family of tests/undist_cases.py: image bytes, camera parameters and sizes, points, statuses, iteration counts.
Then checks that do not rest on the restatement (round trip, an all-255 source, scipy's interpolation, a known
answer), limap's own branches, and the Python surface."""
import os

import numpy as np
import pytest

import undist_cases as uc
import undist_oracle as uo

# the largest round-trip residual |ImgFromCam(CamFromImg(p)) - p| of the restatement over the distorted cameras of
# undist_cases.cameras() on grid_points(), measured on the CPU: 9.00003e-10 px, written here rounded up in its third digit (the
# Newton loop stops once an update is shorter than 1e-5 in normalised units; the update after it would be of the order of
# its square times the focal length).
# The host path is held to 10 times that.
ORACLE_ROUND_TRIP_PX = 9.01e-10


def cam_of(c, cam_id=3):
    from limap_amd import undistortion as und
    return und.Camera(c.model, c.params, cam_id=cam_id, hw=(c.h, c.w))


def same_camera(got, want):
    return got.model == want.model and got.params.tolist() == list(want.params) and (got.h(), got.w()) == (want.h, want.w)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. host path == the restatement, exactly ----
@pytest.mark.parametrize("name", sorted(uc.cameras()))
def test_host_path_equals_the_oracle(gpu_lib, name):
    from limap_amd import undistortion as und
    c = uc.cameras()[name]
    want_cam, _ = uo.undistort_camera(c)
    got_cam = und.undistort_camera(cam_of(c), host=True)
    assert same_camera(got_cam, want_cam), (got_cam, want_cam)
    assert got_cam.camera_id == 3
    for ch in (0, 1, 3, 4):
        img = uc.image(c.h, c.w, ch, seed=ch)
        got = und._warp_batch([(cam_of(c), got_cam, img)], host=True)[0]
        want = uo.warp(c, want_cam, img)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), ch
    pts = np.concatenate([uc.grid_points(c), uc.random_points(c, 50, seed=len(name))])
    want, wstatus, witers = uo.undistort_points(c, want_cam, pts)
    got, status, iters = und.undistort_points(pts, cam_of(c), got_cam, host=True, return_status=True)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(status, wstatus) and np.array_equal(iters, witers)
    assert not status.any()


@pytest.mark.parametrize("options", [dict(blank_pixels=1.0), dict(blank_pixels=0.3), dict(max_scale=0.97),
                                     dict(min_scale=1.05, max_scale=3.0)])
def test_undistort_camera_options(gpu_lib, options):
    from limap_amd import undistortion as und
    for name in ("radial_barrel", "opencv_pincushion"):
        c = uc.cameras()[name]
        want, _ = uo.undistort_camera(c, **options)
        assert same_camera(und.undistort_camera(cam_of(c), host=True, **options), want), name


def test_newton_exits(gpu_lib):
    """the principal point (the step falls back to DBL_EPSILON), the 100 iterations, the singular Jacobian"""
    from limap_amd import undistortion as und
    cam, p100 = uc.hundred_iterations()
    _, psing = uc.singular_jacobian()
    target = uo.make(1, (64.0, 64.0, 32.0, 16.0), cam.h, cam.w)
    pts = np.concatenate([[[32.0, 16.0]], p100, psing])
    want, wstatus, witers = uo.undistort_points(cam, target, pts)
    assert witers.tolist() == [1, 100, 1] and wstatus.tolist() == [0, 0, 1]
    got, status, iters = und.undistort_points(pts, cam_of(cam), cam_of(target), host=True, return_status=True)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(status, wstatus) and np.array_equal(iters, witers)
    assert got[0].tolist() == [32.0, 16.0] and np.isfinite(got[1]).all()
    assert (bits(got[2]) == uo.NAN_BITS).all()
    with pytest.raises(ValueError, match="point 2 has no undistorted position"):
        und.undistort_points(pts, cam_of(cam), cam_of(target), host=True)


# ---- 2. checks that do not rest on the restatement ----
@pytest.mark.parametrize("name", uc.DISTORTED)
def test_round_trip(gpu_lib, name):
    """ImgFromCam(CamFromImg(p)) == p within 10 times the restatement's own residual: the undistorted camera here is the
    identity pinhole (f = 1, c = 0), so undistort_points returns the normalised point, and warping it back is the
    closed-form forward distortion, evaluated in NumPy"""
    from limap_amd import undistortion as und
    c = uc.cameras()[name]
    ident = uo.make(1, (1.0, 1.0, 0.0, 0.0), c.h, c.w)
    pts = uc.grid_points(c)
    uv = und.undistort_points(pts, cam_of(c), cam_of(ident), host=True)
    bx, by = uo.img_from_cam(c, uv[:, 0], uv[:, 1])
    res = float(np.hypot(bx - pts[:, 0], by - pts[:, 1]).max())
    u, v, _, _ = uo.cam_from_img(c, pts[:, 0], pts[:, 1])
    ox, oy = uo.img_from_cam(c, u, v)
    oracle_res = float(np.hypot(ox - pts[:, 0], oy - pts[:, 1]).max())
    print(f"{name}: round-trip residual {res:.3e} px, the restatement's {oracle_res:.3e} px")
    assert oracle_res <= ORACLE_ROUND_TRIP_PX
    assert res <= 10 * ORACLE_ROUND_TRIP_PX


@pytest.mark.parametrize("name", uc.DISTORTED)
def test_all_white_source_is_black_only_at_the_border(gpu_lib, name):
    from limap_amd import undistortion as und
    c = uc.cameras()[name]
    _, raw = uo.undistort_camera(c)
    assert all(0.2 < s < 2.0 for s in raw)  # the precondition: no clamp engages
    target = und.undistort_camera(cam_of(c), host=True)
    out = und._warp_batch([(cam_of(c), target, np.full((c.h, c.w), 255, np.uint8))], host=True)[0]
    zeros = np.argwhere(out == 0)
    h, w = out.shape
    assert all(y < 1 or y >= h - 1 or x < 1 or x >= w - 1 for y, x in zeros.tolist())
    assert (out[1:-1, 1:-1] == 255).all()


@pytest.mark.parametrize("name", uc.DISTORTED)
def test_interior_equals_scipy_bilinear(gpu_lib, name):
    ndi = pytest.importorskip("scipy.ndimage")
    from limap_amd import undistortion as und
    c = uc.cameras()[name]
    target, _ = uo.undistort_camera(c)
    img = uc.image(c.h, c.w, 3, seed=9)
    out = und._warp_batch([(cam_of(c), cam_of(target), img)], host=True)[0]
    sx, sy = uo.source_coords(c, target)
    for ch in range(3):
        ref = ndi.map_coordinates(img[:, :, ch].astype(np.float64), [sy, sx], order=1, mode="constant", cval=0.0)
        diff = np.abs(out[:, :, ch].astype(np.float64) - ref)[2:-2, 2:-2]
        assert diff.size > 0 and diff.max() <= 1.0, (ch, diff.max())


def test_exact_coordinates_known_answer(gpu_lib):
    """SIMPLE_RADIAL with k = 0 forced through the warp: the source, its last row and last column 0"""
    from limap_amd import undistortion as und
    src, dst, img, want = uc.quirk()
    assert cam_of(src).IsUndistorted()
    out = und._warp_batch([(cam_of(src), cam_of(dst), img)], host=True)[0]
    assert np.array_equal(out, want)


def test_overflowing_coefficients_are_black(gpu_lib):
    from limap_amd import undistortion as und
    src, dst, img = uc.overflow()
    sx, sy = uo.source_coords(src, dst)
    assert np.isinf(sx).any() and np.isnan(sy).any() and np.isfinite(sx).any()
    out = und._warp_batch([(cam_of(src), cam_of(dst), img)], host=True)[0]
    assert out.shape == img.shape and not out.any()
    with pytest.raises(ValueError, match="camera 3 .*border point"):
        und.undistort_camera(cam_of(src), host=True)


# ---- 3. limap's branches ----
def test_undistorted_cameras_come_back_as_upstream_says(gpu_lib):
    from limap_amd import undistortion as und
    img = uc.image(uc.H, uc.W, 3)
    flat = {0: (50.0, 20.3, 14.6), 1: (48.0, 52.0, 19.7, 15.2), 2: (50.0, 20.3, 14.6, 0.0),
            3: (50.0, 20.3, 14.6, 0.0, 1e-17), 4: (48.0, 52.0, 19.7, 15.2, 0.0, 0.0, 0.0, 0.0)}
    for model, params in flat.items():
        cam = und.Camera(model, params, cam_id=model + 10, hw=(uc.H, uc.W))
        assert cam.IsUndistorted()
        got, out = und.undistort_image_camera(cam, img, host=True)
        assert np.array_equal(out, img) and out is not img
        if model in (0, 1):
            assert got is cam
        else:
            assert got.model == (0 if model == 2 else 1) and got.camera_id == model + 10
            assert np.array_equal(got.K(), cam.K()) and (got.h(), got.w()) == (uc.H, uc.W)
    assert not und.Camera(2, (50.0, 20.3, 14.6, 1e-15), hw=(uc.H, uc.W)).IsUndistorted()


def test_transposed_image_rescales_before_and_after(gpu_lib):
    from limap_amd import undistortion as und
    c = uc.cameras()["opencv_tangential"]
    img = uc.image(c.w, c.h, 3, seed=2)  # the camera's size transposed
    got_cam, got = und.undistort_image_camera(cam_of(c), img, host=True)
    # by hand: Rescale to the image, undistort, Rescale to (undistorted height, undistorted width)
    sx, sy = c.h / c.w, c.w / c.h
    fx, fy, cx, cy, k = uo.intrinsics(c)
    turned = uo.make(4, (fx * sx, fy * sy, cx * sx, cy * sy) + tuple(k), c.w, c.h)
    target, _ = uo.undistort_camera(turned)
    assert np.array_equal(got, uo.warp(turned, target, img))
    tx, ty = target.h / target.w, target.w / target.h
    tfx, tfy, tcx, tcy, _ = uo.intrinsics(target)
    assert got_cam.params.tolist() == [tfx * tx, tfy * ty, tcx * tx, tcy * ty]
    assert (got_cam.w(), got_cam.h()) == (target.h, target.w)
    with pytest.raises(RuntimeError, match="Error! The height and width of the given camera do not match the input image."):
        und.undistort_image_camera(cam_of(c), uc.image(c.h, c.w + 1, 3), host=True)


@pytest.mark.parametrize("model", [5, 7, 8, 9, 10])
def test_models_left_out(model):
    from limap_amd import undistortion as und
    with pytest.raises(NotImplementedError, match=und.MODEL_NAMES[model]):
        und.Camera(model, [1.0] * 12)
    with pytest.raises(NotImplementedError, match=und.MODEL_NAMES[model]):
        und.Camera(und.MODEL_NAMES[model], [1.0] * 12)


def test_camera_class():
    from limap_amd import undistortion as und
    cam = und.Camera("RADIAL", [50.0, 20.0, 15.0, 0.1, 0.01], cam_id=4, hw=(30, 40))
    assert cam.model == 3 and cam.camera_id == 4 and (cam.h(), cam.w()) == (30, 40)
    assert cam.kvec().tolist() == [50.0, 50.0, 20.0, 15.0]
    assert cam.K().tolist() == [[50.0, 0.0, 20.0], [0.0, 50.0, 15.0], [0.0, 0.0, 1.0]]
    cam.Rescale(80, 30)  # sx = 2, sy = 1: one focal length takes their mean
    assert cam.params.tolist() == [75.0, 40.0, 15.0, 0.1, 0.01] and (cam.h(), cam.w()) == (30, 80)
    two = und.Camera("OPENCV", [48.0, 52.0, 20.0, 15.0, 0.1, 0, 0, 0], hw=(30, 40)).Rescale(20, 60)
    assert two.params[:4].tolist() == [24.0, 104.0, 10.0, 30.0]
    assert und.Camera("PINHOLE", np.array([[48.0, 0, 20.0], [0, 52.0, 15.0], [0, 0, 1]])).params.tolist() == [48.0, 52.0, 20.0, 15.0]
    assert und.Camera(0, [50.0, 1, 2], hw=(3, 4)) == und.Camera("SIMPLE_PINHOLE", [50.0, 1, 2], cam_id=9, hw=(3, 4))
    assert und.Camera(0, [50.0, 1, 2], hw=(3, 4)) != und.Camera(0, [50.0, 1, 2], hw=(4, 3))


# ---- 4. the Python surface on the host path ----
def test_paths_through_pil(gpu_lib, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from limap_amd import undistortion as und
    c = uc.cameras()["radial_barrel"]
    img = uc.image(c.h, c.w, 3, seed=4)
    src = tmp_path / "in.png"
    Image.fromarray(img).save(src)
    want_cam, want = und.undistort_image_camera(cam_of(c), img, host=True)
    got_cam = und.undistort_image_camera(cam_of(c), str(src), str(tmp_path / "out.png"), host=True)
    assert got_cam == want_cam and np.array_equal(np.asarray(Image.open(tmp_path / "out.png")), want)
    cams, imgs = und.undistort_images({7: cam_of(c)}, {7: src}, output_dir=str(tmp_path / "und"), host=True)
    assert cams[7] == want_cam and np.array_equal(imgs[7], want)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "und" / "image00000007.png")), want)


def test_dicts_and_one_border_scan_per_distinct_camera(gpu_lib):
    from limap_amd import undistortion as und
    cs = uc.cameras()
    a, b = cs["radial_barrel"], cs["opencv_tangential"]
    cameras = {5: cam_of(a, 1), 2: cam_of(a, 2), 9: cam_of(b, 3), 4: cam_of(cs["pinhole"], 4)}
    images = {5: uc.image(uc.H, uc.W, 3, 1), 2: uc.image(uc.H, uc.W, 0, 2), 9: uc.image(uc.H, uc.W, 4, 3),
              4: uc.image(uc.H, uc.W, 3, 4)}
    before = dict(und.stats)
    cams, imgs = und.undistort_images(cameras, images, host=True)
    assert und.stats["border_scans"] - before["border_scans"] == 2  # cameras 1 and 2 compare equal
    assert und.stats["warp_calls"] - before["warp_calls"] == 1
    assert sorted(cams) == sorted(imgs) == [2, 4, 5, 9]
    assert cams[4] is cameras[4] and np.array_equal(imgs[4], images[4])
    for i, c in ((5, a), (2, a), (9, b)):
        target, _ = uo.undistort_camera(c)
        assert same_camera(cams[i], target) and cams[i].camera_id == cameras[i].camera_id
        assert np.array_equal(imgs[i], uo.warp(c, target, images[i]))
    pts = {5: uc.random_points(a, 7, 1), 9: uc.random_points(b, 0, 2), 2: uc.random_points(a, 3, 3)}
    got = und.undistort_points_scene(pts, cameras, cams, host=True)
    for i, c in ((5, a), (2, a), (9, b)):
        want = uo.undistort_points(c, uo.undistort_camera(c)[0], pts[i])[0]
        assert got[i].shape == (len(pts[i]), 2) and np.array_equal(bits(got[i]), bits(want))


def test_chunking_gives_the_same_bytes(gpu_lib):
    from limap_amd import undistortion as und
    c = uc.cameras()["full_opencv"]
    cameras = {i: cam_of(c) for i in range(3)}
    images = {i: uc.image(c.h, c.w, 3, seed=i) for i in range(3)}
    _, whole = und.undistort_images(cameras, images, host=True)
    before = und.stats["warp_calls"]
    _, parts = und.undistort_images(cameras, images, host=True, max_chunk_bytes=1)
    assert und.stats["warp_calls"] - before == 3
    assert all(np.array_equal(whole[i], parts[i]) for i in range(3))


def test_errors_before_any_work(gpu_lib):
    from limap_amd import undistortion as und
    c = uc.cameras()["radial_barrel"]
    img = uc.image(c.h, c.w, 3)
    with pytest.raises(ValueError, match="non-finite"):
        und.Camera(3, [50.0, 20.0, np.nan, 0.1, 0.0], hw=(30, 40))
    with pytest.raises(ValueError, match="focal length is 0"):
        und.Camera(4, [48.0, 0.0, 20.0, 15.0, 0, 0, 0, 0], hw=(30, 40))
    with pytest.raises(ValueError, match="size below 1"):
        und.Camera(3, [50.0, 20.0, 15.0, 0.1, 0.0], hw=(0, 40))
    with pytest.raises(ValueError, match="size below 1"):
        und.undistort_camera(und.Camera(3, [50.0, 20.0, 15.0, 0.1, 0.0]), host=True)
    with pytest.raises(ValueError, match="takes 5 parameters"):
        und.Camera(3, [50.0, 20.0, 15.0, 0.1])
    with pytest.raises(ValueError, match="uint8"):
        und.undistort_image_camera(cam_of(c), img.astype(np.float32), host=True)
    with pytest.raises(ValueError, match="channel count"):
        und.undistort_image_camera(cam_of(c), np.zeros((c.h, c.w, 2), np.uint8), host=True)
    with pytest.raises(RuntimeError, match="do not match the input image"):
        und.undistort_image_camera(cam_of(c), np.zeros((c.h + 1, c.w, 3), np.uint8), host=True)
    for bad in (dict(blank_pixels=-0.1), dict(blank_pixels=1.1), dict(min_scale=0.0), dict(min_scale=2.0, max_scale=1.0)):
        with pytest.raises(ValueError, match="Check failed"):
            und.undistort_camera(cam_of(c), host=True, **bad)
    # the library refuses the same on its own (a caller of the C ABI has no Python in front of it)
    L = gpu_lib
    from limap_amd import _capi
    tab = (_capi.LtUndistCamera * 1)()
    tab[0].model, tab[0].n_params = 2, 4
    tab[0].params[0:4] = [0.0, 1.0, 1.0, 0.0]
    assert L.lt_fn_undist_points_host(1, tab, 0, None, None, None, None, None, None, 1) != 0
    assert b"focal length is 0" in L.lt_fn_undist_host_error()


def test_sanitizer_program_of_the_host_unit():
    """tools/undist_host_asan.cpp + lt_undist_host.cpp under AddressSanitizer and UBSan, a program of its own"""
    from helpers import run_host_asan
    run_host_asan("undist_asan", "undist_host_asan")
