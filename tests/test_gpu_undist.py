"""limap_amd.undistortion on the device: k_undist_warp and k_undist_points equal the library's host path bit for bit --
image bytes, points (NaN bits included), statuses, iteration counts and the cameras of the border scan -- on the
smallest shapes at which the kernels can go wrong (tests/undist_cases.py): widths around a lane's run, a wave and a
workgroup, every channel count, padded rows, targets larger and smaller than their source, a mixed batch, exact and
overflowing coordinates, every exit of the Newton loop, torch tensors in place, chunks.  The host path itself is
pinned to tests/undist_oracle.py by test_undist_host.py.  Where a case could misbehave the host path runs first, in the
same test; the device runs only if it returned."""
import numpy as np
import pytest

import undist_cases as uc
import undist_oracle as uo

pytestmark = pytest.mark.gpu

WIDTHS, HEIGHTS = (1, 3, 63, 64, 65, 130, 257), (1, 2, 5)


def cam_of(c, cam_id=3):
    from limap_amd import undistortion as und
    return und.Camera(c.model, c.params, cam_id=cam_id, hw=(c.h, c.w))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def both(items, **kw):
    """host first, then the device: -> the host's images, after asserting the device's are the same bytes"""
    from limap_amd import undistortion as und
    ref = und._warp_batch(items, host=True, **kw)
    dev = und._warp_batch(items, host=False, **kw)
    assert len(ref) == len(dev)
    for k, (r, d) in enumerate(zip(ref, dev)):
        assert r.shape == d.shape and d.dtype == np.uint8 and np.array_equal(r, d), k
    return ref


def sized_items(ch, model=2, same_size=True):
    """every width x height: with same_size the target is the pinhole camera of the source's size (the target widths
    are then exactly WIDTHS), without it the camera UndistortCamera gives (a few pixels smaller or larger)"""
    from limap_amd import undistortion as und
    items = []
    for h in HEIGHTS:
        for w in WIDTHS:
            c = uc.sized_camera(h, w, model=model, sign=-1.0 if (h + w) % 2 else 1.0)
            target = und.Camera("PINHOLE", cam_of(c).kvec(), hw=(h, w)) if same_size else \
                und.undistort_camera(cam_of(c), host=True)
            items.append((cam_of(c), target, uc.image(h, w, ch, seed=ch)))
    return items


@pytest.mark.parametrize("ch", [0, 1, 3, 4])
def test_sizes_and_channels(gpu_lib, ch):
    items = sized_items(ch, model=(2, 3, 4, 4, 3)[ch])
    assert [t.w() for _, t, _ in items[:7]] == list(WIDTHS)
    for it in items:
        both([it])
    ref = both(items + sized_items(ch, model=(2, 3, 4, 4, 3)[ch], same_size=False))  # and all of them in one launch
    assert sum(bool(r.any()) for r in ref) >= 20  # (an image one pixel wide or high has no pixel with four neighbours)


def test_targets_larger_and_smaller_than_the_source(gpu_lib):
    """the scale at the max_scale clamp (the undistorted border lies far outside: target larger) and at the min_scale
    clamp (target smaller); the sign of the radial term that gives each follows from the scale rule"""
    from limap_amd import undistortion as und
    grow = uo.make(2, (40.0, 33.3, 2.4, -0.15), 5, 65)
    shrink = uo.make(3, (40.0, 32.6, 2.7, 0.4, 0.1), 5, 65)
    items = []
    for c, opts, cmp in ((grow, dict(max_scale=1.1), 1), (shrink, dict(min_scale=0.9), -1)):
        want, raw = uo.undistort_camera(c, **opts)
        assert (raw[0] > 1.1) if cmp > 0 else (raw[0] < 0.9)  # the clamp engages along x
        host_cam = und.undistort_camera(cam_of(c), host=True, **opts)
        dev_cam = und.undistort_camera(cam_of(c), host=False, **opts)
        assert host_cam == dev_cam and host_cam.params.tolist() == list(want.params)
        assert (host_cam.w() > c.w) if cmp > 0 else (host_cam.w() < c.w)
        items.append((cam_of(c), host_cam, uc.image(c.h, c.w, 3, seed=cmp + 2)))
    ref = both(items)
    assert all(r.any() for r in ref)


def test_mixed_batch_in_one_call(gpu_lib):
    """1x1, 70x50 and 257x5 images, three cameras of three models, two images sharing one camera, 1, 3 and 4 channels:
    pixel counts on both sides of a workgroup's share (1024 target pixels)"""
    from limap_amd import undistortion as und
    a, b, c = uc.sized_camera(50, 70, 4), uc.sized_camera(5, 257, 3), uc.sized_camera(1, 1, 2)
    ta, tb, tc = (und.undistort_camera(cam_of(x), host=True) for x in (a, b, c))
    items = [(cam_of(c), tc, uc.image(1, 1, 3, 1)), (cam_of(a), ta, uc.image(50, 70, 3, 2)),
             (cam_of(b), tb, uc.image(5, 257, 0, 3)), (cam_of(a), ta, uc.image(50, 70, 4, 4))]
    before = und.stats["warp_calls"]
    ref = both(items)
    assert und.stats["warp_calls"] - before == 2  # one host call, one device call
    assert ref[1].any() and ref[2].any() and ref[3].any()
    for (s, t, img), r in zip(items, ref):
        assert np.array_equal(r, und._warp_batch([(s, t, img)], host=True)[0])


def test_exact_and_overflowing_coordinates(gpu_lib):
    """source coordinates exactly on 0 and exactly on w - 1 (the last row and column are black); coefficients that send
    source coordinates to infinity and NaN (black)"""
    src, dst, img, want = uc.quirk()
    assert np.array_equal(both([(cam_of(src), cam_of(dst), img)])[0], want)
    src, dst, img = uc.overflow()
    sx, sy = uo.source_coords(src, dst)
    assert np.isinf(sx).any() and np.isnan(sy).any()
    assert not both([(cam_of(src), cam_of(dst), img)])[0].any()


def points_both(cams, pts, src_idx, dst_idx):
    from limap_amd import undistortion as und
    ref = und._points_raw(cams, pts, src_idx, dst_idx, host=True)
    dev = und._points_raw(cams, pts, src_idx, dst_idx, host=False)
    assert np.array_equal(bits(ref[0]), bits(dev[0])), "points"
    assert np.array_equal(ref[1], dev[1]) and np.array_equal(ref[2], dev[2]), "statuses and iteration counts"
    return ref


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_point_counts(gpu_lib, n):
    from limap_amd import undistortion as und
    c = uc.cameras()["opencv_tangential"]
    target = und.undistort_camera(cam_of(c), host=True)
    out, status, iters = points_both([cam_of(c), target], uc.random_points(c, n, seed=n), 0, 1)
    assert out.shape == (n, 2) and not status.any() and (iters >= 1).all()


def test_newton_exits(gpu_lib):
    """the principal point (the step falls back to DBL_EPSILON), the stop at 100 iterations, the singular Jacobian
    (status 1, the canonical NaN), beside ordinary points in the same wave"""
    cam, p100 = uc.hundred_iterations()
    _, psing = uc.singular_jacobian()
    target = uo.make(1, (64.0, 64.0, 32.0, 16.0), cam.h, cam.w)
    pts = np.concatenate([[[32.0, 16.0]], p100, psing, uc.random_points(cam, 70, seed=3)])
    out, status, iters = points_both([cam_of(cam), cam_of(target)], pts, 0, 1)
    assert iters[:3].tolist() == [1, 100, 1] and status[:3].tolist() == [0, 0, 1]
    assert out[0].tolist() == [32.0, 16.0] and (bits(out[2]) == uo.NAN_BITS).all()


def test_mixed_cameras_in_one_scene_call(gpu_lib):
    from limap_amd import undistortion as und
    cs = uc.cameras()
    names = ["simple_radial_barrel", "full_opencv", "pinhole", "opencv_pincushion", "radial_barrel"]
    dist = {i: cam_of(cs[n], i) for i, n in enumerate(names)}
    undist = {i: und.undistort_camera(dist[i], host=True) for i in dist}
    pts = {i: uc.random_points(cs[n], 40 + 13 * i, seed=i) for i, n in enumerate(names)}
    ref = und.undistort_points_scene(pts, dist, undist, host=True, return_status=True)
    dev = und.undistort_points_scene(pts, dist, undist, host=False, return_status=True)
    for i in pts:
        assert np.array_equal(bits(ref[0][i]), bits(dev[0][i])) and np.array_equal(ref[2][i], dev[2][i])
        assert not dev[1][i].any()
    assert (dev[2][2] == 0).all() and (dev[2][1] >= 1).all()  # a pinhole source makes no Newton update


@pytest.mark.parametrize("name", uc.DISTORTED)
def test_border_scan_through_the_kernel_gives_the_host_camera(gpu_lib, name):
    from limap_amd import undistortion as und
    c = uc.cameras()[name]
    for opts in (dict(), dict(blank_pixels=1.0)):
        host_cam = und.undistort_camera(cam_of(c), host=True, **opts)
        dev_cam = und.undistort_camera(cam_of(c), host=False, **opts)
        assert host_cam.params.tolist() == dev_cam.params.tolist() and host_cam == dev_cam


def test_torch_tensors_in_place(gpu_lib):
    """device tensors are read and written in place: the same bytes as the NumPy path, with contiguous rows, with rows
    padded to a stride larger than W C, and with a start that is not on a dword"""
    import torch
    from limap_amd import undistortion as und
    items = [it for ch in (0, 3, 4) for it in sized_items(ch)[8:]]  # 3 x 2, 63 x 2, ... 257 x 5
    ref = und._warp_batch(items, host=True)
    tens = []
    for k, (s, t, img) in enumerate(items):
        if k % 3 == 0:
            tens.append(torch.from_numpy(img).cuda())
        else:  # a window of a wider tensor: the row stride is larger than W C; k % 3 == 2 starts one pixel in
            pad = np.zeros((img.shape[0], img.shape[1] + 7) + img.shape[2:], np.uint8)
            x0 = 1 if k % 3 == 2 else 0
            pad[:, x0:x0 + img.shape[1]] = img
            tens.append(torch.from_numpy(pad).cuda()[:, x0:x0 + img.shape[1]])
            assert not tens[-1].is_contiguous() or img.shape[0] == 1
    before = und.stats["warp_calls"]
    dev = und._warp_batch([(s, t, x) for (s, t, _), x in zip(items, tens)], host=False)
    assert und.stats["warp_calls"] - before == 1
    for r, d in zip(ref, dev):
        assert d.is_cuda and d.dtype == torch.uint8 and tuple(d.shape) == r.shape
        assert np.array_equal(d.cpu().numpy(), r)
    # the public call: tensors in, tensors out
    c = uc.cameras()["radial_barrel"]
    img = uc.image(c.h, c.w, 3, seed=8)
    cam_np, out_np = und.undistort_image_camera(cam_of(c), img)
    cam_t, out_t = und.undistort_image_camera(cam_of(c), torch.from_numpy(img).cuda())
    assert cam_np == cam_t and out_t.is_cuda and np.array_equal(out_t.cpu().numpy(), out_np)
    assert np.array_equal(out_np, und.undistort_image_camera(cam_of(c), img, host=True)[1])


def test_chunks_and_repeated_runs(gpu_lib):
    from limap_amd import undistortion as und
    c = uc.cameras()["full_opencv"]
    cameras = {i: cam_of(c) for i in range(3)}
    images = {i: uc.image(c.h, c.w, 3, seed=i) for i in range(3)}
    cams_h, whole_h = und.undistort_images(cameras, images, host=True)
    before = dict(und.stats)
    cams_d, whole = und.undistort_images(cameras, images)
    assert und.stats["warp_calls"] - before["warp_calls"] == 1 and und.stats["border_scans"] - before["border_scans"] == 1
    before = und.stats["warp_calls"]
    _, parts = und.undistort_images(cameras, images, max_chunk_bytes=1)
    assert und.stats["warp_calls"] - before == 3
    _, again = und.undistort_images(cameras, images)
    for i in range(3):
        assert cams_d[i] == cams_h[i]
        assert np.array_equal(whole[i], whole_h[i]) and np.array_equal(parts[i], whole[i]) and np.array_equal(again[i], whole[i])


def test_timers_and_refusals(gpu_lib):
    from limap_amd import undistortion as und
    c = uc.cameras()["radial_barrel"]
    target = und.undistort_camera(cam_of(c), host=True)
    und._warp_batch([(cam_of(c), target, uc.image(c.h, c.w, 3))])
    t = und.timers()
    assert t.shape == (4,) and t[1] > 0.0 and t[3] == target.h() * ((target.w() + 3) // 4)
    with pytest.raises(ValueError, match="pinhole"):
        und._warp_batch([(cam_of(c), cam_of(c), uc.image(c.h, c.w, 3))])
    with pytest.raises(ValueError, match="uint8"):
        und._warp_batch([(cam_of(c), target, uc.image(c.h, c.w, 3).astype(np.int16))])
