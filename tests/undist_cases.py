"""Case families of the undistortion tests (tests/test_undist_host.py, tests/test_gpu_undist.py): cameras of every
built model with barrel and pincushion coefficients, tangential terms, one and two focal lengths; small images with
random bytes; the points that drive the Newton loop to each of its exits.  The shapes are the smallest at which the
kernels can go wrong, not photographs."""
import numpy as np

import undist_oracle as uo

H, W = 30, 40  # the image of the model cases: more than one row of runs, a width that is a multiple of the run


def cameras():
    """name -> oracle Cam (h = 30, w = 40): every built model, both signs of the radial terms, tangential terms"""
    return {
        "simple_pinhole": uo.make(0, (50.0, 20.3, 14.6), H, W),
        "pinhole": uo.make(1, (48.0, 52.0, 19.7, 15.2), H, W),
        "simple_radial_barrel": uo.make(2, (50.0, 20.3, 14.6, -0.2), H, W),
        "simple_radial_pincushion": uo.make(2, (50.0, 19.4, 15.3, 0.15), H, W),
        "radial_barrel": uo.make(3, (45.0, 20.1, 15.2, -0.25, 0.05), H, W),
        "radial_pincushion": uo.make(3, (55.0, 19.8, 14.9, 0.1, 0.02), H, W),
        "opencv_tangential": uo.make(4, (48.0, 52.0, 20.4, 14.7, -0.15, 0.03, 0.01, -0.008), H, W),
        "opencv_pincushion": uo.make(4, (52.0, 47.0, 19.6, 15.4, 0.2, 0.01, -0.005, 0.004), H, W),
        "full_opencv": uo.make(6, (50.0, 49.0, 20.2, 15.1, -0.2, 0.04, 0.003, -0.002, 0.01, 0.02, -0.01, 0.005), H, W),
        "full_opencv_pincushion": uo.make(6, (51.0, 53.0, 19.9, 14.8, 0.12, 0.02, -0.004, 0.006, 0.0, -0.03, 0.0, 0.0), H, W),
    }


DISTORTED = [n for n in cameras() if "pinhole" not in n]


def image(h, w, ch, seed=0):
    """random bytes, (h, w) for ch == 0 else (h, w, ch)"""
    rng = np.random.default_rng(1000 * seed + 7 * h + 13 * w + ch)
    return rng.integers(0, 256, (h, w) if ch == 0 else (h, w, ch), dtype=np.uint8)


def sized_camera(h, w, model=2, sign=-1.0):
    """a distorted camera for an image of any size >= 1: the focal length follows the larger side"""
    f = 1.2 * max(h, w, 4)
    cx, cy = w / 2 + 0.3, h / 2 - 0.2
    if model == 2:
        return uo.make(2, (f, cx, cy, 0.1 * sign), h, w)
    if model == 4:
        return uo.make(4, (f, 1.1 * f, cx, cy, 0.12 * sign, 0.02, 0.004, -0.003), h, w)
    return uo.make(3, (f, cx, cy, 0.1 * sign, 0.01), h, w)


def quirk():
    """SIMPLE_RADIAL with k = 0, f = 64, a dyadic principal point: every coordinate is exact, the warp maps target
    pixel (x, y) to source (x, y), and the source coordinate w - 1 (h - 1) is black: the source with its last row and
    column 0.  -> (source Cam, target Cam, image, expected)"""
    h, w = 6, 9
    src = uo.make(2, (64.0, 4.5, 3.25, 0.0), h, w)
    dst = uo.make(1, (64.0, 64.0, 4.5, 3.25), h, w)
    img = image(h, w, 3, seed=5)
    want = img.copy()
    want[-1] = 0
    want[:, -1] = 0
    return src, dst, img, want


def overflow():
    """coefficients so large that source coordinates overflow to infinity (and to NaN on the row whose normalised
    ordinate is 0, where 0 meets an infinite radial factor): every target pixel is black.  -> (source Cam, target Cam, image)"""
    h, w = 5, 70
    src = uo.make(3, (1.0, 32.0, 2.5, 1e308, 1e308), h, w)
    dst = uo.make(1, (1.0, 1.0, 32.0, 2.5), h, w)
    return src, dst, image(h, w, 3, seed=6)


def grid_points(cam, n=9):
    """an n x n grid over the image, its corners included"""
    xs, ys = np.linspace(0.0, cam.w, n), np.linspace(0.0, cam.h, n)
    return np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)


def random_points(cam, n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform([0.0, 0.0], [cam.w, cam.h], (n, 2))


def singular_jacobian():
    """SIMPLE_RADIAL, k = -1, the point that normalises to (1, 0): the step along v falls back to DBL_EPSILON, r2 rounds
    to 1, the finite difference of dv is exactly -1 and J = diag(-2, 0); its second residual is 0, so the elimination
    divides 0 by 0.  -> (Cam, point)"""
    cam = uo.make(2, (64.0, 32.0, 16.0, -1.0), 32, 64)
    return cam, np.array([[96.0, 16.0]])


def hundred_iterations():
    """SIMPLE_RADIAL, k = -1, a point beyond the fold of r (1 - r^2) at r = 1 / sqrt(3): Newton's updates keep
    jumping across the fold and the loop ends at its 100 updates with a finite point (the search below fixes which
    point; the test asserts the count on the restatement).  -> (Cam, point)"""
    cam = uo.make(2, (64.0, 32.0, 16.0, -1.0), 32, 64)
    return cam, np.array([[HUNDRED_X, 16.0]])


HUNDRED_X = 57.5
