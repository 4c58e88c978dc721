"""Case families of the line patch tests (tests/test_patch_host.py, tests/test_gpu_patch.py): lines on a 40 x 48 map,
option sets, channel counts, feature maps, the double-rounding fixture and the GetLine2DRange scenes."""
import numpy as np

H, W = 40, 48
SMALL_HW = (9, 11)

# name -> (x1, y1, x2, y2) on the H x W map
LINES = {
    "horizontal": (10.0, 20.0, 30.0, 20.0),
    "vertical": (24.0, 5.0, 24.0, 30.0),
    "diagonal": (5.0, 6.0, 40.0, 33.0),
    "reversed": (30.0, 20.0, 10.0, 20.0),
    "subpixel": (3.3, 4.7, 29.1, 31.9),
    "over_left": (-6.0, 10.0, 12.0, 14.5),
    "over_right": (40.0, 12.0, 55.0, 20.0),
    "over_top": (20.0, -8.0, 26.0, 9.0),
    "over_bottom": (14.0, 30.0, 18.5, 47.0),
    "outside": (-80.0, -60.0, -50.0, -70.0),
    "zero_length": (17.25, 9.5, 17.25, 9.5),
}

# k_stretch, t_stretch, range_perp
OPTIONS = {
    "default": dict(k_stretch=1.0, t_stretch=10, range_perp=20),
    "perp0": dict(k_stretch=1.0, t_stretch=10, range_perp=0),
    "perp15": dict(k_stretch=1.0, t_stretch=10, range_perp=15),   # the corner lies on half pixels
    "perp16": dict(k_stretch=1.0, t_stretch=10, range_perp=16),   # cfgs/refinement/default.yaml
    "t0": dict(k_stretch=1.0, t_stretch=0, range_perp=20),
    "k1.5": dict(k_stretch=1.5, t_stretch=10, range_perp=20),
}

CHANNELS = (1, 2, 3, 5, 8, 12, 16, 128)
DTYPES = ("float16", "float32", "float64")

# the value a double rounding (through float) gets wrong: float64 -> float16 is 1 + 2**-10, through float32 it is 1.0
TIE = 1.0 + 2.0 ** -11 + 2.0 ** -30
TIE_F16 = np.float16(1.0 + 2.0 ** -10)


def feature(h=H, w=W, c=3, dtype="float64", seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * c + h)
    return rng.standard_normal((h, w, c)).astype(dtype)


def lines_array(names=None):
    return np.array([LINES[k] for k in (names or sorted(LINES))], np.float64)


def mixed_lines(n, hw=(H, W), seed=0):
    """n lines whose patches have between 1 and about 80 rows with t_stretch = 0: the first is of zero length, the
    rest grow in length, at every angle, some hanging over the edges"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 4))
    for i in range(n):
        length = 0.0 if i == 0 else 79.0 * i / max(n - 1, 1)
        ang = rng.uniform(0, 2 * np.pi)
        mid = np.array([rng.uniform(-4, hw[1] + 4), rng.uniform(-4, hw[0] + 4)])
        half = 0.5 * length * np.array([np.cos(ang), np.sin(ang)])
        out[i, :2], out[i, 2:] = mid - half, mid + half
    return out


# ---- GetLine2DRange scenes: camera, 3D line, supports ----
CAM11 = np.array([500.0, 480.0, 24.0, 20.0, 0.98, 0.05, -0.12, 0.03, 0.2, -0.1, 0.4])
LINE6 = np.array([-0.20, -0.15, 6.0, 0.25, 0.20, 7.0])


def range_scenes(project):
    """name -> (sup_img, sup_seg4, image_id): `project(cam11, p)` -> the 2D point; supports are laid along the
    projection g of LINE6 at given fractions of its length, one pixel off it"""
    gs, ge = project(CAM11, LINE6[:3])[0], project(CAM11, LINE6[3:])[0]
    d = ge - gs
    nrm = np.array([-d[1], d[0]]) / np.hypot(*d)

    def seg(a, b, off=1.0):
        return np.concatenate([gs + a * d + off * nrm, gs + b * d + off * nrm])

    return {
        "one_support": ([7], [seg(0.2, 0.7)], 7),
        "several": ([7, 7, 7], [seg(0.5, 0.3), seg(0.1, 0.4, -2.0), seg(0.6, 0.85)], 7),
        "beyond_both_ends": ([7, 7], [seg(-0.4, 0.3), seg(0.5, 1.6)], 7),
        "other_image_ignored": ([3, 7, 3], [seg(-0.5, 1.5), seg(0.25, 0.5), seg(0.0, 1.0)], 7),
        "reversed_support": ([7], [seg(0.9, 0.15)], 7),
    }
