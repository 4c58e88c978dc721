"""Inputs of the dense-warp matcher's tests ("Dense"): lines, homography warps at any resolution,
certainty maps with holes, and the constructed cases that put a value exactly on a threshold.  Shared by
tests/golden/make_match_dense_golden.py, tests/test_match_dense_host.py and tests/test_gpu_match_dense.py; nothing here
reads the reference."""
import numpy as np

TILE = 16  # kDenseTile: lines per side of a workgroup's tile in k_dense_pairs


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def descinfo(lines, shape):
    """what DenseNaiveExtractor.extract returns, without the image"""
    lines = np.asarray(lines, np.float64).reshape(-1, 2, 2)
    return {"image": None, "image_shape": tuple(int(v) for v in shape), "lines": lines,
            "scores": np.ones(lines.shape[0])}


def rand_lines(rng, n, shape, min_len=20.0):
    """n segments inside an (h, w) image, (n, 2, 2)"""
    h, w = shape[0], shape[1]
    out = np.zeros((n, 2, 2))
    for k in range(n):
        while True:
            p = rng.uniform([4, 4], [w - 4, h - 4], (2, 2))
            if np.linalg.norm(p[0] - p[1]) >= min_len:
                break
        out[k] = p
    return out


def apply_h(H, pts):
    q = np.concatenate([pts, np.ones(pts.shape[:-1] + (1,))], -1) @ np.asarray(H, np.float64).T
    return q[..., :2] / q[..., 2:]


def small_homography(rng, shape, amount=0.04):
    """a homography near the identity in pixel coordinates of an (h, w) image"""
    h, w = shape[0], shape[1]
    a = 1.0 + rng.uniform(-amount, amount)
    t = rng.uniform(-amount, amount)
    H = np.array([[a * np.cos(t), -a * np.sin(t), rng.uniform(-0.05, 0.05) * w],
                  [a * np.sin(t), a * np.cos(t), rng.uniform(-0.05, 0.05) * h],
                  [rng.uniform(-1, 1) * amount / w, rng.uniform(-1, 1) * amount / h, 1.0]])
    return H


def homography_warp(H, dims, src_shape, dst_shape):
    """warp (hw, ww, 2) float32: texel (y, x) holds the normalised coordinates in the target image of the source point
    under its centre, as a dense matcher returns it"""
    hw, ww = dims
    xs = ((np.arange(ww) + 0.5) / ww) * src_shape[1]
    ys = ((np.arange(hw) + 0.5) / hw) * src_shape[0]
    grid = np.stack(np.meshgrid(xs, ys), -1)
    t = apply_h(H, grid)
    return np.stack([2.0 / dst_shape[1] * t[..., 0] - 1.0, 2.0 / dst_shape[0] * t[..., 1] - 1.0], -1).astype(np.float32)


def identity_warp(dims):
    hw, ww = dims
    xs = 2.0 * (np.arange(ww) + 0.5) / ww - 1.0
    ys = 2.0 * (np.arange(hw) + 0.5) / hw - 1.0
    return np.stack(np.meshgrid(xs, ys), -1).astype(np.float32)


def cert_with_holes(rng, dims, holes=3, high=0.9):
    """plateaus of `high` with rectangular holes of 0"""
    hw, ww = dims
    c = np.full((hw, ww), high, np.float32)
    for _ in range(holes):
        y0, x0 = int(rng.integers(0, max(hw - 1, 1))), int(rng.integers(0, max(ww - 1, 1)))
        c[y0:y0 + max(hw // 5, 1), x0:x0 + max(ww // 5, 1)] = 0.0
    return c


def homography_pair(rng, n1, n2, shape1, shape2, dims12, dims21, noise=0.5, holes=0, n_true=None):
    """two images related by a homography: the first n_true lines of image 2 are image 1's lines transformed, with
    endpoint noise; the rest are random.  -> descinfo1, descinfo2, (warp_12, cert_12, warp_21, cert_21)"""
    sx, sy = shape2[1] / shape1[1], shape2[0] / shape1[0]
    H = np.diag([sx, sy, 1.0]) @ small_homography(rng, shape1)
    l1 = rand_lines(rng, n1, shape1)
    n_true = min(n1, n2) if n_true is None else n_true
    l2 = rand_lines(rng, n2, shape2)
    l2[:n_true] = apply_h(H, l1[:n_true]) + rng.normal(0, noise, (n_true, 2, 2))
    w12 = homography_warp(H, dims12, shape1, shape2)
    w21 = homography_warp(np.linalg.inv(H), dims21, shape2, shape1)
    c12 = cert_with_holes(rng, dims12, holes)
    c21 = cert_with_holes(rng, dims21, holes)
    return descinfo(l1, shape1), descinfo(l2, shape2), (w12, c12, w21, c21)


def random_pair(rng, n1, n2, dims12=(5, 3), dims21=(5, 3), shape1=(48, 64), shape2=(40, 56), spread=1.3):
    """lines and warps without structure: warp values beyond [-1, 1], certainties around the threshold 0.5 -- many
    samples leave the maps, many entries sit near the rejections"""
    d1 = descinfo(rand_lines(rng, n1, shape1, 5.0), shape1)
    d2 = descinfo(rand_lines(rng, n2, shape2, 5.0), shape2)
    mk = lambda d: (rng.uniform(-spread, spread, d + (2,)).astype(np.float32), rng.uniform(0, 1, d).astype(np.float32))
    w12, c12 = mk(tuple(dims12))
    w21, c21 = mk(tuple(dims21))
    return d1, d2, (w12, c12, w21, c21)


def overlapping_pair(rng, n1, n2, shape=(48, 64), dims=(40, 56), jitter=1.0):
    """both images the same size, identity warps, lines of image 2 drawn near lines of image 1: many entries under
    pixel_th, several per row"""
    l1 = rand_lines(rng, n1, shape)
    l2 = np.zeros((n2, 2, 2))
    for j in range(n2):
        l2[j] = (l1[j % n1] if n1 else rand_lines(rng, 1, shape)[0]) + rng.normal(0, jitter, (2, 2))
    w = identity_warp(dims)
    c = np.full(dims, 0.9, np.float32)
    return descinfo(l1, shape), descinfo(l2, shape), (w, c, w.copy(), c.copy())


# ---------------------------------------------------------------------------------------------------------------------
# values exactly on the thresholds.  Images and warps are 64 x 64 and every line coordinate is a half-integer, so with
# n_samples 2 or 5 every sample is a texel centre (one tap of weight 1, three of weight 0), the maps are constant apart
# from single texels, and every number on the way is exact in FP32.
SHAPE64 = (64, 64)


def constant_maps(x_px, y_px, cert):
    """a 64 x 64 warp that sends every sample to the pixel (x_px, y_px) of a 64 x 64 image, with certainty `cert`"""
    w = np.zeros((64, 64, 2), np.float32)
    w[..., 0], w[..., 1] = 2.0 / 64 * x_px - 1.0, 2.0 / 64 * y_px - 1.0
    return w, np.full((64, 64), cert, np.float32)


def threshold_case(name):
    """-> descinfo1, descinfo2, warps, options as a dict, sample_thresh, the rows the definition gives.
    Image 1 has the line (8.5, 32.5) - (56.5, 32.5), image 2 the line (16.5, 32.5) - (48.5, 32.5): unit direction
    (1, 0), end projections 16.5 and 48.5, homogeneous line (0, 1, -32.5).  Direction 2 -> 1 sends everything to
    (32.5, 33) -- inside line 1, half a pixel off -- unless the case says otherwise."""
    a = descinfo([[[8.5, 32.5], [56.5, 32.5]]], SHAPE64)
    b = descinfo([[[16.5, 32.5], [48.5, 32.5]]], SHAPE64)
    opts = dict(n_samples=5, segment_percentage_th=0.2, pixel_th=10.0, one_to_many=False)
    thresh, want = 0.5, [[0, 0]]
    back = constant_maps(32.5, 33.0, 0.9)
    fwd = constant_maps(32.5, 32.5, 0.9)
    if name == "cert_equal":            # a certainty equal to the threshold is not above it
        fwd, want = constant_maps(32.5, 32.5, 0.5), []
    elif name == "cert_above":
        fwd = constant_maps(32.5, 32.5, float(np.nextafter(np.float32(0.5), np.float32(1))))
    elif name == "proj_at_start":       # a projection equal to the segment's start is not inside
        fwd, want = constant_maps(16.5, 32.5, 0.9), []
    elif name == "proj_at_end":
        fwd, want = constant_maps(48.5, 32.5, 0.9), []
    elif name == "proj_inside":
        fwd = constant_maps(17.5, 32.5, 0.9)
    elif name in ("dmax_equal", "dmax_above"):   # max(d_12, d_21) against pixel_th: equal is not above (S = 2: 1 / 2 exact)
        opts["n_samples"] = 2
        fwd = constant_maps(32.5, 42.5 if name == "dmax_equal" else 43.0, 0.9)
        want = want if name == "dmax_equal" else []
    elif name in ("dists_equal", "dists_far"):   # the chosen distance against pixel_th: equal still matches
        opts["n_samples"] = 2
        fwd = constant_maps(32.5, 42.5, 0.9)
        back[1][32, 16] = 0.0           # one of line 2's two samples fails: overlap_21 = 0.5 < overlap_12 = 1, d_12 is chosen
        if name == "dists_far":
            opts["pixel_th"], want = float(np.nextafter(np.float32(10), np.float32(0))), []
    elif name in ("overlap_equal", "overlap_below"):
        # one good sample of five (the texel under line 1's END, r = 0): fl(1 / 5) against 0.2f -- equal is not below
        fwd[1][:] = 0.0
        fwd[1][32, 56] = 0.9
        if name == "overlap_below":
            opts["segment_percentage_th"], want = float(np.nextafter(np.float32(0.2), np.float32(1))), []
    elif name != "plain":
        raise KeyError(name)
    return a, b, (fwd[0], fwd[1], back[0], back[1]), opts, thresh, np.array(want, np.int32).reshape(-1, 2)


THRESHOLD_CASES = ["plain", "cert_equal", "cert_above", "proj_at_start", "proj_at_end", "proj_inside", "dmax_equal",
                   "dmax_above", "dists_equal", "dists_far", "overlap_equal", "overlap_below"]
