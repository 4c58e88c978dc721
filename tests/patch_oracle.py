"""NumPy restatement of DESIGN.md section 24 (limap.features' line patches), written from the reference's sources
(features/line_patch_extractor.cc, featurepatch.h, ceresbase/interpolation.h's BiLinearInterpolator, base/linebase.cc,
base/camera_view.cc) and sharing no code with the library.  Everything is float64 NumPy, whose ufuncs round every
operation on its own (no fused multiply-add), in the operation order the section writes down; the narrowing is
``astype``, which rounds once."""
import math

import numpy as np


def _norm2(v):
    return np.sqrt(v[0] * v[0] + v[1] * v[1])


def _unit2(v):
    z = v[0] * v[0] + v[1] * v[1]
    return v / np.sqrt(z) if z > 0 else v.copy()


def _round_half_up(v):
    r = math.floor(v)
    return r + 1 if v - r >= 0.5 else r


def geometry(line4, k_stretch=1.0, t_stretch=10, range_perp=20):
    """-> (R (2, 2), tvec (2,), patch_h, patch_w)"""
    s, e = np.array(line4[:2], np.float64), np.array(line4[2:4], np.float64)
    d = e - s
    length = _norm2(d)
    direc = _unit2(d)
    perp = np.array([direc[1], -direc[0]])
    mid = 0.5 * (s + e)
    a, b = length * np.float64(k_stretch), length + np.float64(t_stretch)
    fl = np.ceil(b if a < b else a)
    s2 = mid - direc * fl / 2.0
    e2 = mid + direc * fl / 2.0
    corner = s2 - perp * np.float64(range_perp) / 2.0
    h = int(_round_half_up(float(_norm2(s2 - e2)))) + 1
    return np.stack([perp, direc]), corner, h, int(range_perp) + 1


def extract(line4, feature, k_stretch=1.0, t_stretch=10, range_perp=20, dtype=np.float64):
    """-> (array (patch_h, patch_w, C) of dtype, R, tvec, img_hw)"""
    R, tvec, h, w = geometry(line4, k_stretch, t_stretch, range_perp)
    H, W, _ = feature.shape
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    gx = (R[0, 0] * xs + R[1, 0] * ys) + tvec[0]
    gy = (R[0, 1] * xs + R[1, 1] * ys) + tvec[1]
    row, col = np.floor(gy), np.floor(gx)
    dy, dx = (gy - row)[..., None], (gx - col)[..., None]
    r0 = np.clip(row, 0, H - 1).astype(np.int64)
    r1 = np.clip(row + 1, 0, H - 1).astype(np.int64)
    c0 = np.clip(col, 0, W - 1).astype(np.int64)
    c1 = np.clip(col + 1, 0, W - 1).astype(np.int64)
    F = np.asarray(feature).astype(np.float64)
    ll, lr, ul, ur = F[r0, c0], F[r0, c1], F[r1, c0], F[r1, c1]
    v0 = (1.0 - dx) * ll + dx * lr
    v1 = (1.0 - dx) * ul + dx * ur
    f = (1.0 - dy) * v0 + dy * v1
    return f.astype(dtype), R, tvec, (H, W)


def rotation(qvec):
    """the project's camera record (DESIGN section 24 states it): the quaternion normalised as CameraPose's constructor
    does, then again as R() does, both norms summed as (w w + y y) + (x x + z z)"""
    q = np.array(qvec, np.float64)
    n0 = np.sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]))
    if n0 > 0:
        q = q / n0
    n = np.sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]))
    if n == 0:
        w, x, y, z = 1.0, q[1], q[2], q[3]
    else:
        w, x, y, z = q / n
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def project(cam11, p):
    """dehomogeneous(K (R p + T)) with the division by z + 1e-12 of the reference's EPS"""
    fx, fy, cx, cy = cam11[:4]
    R, t = rotation(cam11[4:8]), np.array(cam11[8:11], np.float64)
    v = np.array([(R[i, 0] * p[0] + R[i, 1] * p[1]) + R[i, 2] * p[2] for i in range(3)]) + t
    hx, hy, hz = fx * v[0] + cx * v[2], fy * v[1] + cy * v[2], v[2] + 1e-12
    return np.array([hx / hz, hy / hz]), v[2]


def line2d_range(line6, sup_img, sup_seg4, image_id, cam11):
    """GetLine2DRange with the loop index starting at 0 -> (range4, status): 0, 1 without a support, 2 when an endpoint
    is not in front of the camera or the range is not finite"""
    gs, z0 = project(cam11, np.array(line6[:3], np.float64))
    ge, z1 = project(cam11, np.array(line6[3:], np.float64))
    u = _unit2(ge - gs)
    proj = []
    for img, seg in zip(sup_img, sup_seg4):
        if img != image_id:
            continue
        seg = np.array(seg, np.float64)
        for p in (seg[:2], seg[2:]):
            dlt = p - gs
            proj.append(dlt[0] * u[0] + dlt[1] * u[1])
    if not proj:
        return np.zeros(4), 1
    lo, hi = min(proj), max(proj)
    a = lo if 0.0 < lo else 0.0
    length = _norm2(gs - ge)
    b = hi if hi < length else length
    out = np.concatenate([gs + u * a, gs + u * b])
    if not (z0 > 0 and z1 > 0) or not np.isfinite(out).all():
        return out, 2
    return out, 0
