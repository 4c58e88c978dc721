"""Scenes for the bundle-adjustment tests: cameras on a ring around a box of 3D points and lines,
every structure projected with Gaussian pixel noise, poses and structure perturbed from the ground truth.  Everything
as the arrays lt_ba_arrays takes; `obs` lists fix the observation count of the first tracks (beyond the number of
cameras an image observes a track more than once)."""
import numpy as np


def rot_to_quat(R):
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        return np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
    q = np.zeros(4)
    q[0] = (R[k, j] - R[j, k]) / s
    q[1 + i] = 0.25 * s
    q[1 + j] = (R[j, i] + R[i, j]) / s
    q[1 + k] = (R[k, i] + R[i, k]) / s
    return q


def quat_to_rot(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def ring_cameras(rng, n, radius=6.0):
    """n cameras around the origin looking at it: (k (n, 4), q (n, 4), t (n, 3))"""
    k = np.tile(np.array([600.0, 590.0, 400.0, 300.0]), (n, 1))
    q, t = np.zeros((n, 4)), np.zeros((n, 3))
    for i in range(n):
        a = 2 * np.pi * i / n + rng.uniform(-0.1, 0.1)
        c = np.array([radius * np.cos(a), radius * np.sin(a), rng.uniform(-1.0, 1.5)])
        z = -c / np.linalg.norm(c)
        x = np.cross(z, np.array([0.0, 0.0, 1.0]))
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        q[i] = rot_to_quat(R)
        t[i] = -R @ c
    return k, q, t


def project(k, q, t, X):
    x = quat_to_rot(q) @ X + t
    return np.array([k[0] * x[0] / x[2] + k[2], k[1] * x[1] / x[2] + k[3]])


def make_scene(n_cams=4, n_points=24, n_lines=6, seed=0, noise_px=0.5, pose_sigma=0.01, struct_sigma=0.02, point_obs=None,
               line_obs=None, id_step=3, id_offset=5, extra_images=()):
    """point_obs / line_obs: observation counts of the first tracks (the others see every camera once).  extra_images:
    image ids added to the collection without any observation.  Returns the arrays and the ground truth."""
    rng = np.random.default_rng(seed)
    k, q_gt, t_gt = ring_cameras(rng, n_cams)
    ids = (id_offset + id_step * np.arange(n_cams)).astype(np.int32)
    q, t = q_gt.copy(), t_gt.copy()
    for i in range(n_cams):
        dq = np.concatenate([[1.0], rng.normal(0, pose_sigma, 3)])
        q[i] = quat_mul(dq / np.linalg.norm(dq), q_gt[i])
        t[i] = t_gt[i] + rng.normal(0, 5 * pose_sigma, 3)
    point_obs = list(point_obs or [])
    line_obs = list(line_obs or [])
    p_gt = rng.uniform(-1.0, 1.0, (n_points, 3))
    poff, pimg, pxy = [0], [], []
    for n in range(n_points):
        cnt = point_obs[n] if n < len(point_obs) else n_cams
        cams = [(n + j) % n_cams for j in range(cnt)]
        for c in cams:
            pimg.append(int(ids[c]))
            pxy.append(project(k[c], q_gt[c], t_gt[c], p_gt[n]) + rng.normal(0, noise_px, 2))
        poff.append(len(pimg))
    gt6 = np.zeros((n_lines, 6))
    loff, limg, l2d, l3d = [0], [], [], []
    for n in range(n_lines):
        a = rng.uniform(-1.0, 1.0, 3)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        b = a + d * rng.uniform(0.8, 1.6)
        gt6[n] = np.concatenate([a, b])
        cnt = line_obs[n] if n < len(line_obs) else n_cams
        # list order is not image order: the plan sorts
        cams = [(2 * n + 3 * j) % n_cams for j in range(cnt)]
        for c in cams:
            s0, s1 = np.sort(rng.uniform(0.0, 1.0, 2))
            if s1 - s0 < 0.3:
                s0, s1 = 0.05, 0.95
            pa, pb = a + (b - a) * s0, a + (b - a) * s1
            limg.append(int(ids[c]))
            l2d.append(np.concatenate([project(k[c], q_gt[c], t_gt[c], pa), project(k[c], q_gt[c], t_gt[c], pb)]) +
                       rng.normal(0, noise_px, 4))
            l3d.append(np.concatenate([pa, pb]) + rng.normal(0, 0.01, 6))
        loff.append(len(limg))
    p3 = p_gt + rng.normal(0, struct_sigma, p_gt.shape)
    line6 = gt6 + rng.normal(0, struct_sigma, gt6.shape)
    if len(extra_images):
        ex = np.array(extra_images, np.int32)
        ids = np.concatenate([ids, ex])
        m = len(ex)
        k = np.concatenate([k, np.tile(k[:1], (m, 1))])
        qe = rng.normal(size=(m, 4))
        q = np.concatenate([q, qe]); q_gt = np.concatenate([q_gt, qe])
        te = rng.normal(size=(m, 3))
        t = np.concatenate([t, te]); t_gt = np.concatenate([t_gt, te])
        order = np.argsort(ids, kind="stable")
        ids, k, q, t, q_gt, t_gt = ids[order], k[order], q[order], t[order], q_gt[order], t_gt[order]
    c = np.ascontiguousarray
    return dict(img_ids=c(ids, np.int32), k=c(k), q=c(q), t=c(t), q_gt=c(q_gt), t_gt=c(t_gt),
                p3=c(p3.reshape(-1, 3)), p_gt=c(p_gt.reshape(-1, 3)), poff=np.array(poff, np.int64),
                pimg=np.array(pimg, np.int32).reshape(-1), pxy=c(np.array(pxy, float).reshape(-1, 2)),
                line6=c(line6.reshape(-1, 6)), gt6=c(gt6.reshape(-1, 6)), loff=np.array(loff, np.int64),
                limg=np.array(limg, np.int32).reshape(-1), l2d=c(np.array(l2d, float).reshape(-1, 4)),
                l3d=c(np.array(l3d, float).reshape(-1, 6)))


def at_ground_truth(s):
    """the scene with poses and structure at the ground truth (the observations keep their noise)"""
    g = dict(s)
    g.update(q=s["q_gt"].copy(), t=s["t_gt"].copy(), p3=s["p_gt"].copy(), line6=s["gt6"].copy())
    return g


def without_points(s):
    g = dict(s)
    g.update(p3=np.zeros((0, 3)), p_gt=np.zeros((0, 3)), poff=np.zeros(1, np.int64), pimg=np.zeros(0, np.int32), pxy=np.zeros((0, 2)))
    return g


def without_lines(s, keep=()):
    """only the line tracks in `keep`"""
    g = dict(s)
    keep = list(keep)
    off = [0]
    sel = []
    for n in keep:
        sel += list(range(int(s["loff"][n]), int(s["loff"][n + 1])))
        off.append(len(sel))
    sel = np.array(sel, np.int64)
    g.update(line6=np.ascontiguousarray(s["line6"][keep].reshape(-1, 6)), gt6=np.ascontiguousarray(s["gt6"][keep].reshape(-1, 6)),
             loff=np.array(off, np.int64), limg=np.ascontiguousarray(s["limg"][sel]), l2d=np.ascontiguousarray(s["l2d"][sel].reshape(-1, 4)),
             l3d=np.ascontiguousarray(s["l3d"][sel].reshape(-1, 6)))
    return g


def chain_scene(n_cams, seed=0, pts_per_pair=3):
    """many cameras, few observations: about pts_per_pair points per consecutive camera pair, each seen by three
    consecutive cameras, no lines: the camera-count edges of the Schur and Cholesky kernels at a small cost"""
    rng = np.random.default_rng(seed)
    s = make_scene(n_cams=n_cams, n_points=0, n_lines=0, seed=seed)
    k, q_gt, t_gt, ids = s["k"], s["q_gt"], s["t_gt"], s["img_ids"]
    p_gt, poff, pimg, pxy = [], [0], [], []
    for c in range(n_cams):
        for _ in range(pts_per_pair):
            X = rng.uniform(-1.0, 1.0, 3)
            p_gt.append(X)
            for j in range(3):
                cc = (c + j) % n_cams
                pimg.append(int(ids[cc]))
                pxy.append(project(k[cc], q_gt[cc], t_gt[cc], X) + rng.normal(0, 0.5, 2))
            poff.append(len(pimg))
    p_gt = np.array(p_gt)
    s.update(p_gt=p_gt, p3=p_gt + rng.normal(0, 0.02, p_gt.shape), poff=np.array(poff, np.int64),
             pimg=np.array(pimg, np.int32), pxy=np.ascontiguousarray(np.array(pxy)))
    return s


# ---- the native calls on a scene ----
def cfg_of(**kw):
    import ctypes as C
    from limap_amd import _capi
    c = _capi.LtBaConfig()
    _capi.load_library().lt_ba_config_default(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def args_of(s, cfg):
    import ctypes as C
    from limap_amd import _capi
    p = _capi.ptr
    return (len(s["img_ids"]), p(s["img_ids"], C.c_int32), p(s["k"], C.c_double), p(s["q"], C.c_double), p(s["t"], C.c_double),
            len(s["poff"]) - 1, p(s["p3"], C.c_double), p(s["poff"], C.c_int64), p(s["pimg"], C.c_int32), p(s["pxy"], C.c_double),
            len(s["loff"]) - 1, p(s["line6"], C.c_double), p(s["loff"], C.c_int64), p(s["limg"], C.c_int32),
            p(s["l2d"], C.c_double), p(s["l3d"], C.c_double), C.byref(cfg))


def _outs(s):
    N, NP, NL = len(s["img_ids"]), len(s["poff"]) - 1, len(s["loff"]) - 1
    return dict(qvec=np.zeros((N, 4)), tvec=np.zeros((N, 3)), points=np.zeros((NP, 3)), params=np.zeros((NL, 6)),
                segments=np.zeros((NL, 6)), cost=np.zeros(2), iterations=np.zeros(1, np.int32), code=np.zeros(1, np.int32))


def _out_ptrs(o):
    import ctypes as C
    from limap_amd import _capi
    p = _capi.ptr
    return tuple(p(o[k], C.c_double) for k in ("qvec", "tvec", "points", "params", "segments", "cost")) + \
        (p(o["iterations"], C.c_int32), p(o["code"], C.c_int32))


def run_host(s, cfg, threads=4):
    """lt_fn_ba_host -> (return code, outputs)"""
    from limap_amd import _capi
    o = _outs(s)
    rc = _capi.load_library().lt_fn_ba_host(*args_of(s, cfg), int(threads), *_out_ptrs(o))
    return rc, o


def run_device(ctx, s, cfg):
    """lt_ba_arrays + lt_ba_get -> (return code, outputs)"""
    o = _outs(s)
    rc = ctx.L.lt_ba_arrays(ctx.h, *args_of(s, cfg))
    if rc == 0:
        ctx.chk(ctx.L.lt_ba_get(ctx.h, *_out_ptrs(o)))
    return rc, o


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)
