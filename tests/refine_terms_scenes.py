"""Scenes for the tests of the VP and the heatmap term of the line refinement: a ring of small pinhole cameras of two
image sizes around a box of GT 3D lines, ragged support counts, noisy 2D supports, a perturbed initial Line3d; per image a
heatmap of Gaussian ridges along the true projections; per support a vanishing point (the image of the GT direction) and a
label flag.  Everything as the CSR arrays lt_refine_arrays_terms takes, seeded."""
import ctypes as C

import numpy as np

import refine_oracle as ro
from limap_amd import _capi
from limap_amd import synthetic as syn

SIZES = ((17, 23), (24, 32))  # odd rows in FP16 (46 bytes) next to even ones


def _look_at(c, target):
    z = (target - c) / np.linalg.norm(target - c)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])  # rows: the camera axes in the world
    return ro.rot_to_quat_eigen(R), -R @ c


def _project(k, q, t, p):
    x = syn.quat_to_rot(q) @ p + t
    return np.array([k[0] * x[0] / x[2] + k[2], k[1] * x[1] / x[2] + k[3]])


def ridge_heatmap(h, w, lines2d, sigma):
    """max over the 2D lines (a, b, c) with a^2 + b^2 = 1 of exp(-d^2 / (2 sigma^2)) at (x = column, y = row)"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((h, w))
    for a, b, c in lines2d:
        out = np.maximum(out, np.exp(-((a * xx + b * yy + c) ** 2) / (2 * sigma * sigma)))
    return out


def make_scene(counts, seed=0, n_views=8, sizes=SIZES, noise_px=0.05, init_sigma=0.004, sigma_px=1.2, extra_images=2,
               direction=None, vp_label_rate=0.7, focal=1.1):
    """counts: the number of supports of every track.  The last `extra_images` images hold a heatmap and support no
    track.  direction: one 3D direction for all lines (the VP fixtures), or None for random ones."""
    rng = np.random.default_rng(seed)
    n_all = n_views + extra_images
    ids = (3 + 2 * np.arange(n_all)).astype(np.int32)
    kv, qv, tv, hw = [], [], [], []
    for v in range(n_all):
        h, w = sizes[v % len(sizes)]
        ang = 2 * np.pi * v / n_all + rng.uniform(-0.1, 0.1)
        c = np.array([4.0 * np.cos(ang), 4.0 * np.sin(ang), rng.uniform(-0.8, 0.8)])
        q, t = _look_at(c, rng.uniform(-0.15, 0.15, 3))
        kv.append([focal * w, focal * w, (w - 1) / 2.0, (h - 1) / 2.0]); qv.append(q); tv.append(t); hw.append((h, w))
    kv, qv, tv = np.array(kv), np.array(qv), np.array(tv)
    line6, gt6, off, img, l2d, l3d, flag, vp3 = [], [], [0], [], [], [], [], []
    per_image = {int(i): [] for i in ids}
    for K in counts:
        while True:
            d = rng.normal(size=3) if direction is None else np.asarray(direction, float)
            d = d / np.linalg.norm(d)
            a = rng.uniform(-0.7, 0.7, 3)
            b = a + d * rng.uniform(0.8, 1.4)
            views = np.concatenate([rng.permutation(n_views) for _ in range(K // n_views + 1)])[:K]
            sup = []
            for v in views:
                s0, s1 = np.sort(rng.uniform(0.0, 1.0, 2))
                if s1 - s0 < 0.4:
                    s0, s1 = 0.0, 1.0
                pa, pb = a + (b - a) * s0, a + (b - a) * s1
                xa, xb = _project(kv[v], qv[v], tv[v], pa), _project(kv[v], qv[v], tv[v], pb)
                sup.append((v, np.concatenate([xa, xb]) + rng.normal(0, noise_px, 4), np.concatenate([pa, pb]), xa, xb))
            if min(np.linalg.norm(s[3] - s[4]) for s in sup) >= 3.0:
                break
        gt6.append(np.concatenate([a, b]))
        line6.append(np.concatenate([a, b]) + rng.normal(0, init_sigma, 6))
        for v, seg, p3, xa, xb in sup:
            img.append(int(ids[v])); l2d.append(seg); l3d.append(p3 + rng.normal(0, 0.002, 6))
            n = np.array([xa[1] - xb[1], xb[0] - xa[0]])
            n /= np.linalg.norm(n)
            per_image[int(ids[v])].append((n[0], n[1], -n @ xa))
            K3 = np.array([[kv[v, 0], 0, kv[v, 2]], [0, kv[v, 1], kv[v, 3]], [0, 0, 1.0]])
            vp = K3 @ syn.quat_to_rot(qv[v]) @ d
            flag.append(int(rng.random() < vp_label_rate)); vp3.append(vp / np.linalg.norm(vp))
        off.append(len(img))
    heat = {}
    for v, i in enumerate(ids):
        lines = per_image[int(i)] or [(1.0, 0.0, -hw[v][1] / 2.0)]
        heat[int(i)] = ridge_heatmap(hw[v][0], hw[v][1], lines, sigma_px)
    return dict(img_ids=ids, k=np.ascontiguousarray(kv), q=np.ascontiguousarray(qv), t=np.ascontiguousarray(tv),
                hw=np.array(hw, np.int32), line6=np.array(line6), gt6=np.array(gt6), off=np.array(off, np.int64),
                img=np.array(img, np.int32), l2d=np.array(l2d), l3d=np.array(l3d), vp_flag=np.array(flag, np.int32),
                vp3=np.array(vp3), heatmaps=heat)


def texels(s, dtype=np.float16):
    """the scene's heatmaps in the texel type: ids, h, w, list of contiguous arrays (numpy's astype)"""
    ids = np.array(sorted(s["heatmaps"]), np.int32)
    arrs = [np.ascontiguousarray(s["heatmaps"][int(i)].astype(dtype)) for i in ids]
    return ids, np.array([a.shape[0] for a in arrs], np.int32), np.array([a.shape[1] for a in arrs], np.int32), arrs


def track_inputs(s, n, arrs_by_id):
    """(cam11, segs4, vp_flag, vp3, heatmaps) of track n in upstream's residual order"""
    a, b = int(s["off"][n]), int(s["off"][n + 1])
    order = np.argsort(s["img"][a:b], kind="stable") + a
    idx = {int(i): k for k, i in enumerate(s["img_ids"])}
    rows = [idx[int(i)] for i in s["img"][order]]
    cam = np.concatenate([s["k"][rows], s["q"][rows], s["t"][rows]], 1)
    return (np.ascontiguousarray(cam), np.ascontiguousarray(s["l2d"][order]), np.ascontiguousarray(s["vp_flag"][order]),
            np.ascontiguousarray(s["vp3"][order]), [arrs_by_id[int(i)] for i in s["img"][order]])


def line_distance(seg6, gt6):
    """mean distance of the GT endpoints to the infinite line through seg6"""
    a, d = seg6[:3], seg6[3:] - seg6[:3]
    d = d / np.linalg.norm(d)
    return float(np.mean([np.linalg.norm(np.cross(p - a, d)) for p in (gt6[:3], gt6[3:])]))


# ---- the native calls on a scene ----
p = _capi.ptr


def cfg_struct(L, **kw):
    c = _capi.LtRefineConfig()
    L.lt_refine_config_default(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def terms_struct(L, **kw):
    t = _capi.LtRefineTerms()
    L.lt_refine_terms_default(C.byref(t))
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _outs(T):
    return dict(params=np.zeros((T, 6)), segments=np.zeros((T, 6)), cost=np.zeros((T, 2)), iterations=np.zeros(T, np.int32),
                codes=np.zeros(T, np.int32))


def _out_ptrs(r):
    return (p(r["params"]), p(r["segments"]), p(r["cost"]), p(r["iterations"], C.c_int32), p(r["codes"], C.c_int32))


def _scene_args(s, cfg):
    return (len(s["img_ids"]), p(s["img_ids"], C.c_int32), p(s["k"]), p(s["q"]), p(s["t"]), len(s["off"]) - 1, p(s["line6"]),
            p(s["off"], C.c_int64), p(s["img"], C.c_int32), p(s["l2d"]), p(s["l3d"]), C.byref(cfg))


def _term_args(s, terms, view_hw):
    hw = s.get("hw") if view_hw else None
    return (C.byref(terms), p(s["vp_flag"], C.c_int32) if "vp_flag" in s else None, p(s["vp3"]) if "vp3" in s else None,
            None if hw is None else p(hw, C.c_int32))


def heatmap_args(tex):
    ids, h, w, arrs = tex
    ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
    return len(ids), p(ids, C.c_int32), p(h, C.c_int32), p(w, C.c_int32), ptrs


def run_host(L, s, cfg, terms, tex=None, threads=4, view_hw=True):
    """lt_fn_refine_host_terms -> (rc, results); tex: texels(s, ...) with use_heatmap"""
    r = _outs(len(s["off"]) - 1)
    hm = heatmap_args(tex) if tex is not None else (0, None, None, None, None)
    rc = L.lt_fn_refine_host_terms(*_scene_args(s, cfg), *_term_args(s, terms, view_hw), *hm, threads, *_out_ptrs(r))
    return rc, r


def run_device(ctx, s, cfg, terms, view_hw=True):
    """lt_refine_arrays_terms on the context's heatmaps -> (rc, results)"""
    L = ctx.L
    rc = L.lt_refine_arrays_terms(ctx.h, *_scene_args(s, cfg), *_term_args(s, terms, view_hw))
    r = _outs(len(s["off"]) - 1)
    if rc == 0:
        assert L.lt_refine_get(ctx.h, *_out_ptrs(r)) == 0
    return rc, r


def eval_ours(L, cam, sg, pp, terms, flag, vp3, hms, alpha=10.0):
    """lt_fn_refine_eval_terms -> dict(r (K, 3 + n), cost, g, H, failed)"""
    K = len(sg)
    n = terms.n_samples_heatmap if terms.use_heatmap else 0
    r = np.zeros((K, 3 + n)); c = C.c_double(); g = np.zeros(4); H = np.zeros(16); f = C.c_int32()
    hh = np.array([a.shape[0] for a in hms], np.int32); ww = np.array([a.shape[1] for a in hms], np.int32)
    ptrs = (C.c_void_p * K)(*[a.ctypes.data for a in hms])
    rc = L.lt_fn_refine_eval_terms(K, p(np.ascontiguousarray(cam)), p(np.ascontiguousarray(sg)),
                                   p(np.ascontiguousarray(pp, np.float64)), alpha, C.byref(terms),
                                   p(np.ascontiguousarray(flag, np.int32), C.c_int32), p(np.ascontiguousarray(vp3, np.float64)),
                                   p(hh, C.c_int32), p(ww, C.c_int32), ptrs, p(r), C.byref(f), C.byref(c), p(g), p(H))
    assert rc == 0, rc
    return dict(r=r, cost=c.value, g=g, H=H.reshape(4, 4), failed=bool(f.value))


def subset(s, tracks):
    """the scene with the given tracks only, in that order"""
    idx = np.concatenate([np.arange(s["off"][n], s["off"][n + 1]) for n in tracks]).astype(np.int64)
    out = dict(s)
    for k in ("img", "l2d", "l3d", "vp_flag", "vp3"):
        out[k] = np.ascontiguousarray(s[k][idx])
    for k in ("line6", "gt6"):
        out[k] = np.ascontiguousarray(s[k][list(tracks)])
    out["off"] = np.concatenate([[0], np.cumsum(np.diff(s["off"])[list(tracks)])]).astype(np.int64)
    return out


# ---- branch fixtures ----
def long_supports(s, factor=6.0):
    """every 2D support stretched about its midpoint: the sample lines then cross the projection outside the image on
    all four sides, and in its last rows and columns"""
    out = dict(s)
    mid = 0.5 * (s["l2d"][:, :2] + s["l2d"][:, 2:])
    half = 0.5 * (s["l2d"][:, 2:] - s["l2d"][:, :2]) * factor
    out["l2d"] = np.ascontiguousarray(np.concatenate([mid - half, mid + half], 1))
    return out


def checker_heatmaps(s):
    """1 - 2^-11 on a checkerboard: with two samples the squared norm of a block stays below Huber's a^2 = 1e-6 while
    the forward differences are not zero"""
    out = dict(s)
    out["heatmaps"] = {i: 1.0 - 2.0 ** -11 * ((np.add.outer(np.arange(a.shape[0]), np.arange(a.shape[1])) % 2) == 1)
                       for i, a in s["heatmaps"].items()}
    return out


def perpendicular_vps(s):
    """every support labelled, its vanishing point the image of a direction perpendicular to the initial line: the
    sine comes as close to its clamp at 1 as the EPS terms allow"""
    out = dict(s)
    vp3 = s["vp3"].copy()
    idx = {int(i): k for k, i in enumerate(s["img_ids"])}
    for n in range(len(s["off"]) - 1):
        d = s["line6"][n, 3:] - s["line6"][n, :3]
        e = np.cross(d, [0.3, -0.5, 0.8])
        e /= np.linalg.norm(e)
        for j in range(int(s["off"][n]), int(s["off"][n + 1])):
            v = idx[int(s["img"][j])]
            K3 = np.array([[s["k"][v, 0], 0, s["k"][v, 2]], [0, s["k"][v, 1], s["k"][v, 3]], [0, 0, 1.0]])
            vp = K3 @ syn.quat_to_rot(s["q"][v]) @ e
            vp3[j] = vp / np.linalg.norm(vp)
    out["vp3"], out["vp_flag"] = vp3, np.ones_like(s["vp_flag"])
    return out


FAIL_IDS = (901, 902, 903, 904)


def failing_track():
    """A one-track scene whose cost cannot be evaluated at the initial line: the line runs through the origin along x,
    four cameras without rotation look down +z, so it projects to the row y = cy exactly; the supports are exactly
    vertical, so every sample line is parallel to the projection and p_homo[2] = 0."""
    h, w = SIZES[0]
    k = np.array([25.0, 25.0, 11.0, 8.0])
    tv = np.array([[0, 0, 5.0], [0.25, 0, 5.0], [0, 0, 6.0], [-0.5, 0, 5.5]])
    ids = np.array(FAIL_IDS, np.int32)
    line6 = np.array([[-1.0, 0, 0, 1.0, 0, 0]])
    l2d = np.array([[9.0, 3.0, 9.0, 12.0], [12.0, 2.0, 12.0, 13.0], [8.0, 5.0, 8.0, 11.0], [10.0, 4.0, 10.0, 12.5]])
    l3d = np.array([np.concatenate([[-1.0 + 0.05 * j, 0, 0], [1.0 - 0.03 * j, 0, 0]]) for j in range(4)])
    rows = np.arange(h)[:, None] + 0.0 * np.arange(w)[None, :]
    heat = {int(i): np.exp(-((rows - 8.0) ** 2) / 4.0) for i in ids}
    return dict(img_ids=ids, k=np.tile(k, (4, 1)), q=np.tile([1.0, 0, 0, 0], (4, 1)), t=tv, hw=np.tile([h, w], (4, 1)).astype(np.int32),
                line6=line6, gt6=line6.copy(), off=np.array([0, 4], np.int64), img=ids.copy(), l2d=l2d, l3d=l3d,
                vp_flag=np.zeros(4, np.int32), vp3=np.zeros((4, 3)), heatmaps=heat)


def merge(a, b):
    """two scenes with disjoint image ids as one: b's tracks after a's"""
    out = {}
    for k in ("img_ids", "k", "q", "t", "hw", "line6", "gt6", "img", "l2d", "l3d", "vp_flag", "vp3"):
        out[k] = np.ascontiguousarray(np.concatenate([a[k], b[k]]))
    out["off"] = np.concatenate([a["off"], a["off"][-1] + b["off"][1:]]).astype(np.int64)
    out["heatmaps"] = {**a["heatmaps"], **b["heatmaps"]}
    return out
