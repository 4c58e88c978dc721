"""Seeded synthetic scenes for the feature-consistency term (tests only): 3D lines on one plane, 4 to 6 views each, and
per view a (48, 64, 128) feature map that is a smooth per-channel field of the plane point a pixel sees -- so the views
agree along every line of the plane -- with the patches cut from those maps by limap_amd.features on the host path."""
import ctypes as C

import numpy as np

import patch_oracle as po
from limap_amd import _capi, features, optimize
from limap_amd.base import ImageCollection, Line2d, Line3d, LineTrack

H, W, CH = 48, 64, 128
PLANE = np.array([0.1, 0.05, -1.0, 4.0])  # z = 4 + 0.1 x + 0.05 y
PATCH_CFG = dict(patch=dict(k_stretch=1.0, t_stretch=4, range_perp=15), channels=CH, dtype="float16")
N_CAMS = 7


def _cameras(rng, n_cams, hw):
    sc = hw[0] / H
    k = np.tile([60.0 * sc, 62.0 * sc, hw[1] / 2.0, hw[0] / 2.0], (n_cams, 1))
    q = np.concatenate([np.ones((n_cams, 1)), rng.uniform(-0.04, 0.04, (n_cams, 3))], 1)
    q[:, 3] += rng.uniform(-0.15, 0.15, n_cams)  # some roll: rotated patches
    q /= np.linalg.norm(q, axis=1)[:, None]
    centres = np.stack([rng.uniform(-0.5, 0.5, n_cams), rng.uniform(-0.3, 0.3, n_cams), rng.uniform(-0.2, 0.2, n_cams)], 1)
    t = np.array([-po.rotation(q[i]) @ centres[i] for i in range(n_cams)])
    return k, q, t


def _plane_z(x, y):
    return PLANE[3] + PLANE[0] * x + PLANE[1] * y


def render_map(cam11, freq, phase, hw=(H, W), dtype=np.float64):
    """the field sin(freq_c . X + phase_c) at the plane point X every pixel's ray meets"""
    fx, fy, cx, cy = cam11[:4]
    R, t = po.rotation(cam11[4:8]), cam11[8:11]
    ys, xs = np.mgrid[0:hw[0], 0:hw[1]].astype(np.float64)
    rays = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], -1) @ R  # R^T ray
    c = -R.T @ t
    n, d0 = np.array([PLANE[0], PLANE[1], -1.0]), PLANE[3]  # n . X + d0 = 0
    lam = -(c @ n + d0) / (rays @ n)
    X = c + lam[..., None] * rays
    return np.sin((X @ freq.T + phase).astype(dtype))


def make_scene(counts=(5, 4, 6), seed=0, init_sigma=0.004, noise_px=0.02, double_support=True, n_cams=N_CAMS, hw=(H, W),
               map_dtype=np.float64):
    """len(counts) tracks, track n seen in counts[n] of the n_cams cameras (image ids 10, 11, ..); hw: the size of the
    images and maps (the tests keep the default)"""
    rng = np.random.default_rng(seed)
    k, q, t = _cameras(rng, n_cams, hw)
    ids = np.arange(10, 10 + n_cams, dtype=np.int32)
    cam11 = np.concatenate([k, q, t], 1)
    freq, phase = rng.uniform(-3.0, 3.0, (CH, 3)), rng.uniform(0, 2 * np.pi, CH)
    maps = {int(i): render_map(cam11[n], freq, phase, hw, map_dtype) for n, i in enumerate(ids)}
    line6, gt6, off, img, l2d, l3d = [], [], [0], [], [], []
    for cnt in counts:
        while True:
            a, b = rng.uniform([-0.8, -0.45], [0.8, 0.45], (2, 2))
            if np.linalg.norm(a - b) > 0.9:
                break
        gt = np.array([a[0], a[1], _plane_z(*a), b[0], b[1], _plane_z(*b)])
        for cam in np.sort(rng.choice(n_cams, cnt, replace=False)):
            ends = [po.project(cam11[cam], gt[:3])[0], po.project(cam11[cam], gt[3:])[0]]
            parts = [(0.0, 1.0)] if not (double_support and rng.random() < 0.4) else [(0.0, 0.55), (0.35, 1.0)]
            for lo, hi in parts:
                s = ends[0] + lo * (ends[1] - ends[0]) + rng.normal(0, noise_px, 2)
                e = ends[0] + hi * (ends[1] - ends[0]) + rng.normal(0, noise_px, 2)
                img.append(int(ids[cam])); l2d.append(np.concatenate([s, e]))
                l3d.append(gt + rng.normal(0, 0.01, 6))
        gt6.append(gt)
        line6.append(gt + rng.normal(0, init_sigma, 6))
        off.append(len(img))
    s = dict(img_ids=ids, k=k, q=q, t=t, cam11=cam11, maps=maps, hw=tuple(hw), line6=np.array(line6), gt6=np.array(gt6),
             off=np.array(off, np.int64), img=np.array(img, np.int32), l2d=np.array(l2d), l3d=np.array(l3d))
    return s


def cams_of(s):
    return {int(i): s["cam11"][n] for n, i in enumerate(s["img_ids"])}


def imagecols(s):
    return ImageCollection.from_arrays(s["img_ids"], s["k"], s["q"], s["t"], hw=s.get("hw", (H, W)))


def tracks_of(s):
    out = []
    for n in range(len(s["line6"])):
        a, b = int(s["off"][n]), int(s["off"][n + 1])
        t = LineTrack(Line3d(s["line6"][n, :3], s["line6"][n, 3:]), s["img"][a:b].tolist(), list(range(a, b)),
                      [Line2d(s["l2d"][k, :2], s["l2d"][k, 2:]) for k in range(a, b)])
        t.line3d_list = [Line3d(s["l3d"][k, :3], s["l3d"][k, 3:]) for k in range(a, b)]
        t.node_id_list, t.score_list = list(range(a, b)), [1.0] * (b - a)
        out.append(t)
    return out


def sorted_ids(s, n):
    return sorted(set(int(i) for i in s["img"][s["off"][n]:s["off"][n + 1]]))


def patches_of(s, dtype="float16", tracks=None):
    """{(track, img_id): PatchInfo} from limap_amd.features' host path, texels of `dtype`"""
    return features.extract_track_patches(dict(PATCH_CFG, dtype=dtype), tracks or tracks_of(s), imagecols(s), s["maps"],
                                          host=True, dtype=dtype)


def texel_maps(s, dtype="float16"):
    return {i: m.astype(dtype) for i, m in s["maps"].items()}


def texel_digest(m):
    """the SHA-256 of a map's texels (the goldens record it: they hold the maps' recipe, not the maps)"""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest()


def oracle_grids(s, n, form, src):
    """{img_id: (array, R, tvec)} of track n; src: patches_of(..) or texel_maps(..)"""
    if form == "patch":
        return {i: (np.asarray(src[(n, i)].array), src[(n, i)].R, src[(n, i)].tvec) for i in sorted_ids(s, n)}
    return {i: (src[i], np.eye(2), np.zeros(2)) for i in sorted_ids(s, n)}


def native_grids(s, tracks, form, src, keep):
    """the grid tuples of optimize.refine_arrays for the tracks (indices into s), host arrays; keep: a list that holds them"""
    out = []
    for n in tracks:
        for i in sorted_ids(s, n):
            a, R, tv = oracle_grids(s, n, form, src)[i]
            a = np.ascontiguousarray(a)
            keep.append(a)
            out.append((a.ctypes.data, a.shape[0], a.shape[1], np.asarray(R, float).reshape(4), np.asarray(tv, float).reshape(2), 0))
    return out


def subset(s, tracks):
    """the scene with the given tracks only (supports re-packed)"""
    o = dict(s)
    rows = np.concatenate([np.arange(s["off"][n], s["off"][n + 1]) for n in tracks]) if len(tracks) else np.zeros(0, int)
    o["off"] = np.concatenate([[0], np.cumsum([s["off"][n + 1] - s["off"][n] for n in tracks])]).astype(np.int64)
    for key in ("img", "l2d", "l3d"):
        o[key] = s[key][rows]
    for key in ("line6", "gt6"):
        o[key] = s[key][list(tracks)]
    return o


def refine_cfg(**kw):
    """the configuration the tests run: the feature term with few samples and iterations"""
    cfg = dict(min_num_images=4, num_outliers_aggregate=2, use_geometric=True, geometric_alpha=10.0, use_vp=False,
               use_heatmap=False, use_feature=True, n_samples_feature=8, fconsis_multiplier=1.0, sample_range_min=0.05,
               sample_range_max=0.95, channels=128, dtype="float16")
    cfg.update(kw)
    rf = optimize.RefinementConfig(cfg)
    rf.max_num_iterations = int(kw.get("max_num_iterations", 20))
    return rf


def run(s, rf, form, src, host_threads=None, tracks=None, ctx=None, dtype=None, vp=None, heatmaps=None, grids=None):
    """optimize.refine_arrays over the scene's tracks (all, or the given indices, in the given order) -> its dict"""
    tracks = list(range(len(s["line6"]))) if tracks is None else list(tracks)
    sub = subset(s, tracks)
    keep = []
    cams = (s["img_ids"], s["k"], s["q"], s["t"])
    csr = (sub["line6"], sub["off"], sub["img"], sub["l2d"], sub["l3d"])
    kw = {}
    if rf.use_feature:
        kw["feature"] = rf._feature(dtype)
        if grids is not None:
            kw["grids"] = grids
        elif form == "patch":
            kw["grids"] = native_grids(s, tracks, form, src, keep)
        else:
            kw["featuremaps"] = src if isinstance(src, optimize.FeatureMaps) else optimize.FeatureMaps(src, dtype or rf.dtype,
                                                                                                      host_threads is not None)
    if vp is not None:
        rows = np.concatenate([np.arange(s["off"][n], s["off"][n + 1]) for n in tracks])
        kw["vp"] = (vp[0][rows], vp[1][rows])
    hw = np.tile(np.array(s.get("hw", (H, W)), np.int32), (len(s["img_ids"]), 1)) if rf.use_heatmap else None
    return optimize.refine_arrays(cams, csr, rf._struct(rf.num_outliers_aggregate), host_threads, ctx=ctx, terms=rf._terms(),
                                  view_hw=hw, heatmaps=heatmaps, **kw)


RESULT_KEYS = ("params", "segments", "cost", "iterations", "codes")


def same_bits(a, b, what=""):
    for k in RESULT_KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def eval_ours(s, n, rf, grids, p=None, dtype=None):
    """lt_fn_refine_eval_feature for track n -> dict(samples [(ref, coor, tgts)], r, failed, cost, g, H)"""
    L = _capi.load_library()
    ptr = _capi.ptr
    a, b = int(s["off"][n]), int(s["off"][n + 1])
    ids = sorted_ids(s, n)
    keep = []
    glist = []
    for i in ids:
        arr, R, tv = grids[i]
        arr = np.ascontiguousarray(arr)
        keep.append(arr)
        glist.append((arr.ctypes.data, arr.shape[0], arr.shape[1], np.asarray(R, float).reshape(4), np.asarray(tv, float).reshape(2), 0))
    garr, ng = optimize._grid_array(glist)
    terms = rf._terms()
    feat = rf._feature(dtype)
    cap_s, cap_b = feat.n_samples_feature, feat.n_samples_feature * max(len(ids) - 1, 1)
    nk, nb = np.zeros(1, np.int32), np.zeros(1, np.int32)
    ref = np.zeros(cap_s, np.int32); line = np.zeros((cap_s, 3)); ntgt = np.zeros(cap_s, np.int32)
    tgts = np.zeros(cap_b, np.int32); res = np.full((cap_b, 128), np.nan); failed = np.zeros(cap_b, np.int32)
    cost, g, Hm = np.zeros(1), np.zeros(4), np.zeros((4, 4))
    line6 = np.ascontiguousarray(s["line6"][n])
    img = np.ascontiguousarray(s["img"][a:b]); l2d = np.ascontiguousarray(s["l2d"][a:b])
    pp = None if p is None else np.ascontiguousarray(p, np.float64)
    d, i32 = C.c_double, C.c_int32
    rc = L.lt_fn_refine_eval_feature(len(s["img_ids"]), ptr(s["img_ids"], i32), ptr(s["k"], d), ptr(s["q"], d), ptr(s["t"], d),
                                     ptr(line6, d), b - a, ptr(img, i32), ptr(l2d, d), float(rf.geometric_alpha), C.byref(terms),
                                     C.byref(feat), ng, garr, None if pp is None else ptr(pp, d), cap_s, cap_b, ptr(nk, i32),
                                     ptr(ref, i32), ptr(line, d), ptr(ntgt, i32), ptr(tgts, i32), ptr(nb, i32), ptr(res, d),
                                     ptr(failed, i32), ptr(cost, d), ptr(g, d), ptr(Hm, d))
    if rc != 0:
        raise ValueError(L.lt_fn_refine_host_error().decode())
    smps, o = [], 0
    for j in range(int(nk[0])):
        smps.append((int(ref[j]), line[j].copy(), [int(x) for x in tgts[o:o + ntgt[j]]]))
        o += int(ntgt[j])
    return dict(samples=smps, r=res[:int(nb[0])], failed=failed[:int(nb[0])] != 0, cost=float(cost[0]), g=g, H=Hm)


def line_distance(seg6, gt6):
    """the larger distance of the segment's ends to the infinite ground-truth line"""
    d = (gt6[3:] - gt6[:3]) / np.linalg.norm(gt6[3:] - gt6[:3])
    return max(np.linalg.norm(np.cross(p - gt6[:3], d)) for p in (seg6[:3], seg6[3:]))


# ---- edge scenes of the sample selection and of the sampling ----
def projected_supports(s, n):
    """track n with one support per image: exactly the projection of its initial line (perpendicular distance 0)"""
    o = subset(s, [n])
    ids = sorted_ids(s, n)
    cams = cams_of(s)
    l2d = np.array([np.concatenate([po.project(cams[i], o["line6"][0, :3])[0], po.project(cams[i], o["line6"][0, 3:])[0]])
                    for i in ids])
    o["img"], o["l2d"], o["off"] = np.array(ids, np.int32), l2d, np.array([0, len(ids)], np.int64)
    o["l3d"] = np.tile(o["gt6"][0], (len(ids), 1))
    return o


def shifted(o, delta):
    """every support moved by delta pixels along its normal"""
    o = dict(o)
    l = o["l2d"].copy()
    for k in range(len(l)):
        d = l[k, 2:] - l[k, :2]
        nrm = np.array([-d[1], d[0]]) / np.linalg.norm(d)
        l[k, :2] += delta * nrm; l[k, 2:] += delta * nrm
    o["l2d"] = l
    return o


def trimmed(o, spans):
    """support k cut to the part [spans[k][0], spans[k][1]] of itself"""
    o = dict(o)
    l = o["l2d"].copy()
    for k, (lo, hi) in enumerate(spans):
        s, e = o["l2d"][k, :2], o["l2d"][k, 2:]
        l[k, :2], l[k, 2:] = s + lo * (e - s), s + hi * (e - s)
    o["l2d"] = l
    return o


def _ulps(x, n):
    """x and its n neighbours on either side"""
    up, dn = [x], [x]
    for _ in range(n):
        up.append(np.nextafter(up[-1], np.inf)); dn.append(np.nextafter(dn[-1], -np.inf))
    return dn[:0:-1] + up


def length_tie(o, a, b):
    """support b re-ended along its own direction so that its length is support a's to the bit; None if no end within
    80 ulps of either coordinate gives it"""
    o = dict(o)
    l = o["l2d"].copy()
    da = l[a, :2] - l[a, 2:]
    la = np.sqrt(da[0] * da[0] + da[1] * da[1])
    d = (l[b, 2:] - l[b, :2]) / np.linalg.norm(l[b, 2:] - l[b, :2])
    e = l[b, :2] + la * d
    xs, ys = np.array(_ulps(e[0], 80)), np.array(_ulps(e[1], 80))
    dx, dy = l[b, 0] - xs[:, None], l[b, 1] - ys[None, :]
    hit = np.argwhere(np.sqrt(dx * dx + dy * dy) == la)
    if len(hit) == 0:
        return None
    l[b, 2:] = [xs[hit[0][0]], ys[hit[0][1]]]
    o["l2d"] = l
    return o


def swapped(o, a, b):
    """supports a and b exchanged in the track's list"""
    o = dict(o)
    idx = np.arange(len(o["img"]))
    idx[[a, b]] = idx[[b, a]]
    for key in ("img", "l2d", "l3d"):
        o[key] = o[key][idx]
    return o


def failing_scene(n_samples=8):
    """a line along x seen by four unrotated cameras on the x axis: the projection is the row y = cy in every image.  The
    first image's support is a short vertical segment -- the longest good support of the one point the others' tiny
    horizontal supports cover -- so the sample line is parallel to the projection and the reference intersection has
    p_homo[2] = 0 at the initial line"""
    ids = np.array([3, 5, 6, 9], np.int32)
    k = np.tile([64.0, 64.0, 32.0, 24.0], (4, 1))
    q = np.tile([1.0, 0.0, 0.0, 0.0], (4, 1))
    t = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [-0.25, 0.0, 0.0], [0.5, 0.0, 0.0]])
    cam11 = np.concatenate([k, q, t], 1)
    line6 = np.array([[-1.0, 0.0, 4.0, 1.0, 0.0, 4.0]])
    point = line6[0, :3] + 3.0 * ((line6[0, 3:] - line6[0, :3]) / (n_samples - 1))
    l2d = []
    for n in range(4):
        x, y = po.project(cam11[n], point)[0]
        l2d.append([x, 24.0 - 0.25, x, 24.0 + 0.25] if n == 0 else [x - 0.2, 24.0, x + 0.2, 24.0])
    maps = {int(i): np.zeros((8, 8, CH)) for i in ids}
    return dict(img_ids=ids, k=k, q=q, t=t, cam11=cam11, maps=maps, line6=line6, gt6=line6.copy(), off=np.array([0, 4], np.int64),
                img=ids.copy(), l2d=np.array(l2d), l3d=np.tile(line6, (4, 1)))


def merge(*scenes):
    """the tracks of scenes that share their cameras and maps, one after the other"""
    o = dict(scenes[0])
    for key in ("img", "l2d", "l3d", "line6", "gt6"):
        o[key] = np.concatenate([s[key] for s in scenes])
    o["off"] = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(s["off"]) for s in scenes]))]).astype(np.int64)
    return o


def some_vps(s, seed=0):
    """a vanishing point for two supports in three (any finite homogeneous point serves the bit comparison)"""
    rng = np.random.default_rng(seed)
    M = len(s["img"])
    return (np.arange(M) % 3 != 0).astype(np.int32), np.concatenate([rng.uniform(-200, 200, (M, 2)), np.ones((M, 1))], 1)


def some_heatmaps(s):
    """one (48, 64) heatmap per image: a channel of its feature map moved into [0, 1]"""
    return {i: 0.5 + 0.5 * m[:, :, 0] for i, m in s["maps"].items()}
