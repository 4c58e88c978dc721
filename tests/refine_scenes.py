"""Scenes for the refinement tests: cameras from limap_amd.synthetic, GT 3D lines projected to 2D segments with Gaussian
endpoint noise, ragged support counts (above the kernel's group width of 16 too, and images that support a track twice),
a perturbed initial Line3d.  Everything as the CSR arrays lt_refine_arrays takes."""
import numpy as np

from limap_amd import synthetic as syn


def _project(k, q, t, p):
    x = syn.quat_to_rot(q) @ p + t
    return np.array([k[0] * x[0] / x[2] + k[2], k[1] * x[1] / x[2] + k[3]]), x[2]


def make_tracks(n_tracks=200, n_views=30, seed=0, noise_px=0.5, init_sigma=0.02, k_max=40, img_id_offset=0):
    rng = np.random.default_rng(seed)
    sc = syn.make_scene(n_views=n_views, n_segs=8, n_neighbors=4, seed=seed, img_id_offset=img_id_offset)
    ids, kv, qv, tv = sc.img_ids.astype(np.int32), sc.kvec, sc.qvec, sc.tvec
    line6, gt6, off, img, l2d, l3d = [], [], [0], [], [], []
    while len(line6) < n_tracks:
        a = rng.uniform([1.0, 1.0, 0.3], [9.0, 7.0, 2.7])
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        b = a + d * rng.uniform(0.5, 2.0)
        want = int(rng.integers(2, k_max + 1)) if rng.random() < 0.25 else int(rng.integers(4, 13))
        sup_img, sup_2d, sup_3d = [], [], []
        for v in rng.permutation(n_views):
            if len(sup_img) >= want:
                break
            reps = 2 if rng.random() < 0.1 else 1  # an image with two supports of the track
            for _ in range(reps):
                s0, s1 = np.sort(rng.uniform(0.0, 1.0, 2))
                if s1 - s0 < 0.2:
                    s0, s1 = 0.0, 1.0
                pa, pb = a + (b - a) * s0, a + (b - a) * s1
                (xa, za), (xb, zb) = _project(kv[v], qv[v], tv[v], pa), _project(kv[v], qv[v], tv[v], pb)
                if za < 0.3 or zb < 0.3 or np.abs(np.concatenate([xa, xb])).max() > 3000 or np.linalg.norm(xa - xb) < 5:
                    continue
                sup_img.append(int(ids[v]))
                sup_2d.append(np.concatenate([xa, xb]) + rng.normal(0, noise_px, 4))
                sup_3d.append(np.concatenate([pa, pb]) + rng.normal(0, 0.01, 6))
        if len(sup_img) < 2:
            continue
        gt6.append(np.concatenate([a, b]))
        line6.append(np.concatenate([a, b]) + rng.normal(0, init_sigma, 6))
        img += sup_img; l2d += sup_2d; l3d += sup_3d
        off.append(len(img))
    return dict(img_ids=ids, k=np.ascontiguousarray(kv), q=np.ascontiguousarray(qv), t=np.ascontiguousarray(tv),
                line6=np.array(line6), gt6=np.array(gt6), off=np.array(off, np.int64), img=np.array(img, np.int32),
                l2d=np.array(l2d), l3d=np.array(l3d))


def track_supports(s, n):
    """(cam11 (K, 11), segs4 (K, 4)) of track n in upstream's residual order"""
    a, b = int(s["off"][n]), int(s["off"][n + 1])
    order = np.argsort(s["img"][a:b], kind="stable") + a
    idx = {int(i): k for k, i in enumerate(s["img_ids"])}
    rows = [idx[int(i)] for i in s["img"][order]]
    cam = np.concatenate([s["k"][rows], s["q"][rows], s["t"][rows]], 1)
    return np.ascontiguousarray(cam), np.ascontiguousarray(s["l2d"][order])


def edge_tracks():
    """The edge fixtures: (name, cam11 (K, 11), segs4 (K, 4), params6).  A line through the origin (m = 0: the fallback
    basis, w1 = 0), supports parallel and perpendicular to the projection (cosine 1 and near 0), cosine clamped at 1, an
    image with two supports."""
    from refine_oracle import minimal
    out = []
    k = np.array([500.0, 480.0, 320.0, 240.0])
    q = np.array([1.0, 0.0, 0.0, 0.0])

    def cams(ts):
        return np.array([np.concatenate([k, q, t]) for t in ts])
    # through the origin along x, cameras looking down +z from z = -5 (t = (0, 0, 5)) and shifted
    p0 = minimal(np.array([-1.0, 0, 0, 1.0, 0, 0]))
    assert p0[5] == 0.0
    c = cams([[0, 0, 5.0], [0.3, -0.2, 5.0], [0, 0.5, 6.0]])
    par = np.array([[220.0, 240, 420, 240], [250.0, 220.8, 450, 220.8], [236.0, 280, 400, 280]])  # parallel: cosine 1
    out.append(("origin_parallel", c, par, p0))
    out.append(("origin_parallel_noisy", c, par + np.array([0, 0.4, 0, -0.3]), p0))
    perp = np.array([[320.0, 200, 320.0001, 290], [350.0, 180, 350.0, 260], [300.0, 250, 300.0, 320]])  # cosine near 0
    out.append(("origin_perpendicular", c, perp, p0))
    # parallel to the projection (y = 240 in the first camera) but beside it: the cosine is as close to the clamp as the
    # EPS terms let it come (1 - 5e-13), while the residuals, and so g and H, are not zero
    out.append(("clamped", c[:1].repeat(3, 0), np.array([[120.0, 240.75, 520, 240.75], [320.0, 239.5, 330, 239.5],
                                                          [100.0, 241.25, 611, 241.25]]), p0))
    # two supports from one image next to one from another
    p1 = minimal(np.array([0.5, 0.2, 1.0, 1.5, 0.4, 1.2]))
    c2 = cams([[0, 0, 5.0], [0, 0, 5.0], [0.4, 0.1, 4.0]])
    two = np.array([[360.0, 255, 400, 260], [400.0, 259, 440, 266], [420.0, 270, 470, 281]])
    out.append(("two_in_one_image", c2, two, p1))
    return out



EDGE_LINES = {"origin": np.array([-1.0, 0, 0, 1.0, 0, 0]), "two_in_one_image": np.array([0.5, 0.2, 1.0, 1.5, 0.4, 1.2])}


def edge_scene():
    """The edge fixtures as one scene of one-track-each for the whole step (prep, LM, cut): cameras de-duplicated into an
    image collection, line6 = the segment the fixture's parameters come from, line3d = that segment per support,
    shortened a little differently each."""
    cams, line6, off, img, l2d, l3d = [], [], [0], [], [], []
    for name, c, sg, _ in edge_tracks():
        seg = EDGE_LINES["two_in_one_image" if name == "two_in_one_image" else "origin"]
        line6.append(seg)
        for k in range(len(sg)):
            row = [i for i, x in enumerate(cams) if np.array_equal(x, c[k])]
            if not row:
                cams.append(c[k].copy())
                row = [len(cams) - 1]
            img.append(10 + 3 * row[0])
            l2d.append(sg[k])
            a, b = seg[:3], seg[3:]
            l3d.append(np.concatenate([a + (b - a) * 0.05 * k, b - (b - a) * 0.03 * k]))
        off.append(len(img))
    cams = np.array(cams)
    return dict(img_ids=(10 + 3 * np.arange(len(cams))).astype(np.int32), k=np.ascontiguousarray(cams[:, :4]),
                q=np.ascontiguousarray(cams[:, 4:8]), t=np.ascontiguousarray(cams[:, 8:]), line6=np.array(line6),
                off=np.array(off, np.int64), img=np.array(img, np.int32), l2d=np.array(l2d), l3d=np.array(l3d))
