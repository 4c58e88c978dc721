"""Shared helpers of the MergeToLineTracks tests: the golden files of tests/golden/make_merge_golden.py as the
arguments of limap_amd.merging.merging, and the track arrays to compare."""
import importlib.util
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge")
SCENES = ("a", "b", "c", "d")
STAGES = ("merge", "filter1", "remerge", "filter2")
REMERGE_L3 = dict(score_th=0.5, th_angle=5.0, th_overlap=0.001, th_smartoverlap=0.1, th_smartangle=1.0, th_perp=0.5,
                  th_innerseg=0.5)  # cfgs/fitnmerge/default.yaml:77-86
FILTER2D = (8.0, 5.0)


def load(name):
    with np.load(os.path.join(GOLDEN, f"merge_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def generator():
    path = os.path.join(os.path.dirname(GOLDEN), "make_merge_golden.py")
    spec = importlib.util.spec_from_file_location("make_merge_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def call_args(g):
    """(linker, all_2d_segs, imagecols, seg3d_list, neighbors, var2d) of a golden input set"""
    from limap_amd.base import ImageCollection
    ids = [int(i) for i in g["img_ids"]]
    so, no = g["seg_off"], g["nb_off"]
    all_2d = {i: g["segs2"][so[n]:so[n + 1]] for n, i in enumerate(ids)}
    seg3d = {i: g["segs3"][so[n]:so[n + 1]].reshape(-1, 2, 3) for n, i in enumerate(ids)}
    nbs = {i: [int(j) for j in g["nb"][no[n]:no[n + 1]]] for n, i in enumerate(ids)}
    imagecols = ImageCollection.from_arrays(ids, g["kvec"], g["qvec"], g["tvec"])
    return json.loads(str(g["linker"])), all_2d, imagecols, seg3d, nbs, float(g["var2d"])


def tracks_to_arrays(tracks):
    off = np.zeros(len(tracks) + 1, np.int64)
    off[1:] = np.cumsum([len(t.image_id_list) for t in tracks])
    cat = lambda xs, shape, dt: np.array(xs, dt).reshape(shape)  # noqa: E731
    return dict(
        line=cat([list(t.line.start) + list(t.line.end) + [t.line.uncertainty] for t in tracks], (-1, 7), float),
        off=off,
        image_ids=cat([i for t in tracks for i in t.image_id_list], (-1,), np.int32),
        line_ids=cat([i for t in tracks for i in t.line_id_list], (-1,), np.int32),
        node_ids=cat([i for t in tracks for i in t.node_id_list], (-1,), np.int32),
        scores=cat([s for t in tracks for s in t.score_list], (-1,), float),
        line2d=cat([list(l.start) + list(l.end) for t in tracks for l in t.line2d_list], (-1, 4), float),
        line3d=cat([list(l.start) + list(l.end) + list(l.depths) + [l.uncertainty, l.score] for t in tracks
                    for l in t.line3d_list], (-1, 10), float))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def assert_stage(a, g, stage):
    """track arrays `a` (TrackSet.arrays() form) against stage `stage` of golden set `g`"""
    p = stage + "_"
    assert len(a["off"]) == len(g[p + "off"]), f"{stage}: {len(a['off']) - 1} tracks, reference {len(g[p + 'off']) - 1}"
    assert np.array_equal(a["off"], g[p + "off"]), stage
    assert np.array_equal(a["image_ids"], g[p + "img"]), stage
    assert np.array_equal(a["line_ids"], g[p + "lid"]), stage
    assert np.array_equal(a["node_ids"], g[p + "nid"]), stage
    assert np.array_equal(bits(a["scores"]), bits(g[p + "score"])), stage
    assert np.array_equal(bits(a["line2d"]), bits(g[p + "line2d"])), stage
    assert np.array_equal(bits(a["line3d"]), bits(g[p + "line3d"])), stage
    ref = g[p + "line"]
    got = a["line"][:len(ref)]
    # track lines: within 1e-9 relative, start and end not swapped
    tol = 1e-9 * np.maximum(1.0, np.abs(ref[:, :6]))
    assert np.all(np.abs(got[:, :6] - ref[:, :6]) <= tol), stage
    assert np.array_equal(bits(got[:, 6]), bits(ref[:, 6])), stage


# ---- the CPU oracle's merge (oracle/lt_oracle.cpp ora_merge_to_tracks) and the scenes it checks the device on ----

def oracle_chain(mod, g):
    """the oracle (or, with mod = the reference module, the reference) on an input set `g` (golden / pack() form): the
    merge, then the fit-and-merge runner's filter, remerge, filter (num_outliers 0); a dict in the golden files' form"""
    T = mod.OracleTriangulator()
    T.Init(g["img_ids"], g["kvec"], g["qvec"], g["tvec"], g["seg_off"], g["segs2"])
    ts = T.MergeToLineTracks(g["seg_off"], g["segs3"], g["nb_off"], g["nb"], json.loads(str(g["linker"])),
                             float(g["var2d"]))
    out = dict(ts.graph())
    stages = [ts.get()]
    ts.filter_by_reprojection(*FILTER2D, 0)
    stages.append(ts.get())
    ts.remerge(REMERGE_L3, 0)
    stages.append(ts.get())
    ts.filter_by_reprojection(*FILTER2D, 0)
    stages.append(ts.get())
    for name, a in zip(STAGES, stages):
        out.update(golden_form(a, name))
    lab = -np.ones(len(out["node_img"]), np.int32)
    m = stages[0]
    for t in range(len(m["off"]) - 1):
        lab[m["node_ids"][m["off"][t]:m["off"][t + 1]]] = t
    out["labels"] = lab
    return out


def golden_form(a, stage):
    """track arrays (TrackSet.arrays() / OracleTrackSet.get() form) under the keys of a golden file's stage"""
    p = stage + "_"
    return {p + "off": a["off"], p + "img": a["image_ids"], p + "lid": a["line_ids"], p + "nid": a["node_ids"],
            p + "score": a["scores"], p + "line2d": a["line2d"], p + "line3d": a["line3d"], p + "line": a["line"]}


def _pack(ids, kvec, qvec, tvec, segs2, segs3, nbs, linker, var2d=5.0):
    """an input set from per-image lists (any id order): pack() of make_merge_golden.py"""
    inp = dict(ids=[int(i) for i in ids], kvec=np.asarray(kvec, float), qvec=np.asarray(qvec, float),
               tvec=np.asarray(tvec, float), segs2={int(i): np.asarray(s, float).reshape(-1, 4) for i, s in zip(ids, segs2)},
               segs3={int(i): np.asarray(s, float).reshape(-1, 6) for i, s in zip(ids, segs3)},
               neighbors={int(i): [int(j) for j in nb] for i, nb in zip(ids, nbs)}, linker=linker, var2d=var2d)
    return generator().pack(inp)


def remap_ids(g, new_ids):
    """input set `g` with image id g["img_ids"][n] renamed new_ids[n] (in the images and the neighbour lists)"""
    old = [int(i) for i in g["img_ids"]]
    m = dict(zip(old, [int(i) for i in new_ids]))
    so, no = g["seg_off"], g["nb_off"]
    return _pack([m[i] for i in old], g["kvec"], g["qvec"], g["tvec"],
                 [g["segs2"][so[n]:so[n + 1]] for n in range(len(old))],
                 [g["segs3"][so[n]:so[n + 1]] for n in range(len(old))],
                 [[m[int(j)] for j in g["nb"][no[n]:no[n + 1]]] for n in range(len(old))],
                 json.loads(str(g["linker"])), float(g["var2d"]))


L2_KEYS = ("score_th", "th_angle", "th_overlap", "th_smartoverlap", "th_smartangle", "th_perp", "th_innerseg")
USE2 = ("use_angle", "use_overlap", "use_smartangle", "use_perp", "use_innerseg")


def random_linker(rng):
    """every threshold and use_* flag of the 2D linker, every threshold of the 3D one (its use_* flags are forced by
    set_to_spatial_merging), around the fit-and-merge defaults"""
    l2 = dict(score_th=float(rng.choice([0.3, 0.5, 0.7])), th_angle=float(rng.uniform(3.0, 15.0)),
              th_overlap=float(rng.uniform(0.0, 0.15)), th_smartoverlap=float(rng.uniform(0.15, 0.4)),
              th_smartangle=float(rng.uniform(0.5, 3.0)), th_perp=float(rng.uniform(2.0, 10.0)),
              th_innerseg=float(rng.uniform(2.0, 10.0)))
    l2.update({k: bool(rng.integers(0, 2)) for k in USE2})
    l3 = dict(score_th=float(rng.choice([0.3, 0.5, 0.7])), th_angle=float(rng.uniform(4.0, 15.0)),
              th_overlap=float(rng.uniform(0.0, 0.05)), th_smartoverlap=float(rng.uniform(0.05, 0.3)),
              th_smartangle=float(rng.uniform(0.5, 3.0)), th_perp=float(rng.uniform(0.5, 3.0)),
              th_innerseg=float(rng.uniform(0.5, 3.0)), th_scaleinv=float(rng.uniform(0.005, 0.05)))
    return dict(linker2d=l2, linker3d=l3)


def random_scene(seed):
    """random size, neighbour count, failed fits, depth noise and linkers (drawn as in tests/test_gpu_fuzz.py)"""
    from limap_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    nv, ns = int(rng.integers(3, 9)), int(rng.integers(20, 140))
    nn = int(rng.integers(1, nv))
    sc = syn.make_scene(n_views=nv, n_segs=ns, n_neighbors=nn, seed=seed)
    fit = syn.make_fit_segs(sc, seed=seed, fail_frac=float(rng.uniform(0.0, 0.3)),
                            depth_noise=float(rng.choice([0.0, 0.0005, 0.002])))
    gen = generator()
    return gen.pack(gen.scene_inputs(sc, fit, random_linker(rng), var2d=float(rng.choice([2.0, 5.0]))))


def shaped_scene(counts, seed, zero_image=None, empty_neighbour=False):
    """images with exactly counts[n] lines, every image the neighbour of every other.  The lines of an image are drawn
    (with replacement, jittered) from the fitted lines of a synthetic view, so lines at every index -- past every row
    tile and LDS chunk -- have many partners.  A fraction are zeros (failed fits); image `zero_image` has only zeros.
    empty_neighbour: one more image without lines, the only neighbour of one more image."""
    from limap_amd import synthetic as syn
    nv = len(counts) + (2 if empty_neighbour else 0)
    sc = syn.make_scene(n_views=nv, n_segs=120, n_neighbors=nv - 1, seed=seed)
    fit = syn.make_fit_segs(sc, seed=seed, fail_frac=0.0, depth_noise=0.0005)
    rng = np.random.default_rng([seed, 77])
    ids = [int(i) for i in sc.img_ids]
    segs2, segs3 = [], []
    for n, c in enumerate(counts):
        s2, s3 = sc.segs_of(n), fit[ids[n]].reshape(-1, 6)
        real = np.nonzero(np.any(s3 != 0, axis=1))[0]
        pick = rng.choice(real, size=c)
        a2 = s2[pick] + rng.normal(0, 0.3, (c, 4))
        a3 = s3[pick] * (1.0 + rng.normal(0, 2e-4, (c, 1)))
        a3[rng.uniform(size=c) < 0.05] = 0.0
        if n == zero_image:
            a3[:] = 0.0
        segs2.append(a2)
        segs3.append(a3)
    nbs = [[j for j in ids[:len(counts)] if j != i] for i in ids[:len(counts)]]
    if empty_neighbour:
        n = len(counts)
        s2, s3 = sc.segs_of(n), fit[ids[n]].reshape(-1, 6)
        segs2 += [s2, np.zeros((0, 4))]
        segs3 += [s3, np.zeros((0, 6))]
        nbs += [[ids[n + 1]], [ids[0]]]
    linker = dict(linker2d=dict(syn.default_merging_cfg()["linker2d"]), linker3d=dict(syn.default_merging_cfg()["linker3d"]))
    return _pack(ids, sc.kvec, sc.qvec, sc.tvec, segs2, segs3, nbs, linker)


def _two_cameras(z2=-6.0):
    """image 0 looks down +z from (0, 0, -5); image 1 from (0.5, 0.2, z2), both with the identity rotation"""
    k = np.array([[500.0, 500.0, 400.0, 300.0]] * 2)
    q = np.array([[1.0, 0, 0, 0]] * 2)
    t = np.array([[0.0, 0.0, 5.0], [-0.5, -0.2, -z2]])
    return k, q, t


def _project(k, q, t, seg3):
    """2D segments of 3D segments (M, 6) in one pinhole view with the identity rotation (q is unused)"""
    p = seg3.reshape(-1, 3) + t
    z = np.where(np.abs(p[:, 2]) > 1e-9, p[:, 2], 1e-9)
    return np.stack([k[0] * p[:, 0] / z + k[2], k[1] * p[:, 1] / z + k[3]], 1).reshape(-1, 4)


PERMISSIVE_L2 = dict(use_angle=False, use_overlap=False, use_smartangle=False, use_perp=False, use_innerseg=False)


def pair_angles(th_angle, deltas=(1e-9, 1e-7, 1e-5)):
    """the 3D angles (deg) of the pairs of angle_scene, pair n = lines 2n, 2n + 1 of image 0"""
    g = th_angle * (1 + 1e-6) + 1e-6
    if th_angle == 0:
        return [0.0, 0.0, 1e-12, 1e-9, 1e-7, 1e-5, 1e-3]
    return [a * (1 + s * d) for a in (th_angle, g) for d in deltas for s in (-1, 1)]


def angle_scene(th_angle, deltas=(1e-9, 1e-7, 1e-5)):
    """pairs of segments through a common midpoint at 3D angles th_angle (1 +- delta), at the guard's own cut
    g = th_angle (1 + 1e-6) + 1e-6 deg times (1 +- delta), and (th_angle 0) exactly parallel; each pair 50 units from
    the next so that pairs do not link.  Image 0 holds both lines of every pair (self pass), image 1 their second lines
    (cross pass).  The 2D linker accepts everything, the 3D one tests the angle, the overlap and the inner segment."""
    angles = pair_angles(th_angle, deltas)
    l1, l2 = [], []
    for n, a in enumerate(angles):
        c = np.array([50.0 * n, 0.3, 2.0])
        r = np.deg2rad(a)
        u = np.array([0.0, 1.0, 0.0]) if n % 2 else np.array([1.0, 0.0, 0.0])
        v = np.array([np.cos(r), np.sin(r), 0.0]) if n % 2 == 0 else np.array([-np.sin(r), np.cos(r), 0.0])
        l1.append(np.concatenate([c - 0.8 * u, c + 0.8 * u]))
        l2.append(np.concatenate([c - 0.6 * v, c + 0.6 * v]))
    s0 = np.array([x for pair in zip(l1, l2) for x in pair])
    s1 = np.array(l2[::-1])
    k, q, t = _two_cameras()
    linker = dict(linker2d=PERMISSIVE_L2,
                  linker3d=dict(th_angle=float(th_angle), th_overlap=0.0, use_smartangle=False, th_innerseg=50.0))
    return _pack([0, 1], k, q, t, [_project(k[0], q[0], t[0], s0), _project(k[1], q[1], t[1], s1)], [s0, s1],
                 [[1], [0]], linker, var2d=5.0)


def degenerate_scene(permissive):
    """identical and exactly parallel lines in one image and across images, lines of equal length (tied sims), very
    short lines, endpoints at depth 0 and behind the neighbour camera"""
    base = np.array([0.0, 0.0, 1.0, 1.0, 0.0, 1.0])
    par = base + np.array([0.0, 0.01, 0.0, 0.0, 0.01, 0.0])
    same_len = np.array([0.0, 0.02, 1.0, 1.0, 0.02, 1.0])  # (length 1, parallel, 2 cm away)
    short = np.array([0.2, 0.0, 1.0, 0.2 + 1e-9, 1e-9, 1.0])
    short2 = np.array([0.3, 0.0, 1.0, 0.3 + 1e-6, 0.0, 1.0])
    # image 1's camera (_two_cameras(z2=-1)): the depth of a point there is z + 1
    at_plane = np.array([0.0, -0.1, -1.0, 0.8, -0.1, 1.5])   # start on image 1's image plane (depth 0)
    behind = np.array([0.1, -0.2, -1.6, 0.7, -0.2, 1.4])     # start behind image 1's camera
    at_plane2 = at_plane + np.array([0.02, 0, 0, 0.02, 0, 0])
    behind2 = behind + np.array([0.0, 0.01, 0, 0.0, 0.01, 0])
    s0 = np.array([base, base, par, same_len, short, short2, at_plane, behind, base])
    s1 = np.array([base, same_len, par, at_plane2, behind2, short2, base[[3, 4, 5, 0, 1, 2]]])
    s2 = np.array([par, par, base, same_len])
    k, q, t = _two_cameras(z2=-1.0)
    k, q, t = np.vstack([k, [450.0, 460.0, 390.0, 310.0]]), np.vstack([q, [1.0, 0, 0, 0]]), np.vstack([t, [0.1, 0, 4.0]])
    segs3 = [s0, s1, s2]
    segs2 = [_project(k[n], q[n], t[n], s) for n, s in enumerate(segs3)]
    for s in segs2:
        np.nan_to_num(s, copy=False, posinf=1e6, neginf=-1e6)
    l2 = dict(PERMISSIVE_L2) if permissive else dict(th_angle=5.0, th_perp=2.0, th_overlap=0.05)
    linker = dict(linker2d=l2, linker3d=dict(th_angle=8.0, th_innerseg=0.75, th_perp=0.75))
    return _pack([0, 1, 2], k, q, t, segs2, segs3, [[1, 2], [0, 2, 1], [0]], linker, var2d=5.0)


INT_MAX = 2 ** 31 - 1
# image ids of id_scene: ordinary, up to 65535, negative, above 2^29 (generic parity rule), near INT_MAX (the int key
# wraps).  The reference is defined for ids in [0, 65535] only: MergeToLineTracks keeps its pairs as Node2d =
# pair<uint16_t, uint16_t> (util/types.h:16, merging.cc:385), so another id is truncated and indexes all_lengths_3d
# out of range.  The oracle and the device keep the full id and evaluate the key rule as written.
REF_ID_SETS = ("plain", "wide")
ID_SETS = {
    "plain": [0, 1, 2, 3],
    "wide": [3, 4000, 65000, 65535],
    "negative": [-7, -3, 0, 5],
    "large": [2 ** 29 + 1, 2 ** 29 + 8, 2 ** 30 + 3, 2 ** 30 + 4],
    "intmax": [INT_MAX - 3, INT_MAX - 2, INT_MAX - 1, INT_MAX],
    "extremes": [-2 ** 31, -5, 2 ** 30, INT_MAX],
}


def id_scene(kind, self_listed=False, counts=(40, 65, 30, 50), seed=31):
    """shaped_scene(counts) with the image ids ID_SETS[kind]; self_listed: every image is also its own neighbour"""
    g = remap_ids(shaped_scene(counts, seed), ID_SETS[kind])
    if not self_listed:
        return g
    ids = [int(i) for i in g["img_ids"]]
    so, no = g["seg_off"], g["nb_off"]
    return _pack(ids, g["kvec"], g["qvec"], g["tvec"], [g["segs2"][so[n]:so[n + 1]] for n in range(len(ids))],
                 [g["segs3"][so[n]:so[n + 1]] for n in range(len(ids))],
                 [[i] + [int(j) for j in g["nb"][no[n]:no[n + 1]]] for n, i in enumerate(ids)],
                 json.loads(str(g["linker"])), float(g["var2d"]))


ANGLES = (0.0, 0.5, 8.0, 45.0, 89.99, 90.0, 120.0)


def edge_scenes(ref_defined=False):
    """{name: builder} of the edge-case scenes at a size the CPU oracle and the reference run in about a second;
    ref_defined: only those with ids the reference is defined for (REF_ID_SETS)"""
    out = {f"angle_{a:g}": (lambda a=a: angle_scene(a)) for a in ANGLES}
    out["degenerate_permissive"] = lambda: degenerate_scene(True)
    out["degenerate_default"] = lambda: degenerate_scene(False)
    out.update({f"ids_{k}": (lambda k=k: id_scene(k)) for k in ID_SETS if not ref_defined or k in REF_ID_SETS})
    out["ids_wide_self"] = lambda: id_scene("wide", self_listed=True)
    if not ref_defined:
        out["ids_intmax_self"] = lambda: id_scene("intmax", self_listed=True)
        out["ids_large_self"] = lambda: id_scene("large", self_listed=True)
    out["shape_small"] = lambda: shaped_scene((1, 63, 64, 65), 41)
    out["zero_image_and_empty_neighbour"] = lambda: shaped_scene((30, 40, 20), 42, zero_image=1, empty_neighbour=True)
    return out
