"""Times the geometric line refinement (limap_amd.optimize) on two track sets: the tracks this
package triangulates from the 100 views x 500 segments scene, and a set of the size BASELINE config 3 leaves (1000
views; 30 000 synthetic tracks of 4..40 supports).  Device: warm process, median of repeated calls of lt_refine_arrays
with the stages of lt_refine_get_timers (host ms of validation + tables + upload, kernels, download; device ms of
k_refine_lm by HIP events).  Host: lt_fn_refine_host on 16 threads, checked to give the same bits.  There is no Ceres to
time against: the figures are a record.  Writes profiles/refine_timing.json.

usage: python tools/time_refine.py [--repeat 5] [--out profiles/refine_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene_tracks():
    from limap_amd import merging, synthetic as syn, triangulation as tri
    sc = syn.make_scene(n_views=100, n_segs=500, n_neighbors=20, seed=0)
    T = tri.GlobalLineTriangulator(syn.default_triangulation_cfg())
    T.SetRanges(sc.ranges)
    T.InitArrays(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, [sc.segs_of(i) for i in range(sc.n_images)])
    for i in sc.img_ids:
        T.TriangulateImage(int(i), sc.matches_of(int(i)))
    T.ComputeLineTracks()
    a = merging.TrackSet.from_triangulator(T).arrays()
    cams = (sc.img_ids.astype(np.int32), np.ascontiguousarray(sc.kvec), np.ascontiguousarray(sc.qvec),
            np.ascontiguousarray(sc.tvec))
    csr = (np.ascontiguousarray(a["line"][:, :6]), a["off"], np.ascontiguousarray(a["image_ids"]),
           np.ascontiguousarray(a["line2d"]), np.ascontiguousarray(a["line3d"][:, :6]))
    return cams, csr


def synthetic_tracks(n_tracks=30000, n_views=1000, seed=3):
    from limap_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    sc = syn.make_scene(n_views=n_views, n_segs=4, n_neighbors=2, n_rooms=4, seed=seed)
    R = np.array([syn.quat_to_rot(q) for q in sc.qvec])
    line6, off, img, l2, l3 = [], [0], [], [], []
    while len(line6) < n_tracks:
        a = rng.uniform([1.0, 1.0, 0.3], [39.0, 7.0, 2.7])
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        b = a + d * rng.uniform(0.5, 2.0)
        X = np.stack([a, b])
        cam = np.einsum("vij,pj->vpi", R, X) + sc.tvec[:, None, :]
        ok = np.flatnonzero((cam[:, :, 2] > 0.3).all(1))
        if len(ok) < 4:
            continue
        ok = rng.permutation(ok)[:int(rng.integers(4, 41))]
        c = cam[ok]
        xy = np.stack([sc.kvec[ok, None, 0] * c[:, :, 0] / c[:, :, 2] + sc.kvec[ok, None, 2],
                       sc.kvec[ok, None, 1] * c[:, :, 1] / c[:, :, 2] + sc.kvec[ok, None, 3]], 2).reshape(-1, 4)
        good = (np.abs(xy).max(1) < 3000) & (np.linalg.norm(xy[:, :2] - xy[:, 2:], axis=1) > 5)
        if good.sum() < 4:
            continue
        ok, xy = ok[good], xy[good]
        line6.append(np.concatenate([a, b]) + rng.normal(0, 0.02, 6))
        img.append(sc.img_ids[ok]); l2.append(xy + rng.normal(0, 0.5, xy.shape))
        l3.append(np.tile(np.concatenate([a, b]), (len(ok), 1)) + rng.normal(0, 0.01, (len(ok), 6)))
        off.append(off[-1] + len(ok))
    cams = (sc.img_ids.astype(np.int32), np.ascontiguousarray(sc.kvec), np.ascontiguousarray(sc.qvec),
            np.ascontiguousarray(sc.tvec))
    csr = (np.array(line6), np.array(off, np.int64), np.concatenate(img).astype(np.int32), np.concatenate(l2),
           np.concatenate(l3))
    return cams, csr


def measure(name, cams, csr, repeat):
    from limap_amd import _capi, optimize
    cfg = optimize.HybridBAConfig(dict(constant_intrinsics=True, constant_pose=True))
    cfg.max_num_iterations = 200
    c = cfg._struct(2)
    ctx = _capi.Context()
    optimize.refine_arrays(cams, csr, c, ctx=ctx)  # warm: code object, buffers
    rows = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = optimize.refine_arrays(cams, csr, c, ctx=ctx)
        tm = r["timers"]
        rows.append([1e3 * (time.perf_counter() - t0), tm["prepare_ms"], tm["kernels_ms"], tm["download_ms"], tm["lm_device_ms"]])
    med = np.median(np.array(rows), 0).tolist()
    t0 = time.perf_counter()
    h = optimize.refine_arrays(cams, csr, c, host_threads=16)
    host_ms = 1e3 * (time.perf_counter() - t0)
    for k in ("params", "segments", "cost", "iterations", "codes"):
        assert np.array_equal(h[k], r[k]), f"host and device disagree on {k}"
    return dict(name=name, tracks=len(csr[1]) - 1, supports=int(csr[1][-1]), repeat=repeat,
                device=dict(call_ms=med[0], prepare_ms=med[1], kernels_ms=med[2], download_ms=med[3], k_refine_lm_ms=med[4]),
                host_16_threads_ms=host_ms, iterations_median=float(np.median(r["iterations"])),
                iterations_max=int(r["iterations"].max()), codes=np.bincount(r["codes"], minlength=6).tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_timing.json"))
    args = ap.parse_args()
    out = dict(method="warm process; median of `repeat` calls; stages from lt_refine_get_timers; host path timed once",
               runs=[measure("scene_100x500", *scene_tracks(), args.repeat),
                     measure("config3_sized", *synthetic_tracks(), args.repeat)])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
