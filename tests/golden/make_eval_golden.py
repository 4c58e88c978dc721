"""Golden files of limap.evaluation (PointCloudEvaluator, RefLineEvaluator), written by THE REFERENCE'S OWN CODE:
eval_ref_driver.cpp (next to this file) is compiled into a temporary directory together with the reference's
evaluation/base_evaluator.cc, point_cloud_evaluator.cc and refline_evaluator.cc, read where they lie, against the
objects `make -C oracle ref` builds (oracle/_ref/obj/**/*.o: kd_tree.o, linebase.o) and the stand-in headers of
oracle/ref_shim, and called through ctypes.  Run where the reference sources exist, like make_merge_golden.py;
tests/test_eval_host.py and tests/test_gpu_eval.py read the outputs.

  (all under tests/golden/eval/)
  eval_<name>.npz     inputs (points, lines, reference lines, thresholds, query points) and every method's outputs
  eval_ref_time.json  the reference's wall times on 10^6 points x 5 000 lines and its thread count

The generator asserts that the kd-tree's nearest distance equals the brute-force minimum (tests/eval_oracle.py) for
every sample the fixtures use: the contract is the exact minimum.

usage: python tests/golden/make_eval_golden.py [--no-timing] [--timing-only]
"""
import ctypes as C
import json
import os
import subprocess
import sys
import sysconfig
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "eval")
REF_SRC = "/root/reference/src"

import eval_oracle as eo  # noqa: E402

N_SAMPLES = (1000, 37)  # the bindings' default and a small odd count
DIST_LINE_N = (1000, 3)


def build_driver(tmp):
    objs = []
    for root, _, names in os.walk(os.path.join(ROOT, "oracle", "_ref", "obj")):
        objs += [os.path.join(root, n) for n in names if n.endswith(".o") and n != "ref_driver.o"]
    if not any(o.endswith("kd_tree.o") for o in objs):
        raise SystemExit("oracle/_ref/obj has no kd_tree.o: run `make -C oracle ref` first")
    import pybind11
    srcs = [os.path.join(REF_SRC, "limap", "evaluation", f)
            for f in ("base_evaluator.cc", "point_cloud_evaluator.cc", "refline_evaluator.cc")]
    out = os.path.join(tmp, "libeval_ref.so")
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-w", "-shared",
           "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + REF_SRC, "-I" + pybind11.get_include(),
           "-I" + sysconfig.get_paths()["include"], "-I" + os.path.join(ROOT, "oracle"),
           os.path.join(HERE, "eval_ref_driver.cpp")] + srcs + sorted(objs) + ["-o", out]
    subprocess.run(cmd, check=True)
    L = C.CDLL(out)
    dp, vp, i64 = C.POINTER(C.c_double), C.c_void_p, C.c_int64
    L.ev_pcd_create.restype = vp
    L.ev_pcd_create.argtypes = [dp, i64]
    L.ev_pcd_free.argtypes = [vp]
    L.ev_dist_points.argtypes = [vp, dp, i64, dp]
    L.ev_dist_line.restype = C.c_double
    L.ev_dist_line.argtypes = [vp, dp, C.c_int]
    L.ev_inlier_ratio.restype = C.c_double
    L.ev_inlier_ratio.argtypes = [vp, dp, C.c_double, C.c_int]
    L.ev_segs.restype = i64
    L.ev_segs.argtypes = [vp, dp, i64, C.c_double, C.c_int, C.c_int, dp, i64]
    L.ev_dists_each.restype = C.c_double
    L.ev_dists_each.argtypes = [vp, dp, i64, dp]
    L.ev_refline.restype = C.c_double
    L.ev_refline.argtypes = [dp, i64, dp, i64, C.c_double, C.c_int, C.c_int]
    L.ev_threads.restype = C.c_int
    L.ev_set_threads.argtypes = [C.c_int]
    L.ev_time_scene.argtypes = [dp, i64, dp, i64, dp, C.c_int, dp]
    return L


def P(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def f64(a):
    return np.ascontiguousarray(a, np.float64)


def run_reference(L, sc):
    pts, lines, refl = f64(sc["points"]), f64(sc["lines"]).reshape(-1, 6), f64(sc["ref_lines"]).reshape(-1, 6)
    th, qp = f64(sc["thresholds"]), f64(sc["query_points"]).reshape(-1, 3)
    Ln, R = lines.shape[0], refl.shape[0]
    lbuf = lines if Ln else np.zeros(6)
    rbuf = refl if R else np.zeros(6)
    h = L.ev_pcd_create(P(pts), pts.shape[0])
    out = {}
    # the contract: the kd-tree's nearest distance is the exact minimum, for every sample used below
    qs = [qp] + [eo.samples_center(lines, n).reshape(-1, 3) for n in N_SAMPLES] + \
         [eo.samples_ends(lines, n).reshape(-1, 3) for n in DIST_LINE_N]
    allq = f64(np.concatenate(qs, 0))
    kd = np.zeros(allq.shape[0])
    if allq.shape[0]:
        L.ev_dist_points(h, P(allq), allq.shape[0], P(kd))
    bf = eo.nearest_dists(pts, allq)
    assert np.array_equal(kd, bf), f"{sc['name']}: kd-tree nearest distance differs from the brute-force minimum " \
        f"on {int((kd != bf).sum())} samples: change the scene"
    out["dist_points"] = kd[:qp.shape[0]].copy()
    for n in DIST_LINE_N:
        out[f"dist_line_{n}"] = np.array([L.ev_dist_line(h, P(f64(lines[k])), n) for k in range(Ln)])
    for n in N_SAMPLES:
        out[f"ratios_{n}"] = np.array([[L.ev_inlier_ratio(h, P(f64(lines[k])), float(t), n) for t in th]
                                      for k in range(Ln)]).reshape(Ln, th.size)
    # Compute{In,Out}lierSegsOneLine write a std::vector<bool> from an `omp parallel for`: threads race on the bits of
    # one word and lose flags.  The segments are recorded on one thread, the race-free answer.
    threads = L.ev_threads()
    L.ev_set_threads(1)
    for t_i in sc["seg_th_idx"]:
        for inl in (1, 0):
            for n in N_SAMPLES:
                cnt = L.ev_segs(h, P(lbuf), Ln, float(th[t_i]), n, inl, P(np.zeros(6)), 0)
                buf = np.zeros((max(cnt, 1), 6))
                L.ev_segs(h, P(lbuf), Ln, float(th[t_i]), n, inl, P(buf), cnt)
                out[f"{'in' if inl else 'out'}segs_{t_i}_{n}"] = buf[:cnt]
    L.ev_set_threads(threads)
    d = np.zeros(pts.shape[0])
    L.ev_dists_each(h, P(lbuf), Ln, P(d))
    out["dists_each"] = d
    L.ev_pcd_free(h)
    for n in N_SAMPLES:
        out[f"recall_ref_{n}"] = np.array([L.ev_refline(P(rbuf), R, P(lbuf), Ln, float(t), n, 0) for t in th])
        out[f"recall_tested_{n}"] = np.array([L.ev_refline(P(rbuf), R, P(lbuf), Ln, float(t), n, 1) for t in th])
    out["sum_length"] = np.array(L.ev_refline(P(rbuf), R, P(lbuf), Ln, 0.0, 2, 2))
    return out


def rand_lines(rng, n, lo, hi, max_len):
    s = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([s, s + d * rng.uniform(0.01, max_len, (n, 1))], 1)


def exact_thresholds(points, lines, n, picks):
    """thresholds set exactly to sampled distances: they pin <= (ratios) against < (recall)"""
    d = eo.nearest_dists(points, eo.samples_center(lines, n).reshape(-1, 3))
    return [float(d[i]) for i in picks]


def scenes():
    rng = np.random.default_rng(20261015)
    out = []
    # (a) random cloud in the unit cube, lines in and around it, reference lines = perturbed tested lines
    pts = rng.uniform(0, 1, (3000, 3))
    lines = rand_lines(rng, 36, -0.2, 1.2, 0.6)
    refl = np.concatenate([lines[:20] + rng.normal(scale=0.01, size=(20, 6)), rand_lines(rng, 8, 0, 1, 0.5)], 0)
    th = [0.001, 0.005, 0.01, 0.05, 0.1] + exact_thresholds(pts, lines, 1000, [5, 12345, 30001])
    out.append(dict(name="random", points=pts, lines=lines, ref_lines=refl, thresholds=np.array(th),
                    query_points=rng.uniform(-0.5, 1.5, (500, 3)), seg_th_idx=[2, 5]))
    # (b) edges: a coplanar cloud (z = 0) with duplicate points, zero-length lines and reference lines, a line lying
    # on cloud points, a collinear run of points
    g = np.stack(np.meshgrid(np.linspace(0, 1, 21), np.linspace(0, 1, 21)), -1).reshape(-1, 2)
    pts = np.concatenate([g, np.zeros((g.shape[0], 1))], 1)
    pts = np.concatenate([pts, pts[::7], np.stack([np.linspace(0, 1, 50), np.full(50, 0.5), np.full(50, 0.3)], 1)], 0)
    lines = np.concatenate([rand_lines(rng, 12, -0.1, 1.1, 0.8),
                            np.array([[0.5, 0.5, 0.0, 0.5, 0.5, 0.0], [0.2, 0.3, 0.1, 0.2, 0.3, 0.1],
                                      [0.0, 0.0, 0.0, 1.0, 0.0, 0.0], [0.0, 0.5, 0.3, 1.0, 0.5, 0.3],
                                      [0.25, 0.25, 0.02, 0.75, 0.75, 0.02]])], 0)
    refl = np.concatenate([lines[12:] + 0.0, np.array([[0.3, 0.3, 0.0, 0.3, 0.3, 0.0]]),
                           rand_lines(rng, 5, 0, 1, 0.4)], 0)
    th = [0.0, 0.001, 0.01, 0.02, 0.05] + exact_thresholds(pts, lines, 1000, [100, 7000, 15500])
    out.append(dict(name="edges", points=pts, lines=lines, ref_lines=refl, thresholds=np.array(th),
                    query_points=np.concatenate([pts[:50], rng.uniform(-1, 2, (100, 3))], 0), seg_th_idx=[3, 6]))
    # (c) a single-point cloud
    pts = np.array([[0.1, -0.2, 0.3]])
    lines = rand_lines(rng, 6, -1, 1, 2.0)
    th = [0.1, 0.5, 1.0] + exact_thresholds(pts, lines, 1000, [0, 2500])
    out.append(dict(name="single", points=pts, lines=lines, ref_lines=lines[:3][:, ::-1].copy(),
                    thresholds=np.array(th), query_points=rng.uniform(-1, 1, (20, 3)), seg_th_idx=[1]))
    # (d) an empty line list against a small cloud
    pts = rng.uniform(0, 1, (300, 3))
    out.append(dict(name="empty", points=pts, lines=np.zeros((0, 6)), ref_lines=rand_lines(rng, 4, 0, 1, 0.5),
                    thresholds=np.array([0.01, 0.1]), query_points=rng.uniform(0, 1, (10, 3)), seg_th_idx=[0]))
    return out


def timing(L):
    rng = np.random.default_rng(7)
    n, nl = 1_000_000, 5000
    # a cloud on the faces of a box (a surface like a scanned room) and lines near it
    pts = rng.uniform(0, 10, (n, 3))
    face = rng.integers(0, 6, n)
    pts[np.arange(n), face % 3] = np.where(face < 3, 0.0, 10.0)
    lines = rand_lines(rng, nl, 0, 10, 1.0)
    th = np.array([0.001, 0.005, 0.01])
    ms = np.zeros(3)
    t0 = time.time()
    L.ev_time_scene(P(f64(pts)), n, P(f64(lines)), nl, P(th), th.size, P(ms))
    return dict(scene="1e6 points on the faces of a 10^3 box x 5000 random lines of length <= 1, thresholds "
                      "0.001/0.005/0.01, 1000 samples", points=n, lines=nl, threads=int(L.ev_threads()),
                build_ms=float(ms[0]), inlier_ratios_ms=float(ms[1]), dists_for_each_point_ms=float(ms[2]),
                total_s=time.time() - t0, cpu=os.popen("lscpu | grep 'Model name'").read().split(":")[-1].strip())


def main():
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        if "--timing-only" not in sys.argv:
            for sc in scenes():
                res = run_reference(L, sc)
                arrays = {k: np.asarray(v) for k, v in sc.items() if k != "name"}
                np.savez_compressed(os.path.join(OUT, f"eval_{sc['name']}.npz"), **arrays,
                                    **{"out_" + k: v for k, v in res.items()})
                print(f"eval_{sc['name']}.npz: {len(res)} outputs")
        if "--no-timing" not in sys.argv:
            t = timing(L)
            with open(os.path.join(OUT, "eval_ref_time.json"), "w") as f:
                json.dump(t, f, indent=1)
            print(json.dumps(t))


if __name__ == "__main__":
    main()
