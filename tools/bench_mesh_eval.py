"""Times limap_amd.evaluation.MeshEvaluator on synthetic rooms: the six walls of a 10 m box, each a grid of squares cut
into two triangles, with a height perturbation of up to 1 cm so that the surface is not piecewise planar, at about 10^6
and 10^7 triangles.  Per mesh: index build (lt_mesh_build), inlier ratios of 5 000 random lines of length <= 1 m x 1000
samples at thresholds 1 / 5 / 10 mm in one pass (ComputeInlierRatios), and ComputeDistPoints of 10^6 queries within
2 cm of the surface.  On the smaller mesh also the brute-force form (LT_TEST_MESH_BRUTE) on a subset of those queries
beside the walk on the same subset, so that the pruning factor is visible, and (--buckets) the same calls for other
bucket sizes (LT_TEST_MESH_BUCKET).  Prints one JSON line: device ms of each call's kernels (HIP events,
lt_eval_get_timers) and wall ms of the Python call, medians over --steps after --warmup.

usage: python tools/bench_mesh_eval.py [--steps 5] [--warmup 1] [--faces 1000000,10000000] [--lines 5000]
                                       [--buckets 4,8,16,32] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("LT_ENABLE_TEST_SWITCHES", "1")  # the brute-force form and the bucket sizes are test switches
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def room(target_faces, seed=7, bump=0.01):
    """the box's six walls, 12 n^2 triangles, n = sqrt(target / 12)"""
    rng = np.random.default_rng(seed)
    n = max(1, int(round((target_faces / 12) ** 0.5)))
    t = np.linspace(0.0, 10.0, n + 1)
    X, Y = np.meshgrid(t, t, indexing="ij")
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    Fg = np.concatenate([np.stack([i, i + n + 1, i + 1], 1), np.stack([i + 1, i + n + 1, i + n + 2], 1)], 0)
    Vs, Fs, off = [], [], 0
    for axis in range(3):
        for side in (0.0, 10.0):
            W = np.empty(((n + 1) ** 2, 3))
            o = [k for k in range(3) if k != axis]
            W[:, o[0]], W[:, o[1]] = X.ravel(), Y.ravel()
            W[:, axis] = side + bump * rng.uniform(-1, 1, W.shape[0])
            Vs.append(W)
            Fs.append(Fg + off)
            off += W.shape[0]
    return np.concatenate(Vs), np.concatenate(Fs)


def near_queries(V, F, m, seed=11):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, F.shape[0], m)
    w = rng.dirichlet([1, 1, 1], m)
    return (w[:, 0:1] * V[F[k, 0]] + w[:, 1:2] * V[F[k, 1]] + w[:, 2:3] * V[F[k, 2]]) + rng.uniform(-0.02, 0.02, (m, 3))


def random_lines(n, seed=13):
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 10, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([s, s + d * rng.uniform(0.01, 1.0, (n, 1))], 1)


def timed(E, fn, steps, warmup):
    dev, wall = [], []
    for k in range(warmup + steps):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if k >= warmup:
            dev.append(float(E.timers()[0]))
            wall.append((t1 - t0) * 1e3)
    return float(np.median(dev)), float(np.median(wall))


def run(ev, V, F, lines, Q, th, steps, warmup, brute_q=0):
    E = ev.MeshEvaluator.from_arrays(V, F, 1.0)
    b_dev, b_wall = timed(E, E.Build, steps, warmup)
    levels = int(E.timers()[3])
    r_dev, r_wall = timed(E, lambda: E.ComputeInlierRatios(lines, th), steps, warmup)
    p_dev, p_wall = timed(E, lambda: E.ComputeDistPoints(Q), steps, warmup)
    rep = ev.report_error_to_GT(E, lines, th)
    out = dict(faces=int(F.shape[0]), levels=levels, build_dev_ms=b_dev, build_wall_ms=b_wall, ratios_dev_ms=r_dev,
               ratios_wall_ms=r_wall, points=int(Q.shape[0]), points_dev_ms=p_dev, points_wall_ms=p_wall,
               precision=rep["precision"].tolist(), recall=rep["recall"].tolist())
    if brute_q:
        sub = Q[:brute_q]
        w_dev, _ = timed(E, lambda: E.ComputeDistPoints(sub), steps, warmup)
        walk = E.ComputeDistPoints(sub)
        os.environ["LT_TEST_MESH_BRUTE"] = "1"
        try:
            bf_dev, _ = timed(E, lambda: E.ComputeDistPoints(sub), max(1, min(steps, 2)), min(warmup, 1))
            brute = E.ComputeDistPoints(sub)
        finally:
            del os.environ["LT_TEST_MESH_BRUTE"]
        out.update(brute_points=brute_q, walk_subset_dev_ms=w_dev, brute_subset_dev_ms=bf_dev,
                   pruning_factor=bf_dev / w_dev,
                   walk_equals_brute=bool(np.array_equal(walk.view(np.int64), brute.view(np.int64))))
    del E
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--faces", default="1000000,10000000")
    ap.add_argument("--lines", type=int, default=5000)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--brute-points", type=int, default=20000)
    ap.add_argument("--buckets", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from limap_amd import evaluation as ev
    th = [0.001, 0.005, 0.01]
    lines = random_lines(args.lines)
    res = dict(lines=args.lines, samples=1000, thresholds=th, steps=args.steps, runs=[], buckets=[])
    sizes = [int(x) for x in args.faces.split(",") if x]
    for k, target in enumerate(sizes):
        V, F = room(target)
        Q = near_queries(V, F, args.points)
        res["runs"].append(run(ev, V, F, lines, Q, th, args.steps, args.warmup,
                               brute_q=args.brute_points if k == 0 else 0))
        if k == 0 and args.buckets:
            for b in [int(x) for x in args.buckets.split(",")]:
                os.environ["LT_TEST_MESH_BUCKET"] = str(b)
                try:
                    r = run(ev, V, F, lines, Q, th, args.steps, args.warmup)
                finally:
                    del os.environ["LT_TEST_MESH_BUCKET"]
                r["bucket"] = b
                res["buckets"].append(r)
        del V, F, Q
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
