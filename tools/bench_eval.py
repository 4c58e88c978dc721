"""Times limap_amd.evaluation on the evaluation headline scenes: 10^6 and 10^7 GT points on the faces of a 10 m box (a
scanned room's surfaces) against 5 000 random lines of length <= 1 m.  Per cloud size: index build (lt_pcd_build),
inlier ratios of L x 1000 samples at three thresholds in one pass (ComputeInlierRatios, the scripts' loop), and inverse
point recall (ComputeDistsforEachPoint, brute force P x L).  Prints one JSON line: device ms of each call's kernels (HIP
events, lt_eval_get_timers) and the wall ms of the Python call, medians over --steps after --warmup, and the FP64 issue
rate of the brute-force kernel (28 FP64 operations per point-segment pair against 39.3 T lane-operations/s, the
MI355X's 78.6 TFLOPS FP64 vector peak with an FMA counted once).  The reference's CPU times of the same 10^6-point scene
are in tests/golden/eval/eval_ref_time.json.

usage: python tools/bench_eval.py [--steps 5] [--warmup 1] [--points 1000000,10000000] [--lines 5000] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_OPS_PER_PAIR = 28
FP64_LANE_OPS_PEAK = 39.3e12


def scene(n, n_lines, seed=7):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0, 10, (n, 3))
    face = rng.integers(0, 6, n)
    pts[np.arange(n), face % 3] = np.where(face < 3, 0.0, 10.0)
    s = rng.uniform(0, 10, (n_lines, 3))
    d = rng.normal(size=(n_lines, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return pts, np.concatenate([s, s + d * rng.uniform(0.01, 1.0, (n_lines, 1))], 1)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--points", default="1000000,10000000")
    ap.add_argument("--lines", type=int, default=5000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from limap_amd import evaluation as ev
    th = [0.001, 0.005, 0.01]
    res = dict(lines=args.lines, samples=1000, thresholds=th, steps=args.steps, runs=[])
    for n in [int(x) for x in args.points.split(",")]:
        pts, lines = scene(n, args.lines)
        E = ev.PointCloudEvaluator(pts)
        b_dev, b_wall = timed(E, E.Build, args.steps, args.warmup)
        r_dev, r_wall = timed(E, lambda: E.ComputeInlierRatios(lines, th), args.steps, args.warmup)
        steps = max(1, args.steps if n <= 1_000_000 else min(args.steps, 2))
        d_dev, d_wall = timed(E, lambda: E.ComputeDistsforEachPoint(lines), steps, min(args.warmup, 1))
        rep = ev.report_error_to_GT(E, lines, th)
        pairs = float(n) * args.lines
        res["runs"].append(dict(
            points=n, build_dev_ms=b_dev, build_wall_ms=b_wall, ratios_dev_ms=r_dev, ratios_wall_ms=r_wall,
            dists_each_dev_ms=d_dev, dists_each_wall_ms=d_wall,
            brute_force_pairs_per_s=pairs / (d_dev * 1e-3),
            brute_force_fp64_fraction=pairs * FP64_OPS_PER_PAIR / (d_dev * 1e-3) / FP64_LANE_OPS_PEAK,
            precision=rep["precision"].tolist(), recall=rep["recall"].tolist()))
        del E
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
