"""Times the point-line pose refinement and the pose scoring (limap_amd.hybrid_localization).
Solve: one call of 1 and of 2000 problems (200 3D lines with one 2D segment each + 500 points per problem, 0.5 px noise,
the initial pose off by 0.02 rad and 0.05 units; E2DPerpendicularDist2, CauchyLoss(2)): warm process, median of repeated
calls of lt_loc_solve with the stages of lt_loc_get_timers (host ms of validation + table + upload, kernel, download;
device ms of k_loc_lm by HIP events), and lt_fn_loc_host on 16 threads, checked to give the same bits.  Scoring: 1000
poses x 700 correspondences (500 points + 200 segments) with the MSAC score.  There is no Ceres to time against: the
figures are a record.  Writes profiles/loc_timing.json.

usage: python tools/time_loc.py [--repeat 5] [--out profiles/loc_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _quat(rotvec):
    th = np.linalg.norm(rotvec, axis=-1, keepdims=True)
    return np.concatenate([np.cos(th / 2), np.sin(th / 2) * rotvec / np.maximum(th, 1e-300)], -1)


def _rot(q):
    w, x, y, z = np.moveaxis(q, -1, 0)
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def _qmul(a, b):
    aw, ax, ay, az = np.moveaxis(a, -1, 0)
    bw, bx, by, bz = np.moveaxis(b, -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def problems_csr(P, n_lines=200, n_points=500, seed=0):
    """P problems as the CSR arrays of lt_loc_solve, built with array operations"""
    rng = np.random.default_rng(seed)
    k = np.tile([520.0, 515.0, 320.0, 240.0], (P, 1))
    q_gt = _quat(rng.normal(0, 0.3, (P, 3)))
    t_gt = rng.normal(0, 0.5, (P, 3))
    R = _rot(q_gt)

    def cam(n):
        return np.stack([rng.uniform(-1.5, 1.5, (P, n)), rng.uniform(-1.1, 1.1, (P, n)), rng.uniform(3.0, 7.0, (P, n))], -1)

    def world(Y):
        return np.einsum("pji,pnj->pni", R, Y - t_gt[:, None, :])

    def pix(Y):
        return np.stack([k[:, None, 0] * Y[..., 0] / Y[..., 2] + k[:, None, 2], k[:, None, 1] * Y[..., 1] / Y[..., 2] + k[:, None, 3]], -1)
    a = cam(n_lines)
    b = a + rng.normal(0, 0.6, a.shape)
    b[..., 2] = np.clip(b[..., 2], 2.5, 8.0)
    pts = cam(n_points)
    l3 = np.concatenate([world(a), world(b)], -1).reshape(-1, 6)
    sg = (np.concatenate([pix(a), pix(b)], -1) + rng.normal(0, 0.5, (P, n_lines, 4))).reshape(-1, 4)
    p3 = world(pts).reshape(-1, 3)
    p2 = (pix(pts) + rng.normal(0, 0.5, (P, n_points, 2))).reshape(-1, 2)
    dr = rng.normal(0, 1, (P, 3)); dr *= 0.02 / np.linalg.norm(dr, axis=1, keepdims=True)
    dt = rng.normal(0, 1, (P, 3)); dt *= 0.05 / np.linalg.norm(dt, axis=1, keepdims=True)
    q0, t0 = _qmul(_quat(dr), q_gt), t_gt + dt
    c = np.ascontiguousarray
    return (P, c(k), c(q0), c(t0), np.arange(P + 1, dtype=np.int64) * n_lines, c(l3), np.arange(P * n_lines + 1, dtype=np.int64),
            c(sg), np.arange(P + 1, dtype=np.int64) * n_points, c(p3), c(p2)), (q_gt, t_gt)


def measure_solve(P, repeat):
    from limap_amd import _capi, hybrid_localization as hl
    csr, _ = problems_csr(P)
    cfg = hl.LineLocConfig(dict(loss_function=hl.CauchyLoss(2.0)))
    c = cfg._struct()
    ctx = _capi.Context()
    hl.loc_arrays(csr, c, ctx=ctx)  # warm: code object, buffers
    rows = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = hl.loc_arrays(csr, c, ctx=ctx)
        tm = r["timers"]
        rows.append([1e3 * (time.perf_counter() - t0), tm["prepare_ms"], tm["kernel_ms"], tm["download_ms"], tm["lm_device_ms"]])
    med = np.median(np.array(rows), 0).tolist()
    t0 = time.perf_counter()
    h = hl.loc_arrays(csr, c, host_threads=16)
    host_ms = 1e3 * (time.perf_counter() - t0)
    for key in ("qvec", "tvec", "cost", "iterations", "codes"):
        assert np.array_equal(h[key], r[key]), f"host and device disagree on {key}"
    return dict(problems=P, blocks_per_problem=700, repeat=repeat,
                device=dict(call_ms=med[0], prepare_ms=med[1], kernel_ms=med[2], download_ms=med[3], k_loc_lm_ms=med[4]),
                host_16_threads_ms=host_ms, iterations_median=float(np.median(r["iterations"])),
                iterations_max=int(r["iterations"].max()), codes=np.bincount(r["codes"], minlength=8).tolist())


def measure_score(H, repeat):
    from limap_amd import _capi, hybrid_localization as hl
    csr, (q_gt, t_gt) = problems_csr(1, seed=5)
    rng = np.random.default_rng(6)
    poses = np.concatenate([_qmul(_quat(rng.normal(0, 0.05, (H, 3))), np.tile(q_gt, (H, 1))), t_gt + rng.normal(0, 0.3, (H, 3))], 1)
    a = ("PerpendicularDist", csr[5].reshape(-1, 2, 3), np.arange(200), csr[7].reshape(-1, 2, 2), csr[9], csr[10], csr[1][0], poses)
    ctx = _capi.Context()
    kw = dict(thresholds=(16.0, 16.0), weights=(1.0, 1.0))
    hl.score_poses(*a, ctx=ctx, **kw)
    rows = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = hl.score_poses(*a, ctx=ctx, **kw)
        tm = r["timers"]
        rows.append([1e3 * (time.perf_counter() - t0), tm["prepare_ms"], tm["kernel_ms"], tm["download_ms"], tm["score_device_ms"]])
    med = np.median(np.array(rows), 0).tolist()
    t0 = time.perf_counter()
    h = hl.score_poses(*a, host_threads=16, **kw)
    host_ms = 1e3 * (time.perf_counter() - t0)
    for key in ("residuals", "scores", "inliers"):
        assert np.array_equal(h[key], r[key]), f"host and device disagree on {key}"
    return dict(poses=H, correspondences=700, repeat=repeat,
                device=dict(call_ms=med[0], prepare_ms=med[1], kernel_ms=med[2], download_ms=med[3], k_loc_score_ms=med[4]),
                host_16_threads_call_ms=host_ms, failed_cells=float((r["residuals"] == np.finfo(float).max).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loc_timing.json"))
    args = ap.parse_args()
    out = dict(method="warm process; median of `repeat` calls; stages from lt_loc_get_timers / lt_loc_score_get_timers; "
                      "call_ms includes the Python marshalling; host path timed once",
               solve=[measure_solve(1, args.repeat), measure_solve(2000, args.repeat)], score=measure_score(1000, args.repeat))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
