#!/usr/bin/env python3
"""Times the bundle adjustment with free poses on one GPU and writes profiles/ba_timing.json.

Scene in the shape of runners/hypersim/refine_sfm.py: 100 images, about 30 000 point tracks of 3 to 12 observations,
the 1 367 line tracks of tests/refine_scenes.make_tracks, poses and structure perturbed.  Protocol: a warm process (one
call before the clock), the median of five calls by the host clock, per-kernel times by HIP events in a call of their own
(kernel_timers: the status record is then read after every attempt), iterations and code, and the host twin on 16
threads checked to give the same bits.  A record, not a bar: there is no Ceres to time against.

    python tools/time_ba.py [--out profiles/ba_timing.json] [--iterations 30] [--points 30000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_scene(n_points, seed=0):
    import ba_scenes as bs
    import refine_scenes as rs
    rng = np.random.default_rng(seed)
    s = rs.make_tracks(n_tracks=1367, n_views=100, seed=seed)
    ids, k, q, t = s["img_ids"], s["k"], s["q"], s["t"]
    R = np.stack([bs.quat_to_rot(x) for x in q])
    p_gt, poff, pimg, pxy = [], [0], [], []
    while len(p_gt) < n_points:
        X = rng.uniform([0.5, 0.5, 0.2], [9.5, 7.5, 2.8], (4096, 3))
        cam = np.einsum("cij,nj->cni", R, X) + t[:, None, :]
        z = cam[..., 2]
        u = k[:, None, 0] * cam[..., 0] / z + k[:, None, 2]
        v = k[:, None, 1] * cam[..., 1] / z + k[:, None, 3]
        ok = (z > 0.5) & (u > 0) & (u < 800) & (v > 0) & (v < 600)
        for n in range(len(X)):
            vis = np.flatnonzero(ok[:, n])
            if len(vis) < 3 or len(p_gt) >= n_points:
                continue
            sel = rng.permutation(vis)[:int(rng.integers(3, 13))]
            p_gt.append(X[n])
            for c in sel:
                pimg.append(int(ids[c]))
                pxy.append([u[c, n] + rng.normal(0, 0.5), v[c, n] + rng.normal(0, 0.5)])
            poff.append(len(pimg))
    p_gt = np.array(p_gt)
    q0, t0 = q.copy(), t.copy()
    for i in range(len(ids)):
        dq = np.concatenate([[1.0], rng.normal(0, 0.002, 3)])
        q0[i] = bs.quat_mul(dq / np.linalg.norm(dq), q[i])
        t0[i] = t[i] + rng.normal(0, 0.01, 3)
    c = np.ascontiguousarray
    return dict(img_ids=c(ids, np.int32), k=c(k), q=c(q0), t=c(t0), p3=c(p_gt + rng.normal(0, 0.02, p_gt.shape)),
                poff=np.array(poff, np.int64), pimg=np.array(pimg, np.int32), pxy=c(np.array(pxy)), line6=c(s["line6"]),
                loff=c(s["off"], np.int64), limg=c(s["img"], np.int32), l2d=c(s["l2d"]), l3d=c(s["l3d"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_timing.json"))
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--points", type=int, default=30000)
    a = ap.parse_args()
    import ba_scenes as bs
    from limap_amd import _capi
    s = make_scene(a.points)
    ctx = _capi.Context()
    L = ctx.L
    cfg = bs.cfg_of(max_num_iterations=a.iterations)

    def timers():
        tm = np.zeros(16)
        ctx.chk(L.lt_ba_get_timers(ctx.h, _capi.ptr(tm, __import__("ctypes").c_double)))
        return tm
    rc, dev = bs.run_device(ctx, s, cfg)  # warm
    assert rc == 0, L.lt_last_error(ctx.h)
    wall, loop = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        rc, dev = bs.run_device(ctx, s, cfg)
        wall.append((time.perf_counter() - t0) * 1e3)
        loop.append(float(timers()[1]))
    rc, prof = bs.run_device(ctx, s, bs.cfg_of(max_num_iterations=a.iterations, kernel_timers=1))
    tm = timers()
    names = ("linearize", "blocks", "images", "damp", "schur", "chol", "backsub", "cost", "decide")
    kern = {"k_ba_" + n: float(tm[4 + i]) for i, n in enumerate(names)}
    total = sum(kern.values())
    t0 = time.perf_counter()
    rc, host = bs.run_host(s, cfg, 16)
    host_ms = (time.perf_counter() - t0) * 1e3
    n_img = len(s["img_ids"])
    rec = dict(scene=dict(images=n_img, point_tracks=len(s["poff"]) - 1, point_observations=int(s["poff"][-1]),
                          line_tracks=len(s["loff"]) - 1, line_supports=int(s["loff"][-1])),
               S=dict(unknowns=6 * n_img, bytes=8 * (6 * n_img) ** 2), max_num_iterations=a.iterations,
               iterations=int(dev["iterations"][0]), code=int(dev["code"][0]), cost=[float(x) for x in dev["cost"]],
               call_ms_median_of_5=float(np.median(wall)), call_ms=wall, loop_ms_median_of_5=float(np.median(loop)),
               poll_interval=int(L.lt_ba_poll_default()), kernels_ms_sum_over_attempts=kern,
               kernels_share={n: (v / total if total > 0 else 0.0) for n, v in kern.items()},
               host_twin_16_threads_ms=host_ms, host_twin_same_bits=bool(bs.same_bits(dev, host)),
               kernel_timer_run_same_bits=bool(bs.same_bits(dev, prof)),
               not_measured="hardware counters; occupancy beyond the compiler's resource report")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
