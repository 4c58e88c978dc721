#!/usr/bin/env python3
"""Times the global point-line association on one GPU and writes profiles/assoc_timing.json.

Scene: section 27's timing scene (tools/time_ba.py: 100 images, about 30 000 point tracks, 1 367 line tracks) with
generated incidences -- the point tracks nearest to three positions on every line track (a few centimetres to decimetres
away: the Huber loss bounds them) -- and three vanishing-point tracks along
the coordinate axes, every line tied to the nearest.  Protocol: a warm process (one call before the clock), the median of
five calls by the host clock, per-kernel times by HIP events summed over the batches in a call of their own
(kernel_timers), CG iterations per attempt, and the host twin on 16 threads checked to give the same bits.  A record, not
a bar: there is no Ceres to time against.

    python tools/time_assoc.py [--out profiles/assoc_timing.json] [--iterations 30] [--points 30000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def make_scene(n_points, seed=0):
    import assoc_scenes as sc
    import time_ba
    rng = np.random.default_rng(seed + 1)
    s = time_ba.make_scene(n_points, seed)
    NL = len(s["loff"]) - 1
    edges = set()
    for n in range(NL):  # the point tracks nearest to three positions on the line
        a, b = s["line6"][n, :3], s["line6"][n, 3:]
        for u in (0.2, 0.5, 0.8):
            X = a + u * (b - a)
            edges.add((sc.PL, int(np.argmin(((s["p3"] - X) ** 2).sum(1))), n))
    edges = [(k, p, n, int(rng.integers(3, 8))) for k, p, n in sorted(edges)]
    edges.sort()
    vps = np.eye(3) + rng.normal(0, 0.02, (3, 3))
    vps /= np.linalg.norm(vps, axis=1, keepdims=True)
    d = s["line6"][:, 3:] - s["line6"][:, :3]
    cls = np.argmax(np.abs(d / np.linalg.norm(d, axis=1, keepdims=True) @ np.eye(3)), axis=1)
    edges += sorted((sc.VL, int(cls[n]), n, int(rng.integers(3, 8))) for n in range(NL))
    edges += [(sc.ORTH, 0, 1, 1), (sc.ORTH, 0, 2, 1), (sc.ORTH, 1, 2, 1)]
    return sc._with_edges(s, vps, edges)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc_timing.json"))
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--points", type=int, default=30000)
    a = ap.parse_args()
    import assoc_scenes as sc
    from limap_amd import _capi
    from limap_amd.global_pl_association import _KERNELS
    s = make_scene(a.points)
    ctx = _capi.Context()
    L = ctx.L
    cfg = sc.cfg_of(max_num_iterations=a.iterations)

    def timers():
        tm = np.zeros(20)
        ctx.chk(L.lt_assoc_get_timers(ctx.h, _capi.ptr(tm, C.c_double)))
        return tm
    rc, dev = sc.run_device(ctx, s, cfg)  # warm
    assert rc == 0, L.lt_last_error(ctx.h)
    wall, loop = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        rc, dev = sc.run_device(ctx, s, cfg)
        wall.append((time.perf_counter() - t0) * 1e3)
        loop.append(float(timers()[1]))
    batches = int(timers()[3])
    rc, prof = sc.run_device(ctx, s, sc.cfg_of(max_num_iterations=a.iterations, kernel_timers=1))
    tm = timers()
    kern = {"k_as_" + n: float(tm[4 + i]) for i, n in enumerate(_KERNELS)}
    total = sum(kern.values())
    t0 = time.perf_counter()
    rc, host, tr = sc.run_host(s, cfg, 16, trace=a.iterations + 8)
    host_ms = (time.perf_counter() - t0) * 1e3
    ev = sc.evaluate(s, cfg)
    rec = dict(scene=dict(images=len(s["img_ids"]), point_tracks=len(s["poff"]) - 1, point_observations=int(s["poff"][-1]),
                          line_tracks=len(s["loff"]) - 1, line_supports=int(s["loff"][-1]), vps=len(s["vp3"]),
                          edges=int(ev["dims"][5]), r1_blocks=int(ev["dims"][4]), unknowns=int(ev["dims"][0]),
                          free_dimensions=int(ev["nd"].sum())),
               max_num_iterations=a.iterations, iterations=int(dev["iterations"][0]), code=int(dev["code"][0]),
               cost=[float(x) for x in dev["cost"]], cg_iterations=int(dev["cg_iterations"][0]),
               cg_iterations_per_attempt=[int(x) for x in tr["rec"][:, 5]],
               call_ms_median_of_5=float(np.median(wall)), call_ms=wall, loop_ms_median_of_5=float(np.median(loop)),
               batches_enqueued=batches, kernels_ms_sum_over_batches=kern,
               kernels_share={n: (v / total if total > 0 else 0.0) for n, v in kern.items()},
               host_twin_16_threads_ms=host_ms, host_twin_same_bits=bool(sc.same_bits(dev, host)),
               kernel_timer_run_same_bits=bool(sc.same_bits(dev, prof)),
               not_measured="hardware counters; occupancy beyond the compiler's resource report; the per-kernel times "
                            "include the launches that return at once because the record is in another phase")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
