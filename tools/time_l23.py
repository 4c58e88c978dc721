"""Times the 2D-3D line matching of limap_amd.localization on the scene of a localization run:
100 queries of 1000 lines, each with 20 retrieved database images of 1000 lines, 5000 tracks, the "epipolar" matcher
(all_pairs: 2 * 10^9 pair tests), without a filter and with the Perpendicular reprojection filter at dist_thres 2.
Segments are images of the tracks' lines (half of a database image's lines belong to a track, the rest is clutter);
a query's coarse pose is some two degrees and five centimetres off.  Warm process (one untimed call first), the median
of repeated calls of lt_l23_match with the stages of lt_l23_get_timers (host ms of validation + upload, launches,
download; device ms per stage by HIP events around the launches), then lt_fn_l23_host on 16 threads for the same call,
once, checked to give the same bytes.  Upstream's Python loop is not timed here and the parent commit has no such
step: the figures are a record.  Not measured: hardware counters, occupancy, the share of the divisions in k_l23_pairs.
Writes profiles/l23_timing.json.

usage: python tools/time_l23.py [--repeat 3] [--queries 100] [--out profiles/l23_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KVEC = np.array([600.0, 590.0, 400.0, 300.0])


def _rot(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _project(cam, X):
    pc = X @ _rot(cam[4:8]).T + cam[8:11]
    return np.stack([KVEC[0] * pc[:, 0] / pc[:, 2] + KVEC[2], KVEC[1] * pc[:, 1] / pc[:, 2] + KVEC[3]], 1)


def scene(n_query, n_db=200, n_lines=1000, n_retrieved=20, n_tracks=5000, seed=0):
    rng = np.random.default_rng(seed)
    a = np.column_stack([rng.uniform(-4, 4, n_tracks), rng.uniform(-3, 3, n_tracks), rng.uniform(5, 9, n_tracks)])
    tracks6 = np.concatenate([a, a + rng.normal(0, 0.25, (n_tracks, 3))], 1)

    def cam(k, n, off=0.0):
        ang = 0.2 * (k / max(n - 1, 1) - 0.5) + off
        return np.concatenate([KVEC, [np.cos(ang / 2), 0.0, np.sin(ang / 2), 0.0], [2.0 * (k / max(n - 1, 1) - 0.5) + off, 0.02 * off, off]])

    def view(c, n_from_tracks):
        ids = rng.permutation(n_tracks)[:n_from_tracks]
        segs = np.concatenate([_project(c, tracks6[ids, :3]), _project(c, tracks6[ids, 3:])], 1) + rng.normal(0, 0.5, (n_from_tracks, 4))
        p = np.column_stack([rng.uniform(0, 800, n_lines - n_from_tracks), rng.uniform(0, 600, n_lines - n_from_tracks)])
        segs = np.concatenate([segs, np.concatenate([p, p + rng.normal(0, 40, p.shape)], 1)], 0)
        trk = np.concatenate([ids, -np.ones(n_lines - n_from_tracks, np.int64)])
        o = rng.permutation(n_lines)
        return segs[o], trk[o]

    db_cams = [cam(d, n_db) for d in range(n_db)]
    views = [view(c, n_lines // 2) for c in db_cams]
    q_cams = [cam(q, n_query, 0.03) for q in range(n_query)]
    q_segs = [view(cam(q, n_query), n_lines)[0] for q in range(n_query)]
    tasks = [[int(d) for d in rng.permutation(n_db)[:n_retrieved]] for _ in range(n_query)]
    return (db_cams, [v[0] for v in views], [v[1] for v in views], q_cams, q_segs, tasks, None, tracks6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--lines", type=int, default=1000)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l23_timing.json"))
    args = ap.parse_args()
    from limap_amd import localization as loc
    sc = loc.scene_arrays(*scene(args.queries, n_lines=args.lines))
    pairs = float(sum(int(sc["q_seg_off"][q + 1] - sc["q_seg_off"][q]) * sum(int(sc["db_seg_off"][d + 1] - sc["db_seg_off"][d])
                      for d in sc["task_db"][sc["task_off"][q]:sc["task_off"][q + 1]]) for q in range(args.queries)))
    report = dict(scene=dict(queries=args.queries, lines_per_image=args.lines, retrieved=20, database_images=200, tracks=5000,
                             pair_tests=pairs, mode="all_pairs", IoU_threshold=0.2), repeat=args.repeat, runs={})
    for label, kw in (("no_filter", dict()), ("perpendicular_filter", dict(dist_func="Perpendicular", dist_thres=2.0))):
        loc.match_lines_arrays(sc, "all_pairs", **kw)  # warm: code objects, buffers
        walls, timers = [], []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            res = loc.match_lines_arrays(sc, "all_pairs", **kw)
            walls.append(1e3 * (time.perf_counter() - t0))
            timers.append(res["timers"])
        med = {k: float(np.median([t[k] for t in timers])) for k in timers[0]}
        t0 = time.perf_counter()
        twin = loc.match_lines_arrays(sc, "all_pairs", host_threads=args.host_threads, **kw)
        host_ms = 1e3 * (time.perf_counter() - t0)
        same = (np.array_equal(twin["rows"], res["rows"]) and np.array_equal(twin["q_off"], res["q_off"])
                and twin["loss"].tobytes() == res["loss"].tobytes())
        kernels = med["count_device_ms"] + med["fill_device_ms"]
        report["runs"][label] = dict(rows=int(len(res["rows"])), call_wall_ms_median=float(np.median(walls)), call_wall_ms=walls,
                                     stages_ms_median=med, pair_tests_per_second_count_pass=pairs / (1e-3 * med["count_device_ms"]),
                                     pair_tests_per_second_both_passes=2.0 * pairs / (1e-3 * kernels),
                                     host_twin_threads=args.host_threads, host_twin_wall_ms=host_ms, host_twin_same_bytes=bool(same))
        print(label, json.dumps(report["runs"][label]))
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
