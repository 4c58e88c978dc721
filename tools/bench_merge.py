"""Times limap_amd.merging.merging (MergeToLineTracks) on the fit-and-merge headline scene: 100 views x 500 segments,
20 neighbours, 3D segments from synthetic.make_fit_segs.  Prints one JSON line: the device time of the pair kernels
(HIP events, lt_merge_get_timers), the host time inside the library, the wall time of the Python call (median over
--steps after --warmup), and next to them the reference's CPU time of MergeToLineTracks on the same scene as
tests/golden/make_merge_golden.py recorded it with its thread count
(tests/golden/merge/merge_ref_time.json).

usage: python tools/bench_merge.py [--steps 5] [--warmup 1] [--views 100] [--segs 500] [--nn 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--segs", type=int, default=500)
    ap.add_argument("--nn", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from limap_amd import merging, synthetic as syn
    sc = syn.make_scene(n_views=args.views, n_segs=args.segs, n_neighbors=args.nn, seed=args.seed)
    fit = syn.make_fit_segs(sc, seed=args.seed)
    cfg = syn.default_merging_cfg()
    linker = dict(linker2d=cfg["linker2d"], linker3d=cfg["linker3d"])
    call = (linker, sc.all_2d_segs(), syn.imagecols_of(sc), fit, sc.neighbors, cfg["var2d"])
    dev, host, wall = [], [], []
    ts = None
    for k in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        ts = merging.TrackSet.from_merge(*call)
        tracks = ts.tracks()
        t1 = time.perf_counter()
        if k >= args.warmup:
            dev.append(ts.merge_timers["device_ms"])
            host.append(ts.merge_timers["host_ms"])
            wall.append((t1 - t0) * 1e3)
    out = dict(scene=dict(n_views=args.views, n_segs=args.segs, n_neighbors=args.nn, seed=args.seed),
               steps=args.steps, device_ms=float(np.median(dev)), library_ms=float(np.median(host)),
               wall_ms=float(np.median(wall)), nodes=ts.graph.num_nodes(), edges=ts.graph.num_edges(),
               tracks=len(tracks))
    ref_path = os.path.join(ROOT, "tests", "golden", "merge", "merge_ref_time.json")
    if os.path.exists(ref_path):
        with open(ref_path) as f:
            ref = json.load(f)
        if ref.get("scene", {}).get("n_views") == args.views and ref["scene"].get("n_segs") == args.segs and \
                ref["scene"].get("n_neighbors") == args.nn and ref["scene"].get("seed") == args.seed:
            out["reference_cpu_ms"] = ref["merge_ms"]
            out["reference_threads"] = ref["threads"]
            out["same_graph_as_reference"] = (ref["n_nodes"], ref["n_edges"], ref["n_tracks"]) == \
                (out["nodes"], out["edges"], out["tracks"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
