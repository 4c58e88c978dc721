"""Times limap_amd.fitting.fit_3d_segs_with_points3d_arrays (the scan fitter of line_fitting_with_points3d) on the
scan headline scene: 100 views x 500 segments at 1024 x 768 with float64 scans (synthetic.render_scans, 0.2 % depth
noise, 2 % NaN holes).  Prints one JSON line: the device time of the fit kernel (HIP events, lt_fit_get_timers) with
the scan upload reported apart, the host time inside the library, the wall time of the Python call (medians over
--steps after --warmup; host scans and scans already on the device), segments per second, the success rate, the mean
kept points / inliers / iterations per segment, and the same scene's first --oracle-segs segments through the Python
test oracle (tests/fit_scan_oracle.py): its time and whether the device equals it bit for bit.  There is no reference
timing: the reference's fitter needs RansacLib and hloc, which this tree does not build.

usage: python tools/bench_fit_scan.py [--steps 5] [--warmup 1] [--views 100] [--segs 500] [--h 768] [--w 1024]
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
    ap.add_argument("--h", type=int, default=768)
    ap.add_argument("--w", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--oracle-segs", type=int, default=100)
    args = ap.parse_args()
    import torch
    from limap_amd import fitting, synthetic as syn
    base = syn.make_scene(n_views=args.views, n_segs=args.segs, n_neighbors=2, seed=args.seed)
    sc = syn.resize_scene(base, args.h, args.w)
    scans = syn.render_scans(base, args.h, args.w, noise=0.002, hole_frac=0.02, dtype=np.float64, seed=args.seed)
    imagecols = syn.imagecols_of(sc, hw=(args.h, args.w))
    all_2d = sc.all_2d_segs()
    fc = dict(ransac_th=0.75, min_percentage_inliers=0.6, var2d=5.0)
    on_dev = {i: torch.from_numpy(d).to("cuda") for i, d in scans.items()}
    torch.cuda.synchronize()
    res = {}
    for name, maps in (("host_maps", scans), ("device_maps", on_dev)):
        dev, up, host, wall = [], [], [], []
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            arrs, info, tm = fitting.fit_3d_segs_with_points3d_arrays(all_2d, imagecols, maps, fc)
            t1 = time.perf_counter()
            if k >= args.warmup:
                dev.append(tm["device_ms"]); up.append(tm["upload_ms"]); host.append(tm["host_ms"])
                wall.append((t1 - t0) * 1e3)
        res[name] = dict(device_ms=float(np.median(dev)), upload_ms=float(np.median(up)),
                         library_ms=float(np.median(host)), wall_ms=float(np.median(wall)))
    ids = [int(i) for i in sc.img_ids]
    st = np.concatenate([info[i]["status"] for i in ids])
    stats = np.concatenate([info[i]["stats"] for i in ids])
    G = len(st)
    ran = (st != 1) & (st != 3)
    out = dict(scene=dict(n_views=args.views, n_segs=args.segs, h=args.h, w=args.w, dtype="float64", seed=args.seed),
               steps=args.steps, segments=G, **{f"{k}_{n}": v for n, r in res.items() for k, v in r.items()},
               segments_per_s=G / (res["host_maps"]["wall_ms"] / 1e3),
               success_rate=float((st == 0).mean()), too_few_rate=float((st == 1).mean()),
               mean_points=float(stats[:, 0].mean()), mean_inliers=float(stats[ran, 1].mean()),
               mean_iterations=float(stats[ran, 2].mean()), mean_lo=float(stats[ran, 3].mean()),
               max_points=int(stats[:, 0].max()))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fit_oracle as fo
    import fit_scan_oracle as so
    i0 = ids[0]
    n_or = min(args.oracle_segs, len(all_2d[i0]))
    t0 = time.perf_counter()
    same = True
    for l in range(n_or):
        r = so.fit_scan_segment(all_2d[i0][l], scans[i0], (args.h, args.w), sc.qvec[0], sc.tvec[0], i0, l,
                                fo.Options())
        same &= r["status"] == int(info[i0]["status"][l]) and np.array_equal(r["seg"].view(np.uint64),
                                                                                 arrs[i0][l].view(np.uint64))
    t1 = time.perf_counter()
    out["oracle_subset"] = dict(label=f"Python oracle, image {i0}, segments 0..{n_or - 1}", segments=n_or,
                                ms_per_segment=(t1 - t0) * 1e3 / max(n_or, 1), equal_to_device=bool(same))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
