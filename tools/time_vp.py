"""Times limap_amd.vplib on a scene of 100 images x 500 lines (a quarter of each image's lines through each of two
points, the rest clutter): the device path per scene and per image -- warm process, median of repeated runs, with the
stages of lt_vp_get_timers (host ms of upload + length filter, kernels, download, host tail; device ms of the
preference kernel and of the clustering kernel) -- and the library's host path on 1 thread and on 16 threads, the only
baseline there is (upstream's clustering is a third party that is not on disk).  Writes profiles/vp_timing.json.

usage: python tools/time_vp.py [--repeat 5] [--images 100] [--lines 500] [--out profiles/vp_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W_IMG, H_IMG = 1024.0, 768.0


def image_lines(rng, n):
    c = rng.uniform([0, 0], [W_IMG, H_IMG], (n, 2))
    ang = rng.uniform(0, np.pi, n)
    h = 0.5 * rng.uniform(45.0, 200.0, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    lines = np.concatenate([c - h, c + h], 1)
    for _ in range(2):
        k = rng.choice(n, n // 4, replace=False)
        pt = rng.uniform([-2000, -2000], [3000, 3000])
        d = lines[k, :2] - pt
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        lines[k, 2:] = lines[k, :2] + d * rng.uniform(45, 150, (len(k), 1)) + rng.normal(0, 0.2, (len(k), 2))
    return lines


def scene(n_img, n_lines, seed=13):
    rng = np.random.default_rng(seed)
    return {i: image_lines(rng, n_lines) for i in range(n_img)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--lines", type=int, default=500)
    ap.add_argument("--host-images", type=int, default=16, help="images of the scene the host path is timed on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vp_timing.json"))
    args = ap.parse_args()
    from limap_amd import vplib
    cfg = vplib.BaseVPDetectorConfig()
    sc = scene(args.images, args.lines)
    out = dict(images=args.images, lines_per_image=args.lines, num_hypotheses=cfg.num_hypotheses, repeat=args.repeat,
               stages="host ms: upload + length filter, kernels, download, host tail; device ms: k_vp_pref, k_vp_cluster")
    vplib.detect_vps({0: sc[0]}, cfg)  # warm: code objects, buffers
    res = vplib.detect_vps(sc, cfg)
    rows = []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        vplib.detect_vps(sc, cfg)
        rows.append([1e3 * (time.perf_counter() - t0)] + vplib.timers().tolist())
    med = np.median(np.array(rows), 0).tolist()
    out["device"] = dict(call_ms=med[0], upload_filter_ms=med[1], kernels_ms=med[2], download_ms=med[3], host_tail_ms=med[4],
                         k_vp_pref_ms=med[5], k_vp_cluster_ms=med[6], per_image_ms=med[0] / args.images,
                         vps=int(sum(r.count_vps() for r in res.values())))
    one = []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        vplib.detect_vps({0: sc[0]}, cfg)
        one.append(1e3 * (time.perf_counter() - t0))
    out["device"]["single_image_call_ms"] = float(np.median(one))
    sub = {i: sc[i] for i in range(min(args.host_images, args.images))}
    out["host"] = dict(images=len(sub))
    for nt in (1, 16):
        t0 = time.perf_counter()
        h = vplib.detect_vps_host(sub, cfg, n_threads=nt)
        ms = 1e3 * (time.perf_counter() - t0)
        out["host"][f"threads_{nt}_ms"] = ms
        out["host"][f"threads_{nt}_per_image_ms"] = ms / len(sub)
        out["host"][f"threads_{nt}_scene_ms_extrapolated"] = ms / len(sub) * args.images
        assert all(h[i].labels == res[i].labels for i in sub), "host and device disagree"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
