"""Times limap_amd.structures on the inputs whose reference times tests/golden/make_bpt_golden.py recorded
(tests/golden/bpt/bpt_ref_time.json): the keypoint-line association of a scene and the junctions of single images.
Warm process, median of repeated runs; per run the stages of lt_bpt_get_timers (host ms between stream
synchronisations: upload, kernels, sorts, download + host replay), the wall time of the native path and of the whole
Python call.  Writes profiles/bpt_timing.json.

usage: python tools/time_bipartite.py [--repeat 7] [--out profiles/bpt_timing.json]
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
ASSOC_SHAPE = (100, 500, 2000)  # images, lines per image, keypoints per image
JUNCTION_LINES = (500, 1000)


def rand_lines(rng, n, lo=20.0, hi=150.0):
    """n segments inside the image, lengths lo..hi pixels"""
    c = rng.uniform([0, 0], [W_IMG, H_IMG], (n, 2))
    ang = rng.uniform(0, np.pi, n)
    h = 0.5 * rng.uniform(lo, hi, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    return np.concatenate([c - h, c + h], 1)


def rand_points(rng, n):
    return rng.uniform([0, 0], [W_IMG, H_IMG], (n, 2))


def assoc_scene(seed=11):
    """the association input: per image (lines (M, 4), keypoints (P, 2))"""
    rng = np.random.default_rng(seed)
    n, m, p = ASSOC_SHAPE
    return [(rand_lines(rng, m), rand_points(rng, p)) for _ in range(n)]


def junction_scene(n_lines, seed=12):
    """one image of the junction input: (lines (M, 4), keypoints (3000, 2))"""
    rng = np.random.default_rng([seed, n_lines])
    return rand_lines(rng, n_lines), rand_points(rng, 3000)


def median_runs(fn, repeat):
    rows = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        stages = fn()
        rows.append([1e3 * (time.perf_counter() - t0)] + list(stages))
    return np.median(np.array(rows), 0).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bpt_timing.json"))
    args = ap.parse_args()
    from limap_amd import structures as st
    cfg = st.PL_Bipartite2dConfig()
    out = dict(repeat=args.repeat, stages="host ms between stream synchronisations: upload, kernels, sorts, "
               "download + host replay; native = the C call and its getters, call = the Python entry point")

    scene = assoc_scene()
    lines, pts = [a for a, _ in scene], [p for _, p in scene]
    st._associate(lines[:2], pts[:2], cfg)  # warm: code objects, buffers
    st._associate(lines, pts, cfg)
    native = median_runs(lambda: (st._associate(lines, pts, cfg), st.timers())[1], args.repeat)
    kp = {i: (pts[i], np.arange(pts[i].shape[0]), None) for i in range(len(scene))}
    l2d = {i: lines[i] for i in range(len(scene))}
    call = median_runs(lambda: (st.compute_2d_bipartites(l2d, kp, cfg), [])[1], max(args.repeat // 2, 1))
    out["association"] = dict(images=len(scene), lines_per_image=ASSOC_SHAPE[1], keypoints_per_image=ASSOC_SHAPE[2],
                              native_ms=native[0], upload_ms=native[1], kernels_ms=native[2], sort_ms=native[3],
                              download_replay_ms=native[4], call_ms=call[0])
    out["junctions"] = []
    for m in JUNCTION_LINES:
        a, k = junction_scene(m)
        res = st._junctions([a], [k], cfg)
        native = median_runs(lambda: (st._junctions([a], [k], cfg), st.timers())[1], args.repeat)
        out["junctions"].append(dict(lines=m, keypoints=int(k.shape[0]), junctions=int(res[0][0].shape[0]),
                                     native_ms=native[0], upload_ms=native[1], kernels_ms=native[2], sort_ms=native[3],
                                     download_replay_ms=native[4]))
    # a scene-sized batch of junction images: what one call for the whole scene costs per image
    batch = [junction_scene(500, seed=100 + i) for i in range(20)]
    bl, bk = [a for a, _ in batch], [k for _, k in batch]
    st._junctions(bl, bk, cfg)
    native = median_runs(lambda: (st._junctions(bl, bk, cfg), st.timers())[1], max(args.repeat // 2, 1))
    out["junctions_batch"] = dict(images=len(batch), lines=500, native_ms=native[0], upload_ms=native[1],
                                  kernels_ms=native[2], sort_ms=native[3], download_replay_ms=native[4],
                                  per_image_ms=native[0] / len(batch))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
