"""limap_amd.pointsfm on a synthetic model of limap_amd.synthetic: the cameras of a config-2 / config-5 scene, the
endpoints of its GT segments as points, track of a point = the images that observe its segment.  Runs
``compute_metainfos`` on the device path and on the host path, checks that they agree, and prints one JSON line: E (pair
instances), unique image pairs, the stages of ``pointsfm.timers()`` and the host path's time.

usage: python tools/sfm_scene.py [--views 5000] [--segs 600] [--neighbors 20] [--threads 16] [--repeat 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {"min_triangulation_angle": 1.0, "neighbor_type": "iou", "ranges": {"range_robust": [0.05, 0.95], "k_stretch": 1.25}}


def model_of(scene):
    """SfmModel of a synthetic scene, and its number of pair instances"""
    from limap_amd import pointsfm, synthetic as syn
    n = scene.n_images
    R = np.stack([syn.quat_to_rot(q) for q in scene.qvec], 0)
    img_of_seg = np.repeat(np.arange(n), np.diff(scene.seg_off))
    seen = scene.gt_ids >= 0
    pairs = np.unique(np.stack([scene.gt_ids[seen], img_of_seg[seen]], 1), axis=0)  # (segment, image), sorted
    gids, counts = np.unique(pairs[:, 0], return_counts=True)
    # both endpoints of a segment share its track
    xyz = np.concatenate([scene.gt_lines[gids, :3], scene.gt_lines[gids, 3:]], 0)
    track_img = np.concatenate([pairs[:, 1], pairs[:, 1]]).astype(np.int32)
    track_off = np.zeros(2 * len(gids) + 1, np.int64)
    track_off[1:] = np.cumsum(np.concatenate([counts, counts]))
    slots = int(2 * (counts.astype(np.int64) * (counts - 1) // 2).sum())
    return pointsfm.SfmModel.from_arrays(scene.img_ids, R, scene.tvec, xyz, track_off, track_img), slots


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=5000)
    ap.add_argument("--segs", type=int, default=600)
    ap.add_argument("--neighbors", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from limap_amd import pointsfm, synthetic as syn
    scene = syn.make_scene(n_views=a.views, n_segs=a.segs, n_neighbors=a.neighbors, n_rooms=max(1, a.views // 100), seed=2)
    model, slots = model_of(scene)
    small, _ = model_of(syn.make_scene(n_views=8, n_segs=50, seed=1))
    pointsfm.compute_metainfos(CFG, small, a.neighbors)  # warm: code objects, the context
    rows = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        neighbors, ranges = pointsfm.compute_metainfos(CFG, model, a.neighbors)
        rows.append([1e3 * (time.perf_counter() - t0)] + pointsfm.timers().tolist())
    med = np.median(np.array(rows), 0).tolist()
    n_pairs = len(model.pair_records()[1])
    t0 = time.perf_counter()
    nb_host = model.GetMaxIoUImages(a.neighbors, CFG["min_triangulation_angle"], host=True, n_threads=a.threads)
    host_ms = 1e3 * (time.perf_counter() - t0)
    assert nb_host == neighbors, "host and device disagree"
    out = dict(views=a.views, points=len(model._arrays()[2]), pair_instances=slots, unique_pairs=n_pairs,
               n_neighbors=a.neighbors, neighbours_total=int(sum(len(v) for v in neighbors.values())),
               device=dict(call_ms=med[0], setup_upload_ms=med[1], device_stage_ms=med[2], download_ms=med[3],
                           k_sfm_pairs_ms=med[4], sort_ms=med[5], k_sfm_segments_ms=med[6], lists_select_ms=med[7],
                           segment_launches=med[8]),
               host=dict(threads=a.threads, neighbours_ms=host_ms),
               ranges=[np.asarray(ranges[0]).tolist(), np.asarray(ranges[1]).tolist()])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
