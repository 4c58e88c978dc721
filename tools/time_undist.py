"""limap_amd.undistortion on one GPU: a record of what the step costs, nothing asserts a time.
A warm process, one untimed call first, the median of five:

  warp        k_undist_warp by HIP events on N device-resident W x H RGB images under one OPENCV camera; bytes read
              once plus bytes written once, divided by the time; beside it a 16-bytes-per-lane device copy kernel over
              the same byte count, timed in the same process (the yardstick)
  whole call  undistort_images from host arrays: upload, warp, download
  host path   the library's host path on --threads threads, its bytes checked equal to the device's
  points      k_undist_points on --points points

usage: python tools/time_undist.py [--images 100] [--width 1600] [--height 1200] [--points 1000000] [--threads 16]
                                   [--out profiles/undist_timing.json]
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


def median5(fn):
    fn()  # untimed
    return float(np.median([fn() for _ in range(5)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from limap_amd import undistortion as und
    w, h, n = a.width, a.height, a.images
    f = 0.75 * w
    cam = und.Camera("OPENCV", [f, f, w / 2 + 0.3, h / 2 - 0.4, -0.12, 0.03, 0.001, -0.0005], cam_id=1, hw=(h, w))
    target = und.undistort_camera(cam)
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ctx = und._context(0)

    # ---- the warp on device-resident images ----
    tens = [torch.from_numpy(img).cuda() for _ in range(n)]
    items = [(cam, target, t) for t in tens]
    outs = []

    def warp_ms():
        outs[:] = und._warp_batch(items)
        return und.timers()[1]

    warp = median5(warp_ms)
    moved = n * (h * w * 3 + target.h() * target.w() * 3)
    dev_first = outs[0].cpu().numpy()
    del outs[:], tens, items
    torch.cuda.empty_cache()

    def copy_ms():
        ms = C.c_double(0.0)
        ctx.chk(ctx.L.lt_undist_copy_yardstick(ctx.h, moved // 2, C.byref(ms)))  # reads moved / 2, writes moved / 2
        return ms.value

    copy = median5(copy_ms)

    # ---- the whole call from host arrays ----
    cameras, images = {i: cam for i in range(n)}, {i: img for i in range(n)}
    res = {}

    def call_ms():
        t0 = time.perf_counter()
        res["out"] = und.undistort_images(cameras, images, max_chunk_bytes=1 << 34)[1]
        return 1e3 * (time.perf_counter() - t0)

    call = median5(call_ms)
    assert np.array_equal(res["out"][0], dev_first), "host arrays and device tensors disagree"

    # ---- the host path ----
    t0 = time.perf_counter()
    host_out = und._warp_batch([(cam, target, img)] * n, host=True, n_threads=a.threads)
    host_ms = 1e3 * (time.perf_counter() - t0)
    assert all(np.array_equal(host_out[i], res["out"][i]) for i in range(n)), "host and device disagree"

    # ---- points ----
    pts = rng.uniform([0.0, 0.0], [w, h], (a.points, 2))

    def points_ms():
        res["pts"] = und._points_raw([cam, target], pts, 0, 1)
        return und.timers()[1]

    points = median5(points_ms)
    t0 = time.perf_counter()
    host_pts = und._points_raw([cam, target], pts, 0, 1, host=True, n_threads=a.threads)
    host_pts_ms = 1e3 * (time.perf_counter() - t0)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(res["pts"], host_pts))

    out = dict(images=n, width=w, height=h, channels=3, target=[target.w(), target.h()], bytes_moved=moved,
               warp=dict(k_undist_warp_ms=warp, tb_per_s=moved / warp / 1e9, copy16_ms=copy, copy16_tb_per_s=moved / copy / 1e9,
                         fraction_of_copy=copy / warp),
               whole_call_from_host_ms=call,
               host_path=dict(threads=a.threads, warp_ms=host_ms, points_ms=host_pts_ms),
               points=dict(n=a.points, k_undist_points_ms=points, mean_iterations=float(res["pts"][2].mean())))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(out, fo, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
