"""limap_amd.line2d on one GPU: a record of what SOLD2's line detection from junctions and heatmaps costs (DESIGN.md
section 23), nothing asserts a time.  A warm process, one untimed call first, the median of five:

  scene       detect_scene under the shipped configuration (every option on) on 1 and on --images synthetic heatmaps
              of --size x --size with --junctions junctions each: per-kernel times by HIP events, all kernels, the
              whole native call (staging, upload, kernels, download) and the whole Python call with its NumPy tail
  window      the junction-refinement kernel alone with its LDS heatmap window on (the default size) and off (every
              segment reads global memory), on a scene of one long and one of one short segment
  host path   the library's host path on one image, its segments checked equal to the device's
  reference   the reference's CPU time per image from tests/golden/sold2_detect/ref_time.json, where present

usage: python tools/time_sold2_detect.py [--images 32] [--size 512] [--junctions 300] [--out profiles/sold2_detect_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def median5(fn):
    fn()  # untimed
    runs = [fn() for _ in range(5)]
    return {k: float(np.median([r[k] for r in runs])) for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--junctions", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import make_sold2_detect_golden as gen
    from limap_amd import line2d

    module = line2d.LineSegmentDetectionModule(**line2d.SHIPPED_CFG)
    scenes = []
    for k in range(a.images):
        rng = np.random.default_rng(512 + k)
        junc, heat = gen.random_scene(rng, a.size, a.size, a.junctions // 5, a.junctions)
        scenes.append((np.ascontiguousarray(junc[:a.junctions]), heat))

    def run(n):
        def once():
            t0 = time.perf_counter()
            segs = line2d.detect_scene(module, [s[0] for s in scenes[:n]], [s[1] for s in scenes[:n]])
            ms = line2d.kernel_ms()
            ms["python_call"] = (time.perf_counter() - t0) * 1e3
            ms["segments"] = float(sum(len(s) for s in segs))
            return ms
        return median5(once)

    res = {"shape": {"size": a.size, "junctions": a.junctions, "config": "shipped (every option on)"},
           "ms_1_image": run(1), f"ms_{a.images}_images": run(a.images)}

    # the LDS window of the junction refinement, on and off, on a long and a short segment
    window = {}
    for name, line in (("long", [[5.3, 6.2], [a.size - 7.6, a.size - 9.1]]), ("short", [[200.4, 210.7], [214.2, 236.9]])):
        rng = np.random.default_rng(7)
        heat = gen.ridge_heatmap(rng, a.size, a.size, np.array([line]))
        junc = np.round(np.array(line)).astype(np.float32)
        for label, floats in (("lds", None), ("global", 0)):
            module.lds_window_floats = floats

            def once():
                segs = line2d.detect_scene(module, [junc] * 64, [heat] * 64)
                return {"refine_junctions_ms_64_segments": line2d.kernel_ms()["refine_junctions"],
                        "segments": float(sum(len(s) for s in segs))}
            window[f"{name}_{label}"] = median5(once)
    module.lds_window_floats = None
    res["refinement_window"] = window

    t0 = time.perf_counter()
    host = line2d.detect_scene(module, [scenes[0][0]], [scenes[0][1]], host=True)
    res["host_path_ms_1_image"] = (time.perf_counter() - t0) * 1e3
    dev = line2d.detect_scene(module, [scenes[0][0]], [scenes[0][1]])
    res["host_equals_device"] = bool(np.array_equal(host[0], dev[0]))
    ref = os.path.join(ROOT, "tests", "golden", "sold2_detect", "ref_time.json")
    if os.path.exists(ref):
        res["reference_cpu"] = json.load(open(ref)).get("image_512x512_300_junctions")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
