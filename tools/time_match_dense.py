#!/usr/bin/env python3
"""Times the dense kind of limap_amd.matching on one GPU, warm process, median of 7: 20 pairs of 500 x 500 lines per
native call, n_samples 21, warps and certainties of 864 x 864 texels (RoMa's output_res), once with the maps as torch
GPU tensors (read in place, as RoMa returns them) and once as host arrays (uploaded by the call).  Columns: wall, the
stages as lt_match_get_timers separates them (validation + upload, kernels, download, rows) and the three kernels by
HIP events (lt_match_dense_get_kernel_ms: k_dense_warp, k_dense_pairs, k_dense_select with its prefix sum).  Beside it,
labelled as CPU: limap's own wall time for one such pair from tests/golden/match_dense/ref_time.json (the CPU of the
machine that generated the goldens; that figure covers both one_to_many forms and the two directions once more).
Writes profiles/match_dense_timing.json."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from limap_amd import matching  # noqa: E402
import dense_cases as dc  # noqa: E402

N, S, RES, PAIRS = 500, 21, 864, 20
SHAPE = (480, 640)


def med(f, n=7):
    return np.median(np.array([f() for _ in range(n)]), axis=0)


def main():
    import torch
    rng = np.random.default_rng(0)
    images, maps = [], []
    for _ in range(PAIRS):
        a, b, w = dc.homography_pair(rng, N, N, SHAPE, SHAPE, (RES, RES), (RES, RES), holes=3)
        images += [matching._dense_image(a), matching._dense_image(b)]
        maps.append(w)
    pairs = [(2 * q, 2 * q + 1) for q in range(PAIRS)]
    opts = matching.DefaultDenseLineMatcherOptions
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "match_dense", "ref_time.json")))
    out = {"shape": {"pairs_per_call": PAIRS, "lines": [N, N], "n_samples": S, "warp": [RES, RES]},
           "reference_cpu": ref["pair_500_500_S21_warp864"], "cases": {}}
    for tag, m in (("maps_on_device", [[torch.from_numpy(x).cuda() for x in w] for w in maps]), ("maps_on_host", maps)):
        rows = [0]

        def once():
            t = time.perf_counter()
            rows[0] = len(matching._match_dense_flat(images, pairs, m, opts, 0.5, 0)[1])
            wall = (time.perf_counter() - t) * 1e3
            return np.concatenate([[wall], matching.timers(0), matching.dense_kernel_ms(0)])
        once()
        t = med(once)
        case = {"rows": rows[0], "wall_ms": t[0], "upload_ms": t[1], "kernels_ms": t[2], "download_ms": t[3],
                "rows_ms": t[4], "k_dense_warp_ms": t[5], "k_dense_pairs_ms": t[6], "k_dense_select_ms": t[7],
                "entries": PAIRS * N * N, "sample_line_tests": 2 * PAIRS * N * N * S}
        out["cases"][tag] = case
        print(tag, json.dumps(case), flush=True)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "match_dense_timing.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
