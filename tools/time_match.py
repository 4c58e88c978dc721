#!/usr/bin/env python3
"""Times limap_amd.matching on one GPU, warm process, median of 7, stages as lt_match_get_timers separates them (upload,
kernels, download, rows): L2D2 and endpoints at 100 images x 500 lines x 20 neighbours x top-10, and one pair of
1000 x 1000.  Beside it: torch.matmul + torch.topk on the same GPU in the same process (a roof for the contraction,
batched per image), and limap's own wall time from tests/golden/match/match_ref_time.json (CPU of the machine that
generated the goldens).  Writes profiles/match_timing.json."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from limap_amd import matching  # noqa: E402

PEAK_F32_MFMA = 256 * 4 * 64 * 2.4e9  # CUs x SIMDs x flop/clk/SIMD x Hz


def med(f, n=7):
    out = []
    for _ in range(n):
        out.append(f())
    return np.median(np.array(out), axis=0)


def native(parts, pair_off, pair_nb, kind):
    def once():
        t = time.perf_counter()
        matching._match_flat(parts, pair_off, pair_nb, kind, 10, 0)
        wall = (time.perf_counter() - t) * 1e3
        return np.concatenate([[wall], matching.timers(0)])
    once()
    return med(once)


def torch_roof(parts, pair_off, pair_nb, kind):
    import torch
    d = [torch.from_numpy(p).cuda() for p in parts]

    def once():
        torch.cuda.synchronize()
        t = time.perf_counter()
        for m in range(len(d)):
            nb = pair_nb[pair_off[m]:pair_off[m + 1]]
            if not len(nb):
                continue
            s = torch.matmul(d[m], torch.stack([d[j] for j in nb]).transpose(1, 2))
            if kind == 1:
                b, r, c = s.shape
                s = s.reshape(b, r // 2, 2, c // 2, 2)
                s = 0.5 * torch.maximum(s[:, :, 0, :, 0] + s[:, :, 1, :, 1], s[:, :, 0, :, 1] + s[:, :, 1, :, 0])
            torch.topk(s, 10, dim=2)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3
    once()
    return float(med(once))


def main():
    rng = np.random.default_rng(0)
    out = {"peak_f32_mfma_flops": PEAK_F32_MFMA, "cases": {}}
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "match", "match_ref_time.json")))
    out["reference_cpu"] = {k: v for k, v in ref.items() if k != "fixtures"}
    for name, kind, dim, n, m, nnb in (("l2d2_scene", 0, 128, 100, 500, 20), ("endpoints_scene", 1, 256, 100, 500, 20),
                                       ("l2d2_pair_1000", 0, 128, 2, 1000, 1), ("endpoints_pair_1000", 1, 256, 2, 1000, 1)):
        per = 2 if kind else 1
        parts = [rng.standard_normal((m * per, dim)).astype(np.float32) for _ in range(n)]
        for p in parts:
            p /= np.linalg.norm(p, axis=1, keepdims=True)
        pair_off = np.arange(n + 1) * nnb if n > 2 else np.array([0, 1, 1])
        pair_nb = np.concatenate([(i + 1 + np.arange(nnb)) % n for i in range(n)]) if n > 2 else np.array([1])
        t = native(parts, pair_off, pair_nb, kind)
        flop = 2.0 * len(pair_nb) * (m * per) ** 2 * dim
        case = {"pairs": int(len(pair_nb)), "flop": flop, "wall_ms": t[0], "upload_ms": t[1], "kernels_ms": t[2],
                "download_ms": t[3], "rows_ms": t[4], "kernel_flops": flop / (t[2] * 1e-3),
                "share_of_f32_mfma_peak": flop / (t[2] * 1e-3) / PEAK_F32_MFMA,
                "torch_matmul_topk_ms": torch_roof(parts, pair_off, pair_nb, kind)}
        out["cases"][name] = case
        print(name, json.dumps(case), flush=True)
    dst = os.path.join(ROOT, "profiles", "match_timing.json")
    if len(sys.argv) > 1:
        dst = sys.argv[1]
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
