#!/usr/bin/env python3
"""Times the SOLD2 kind of limap_amd.matching on one GPU, warm process, median of 7: 100 images x 500 lines x 5 samples,
width 128, 20 neighbours, and one pair of 1000 x 1000 lines, each in the top-10 and in the mutual Needleman-Wunsch
form.  Columns: wall, the stages as lt_match_get_timers separates them (upload, kernels, download, rows), the line-score
kernel and the NW kernel by HIP events (lt_match_wunsch_get_kernel_ms), and the line-score kernel's flop rate against
the padded work it issues (8 x 8 slots per line pair) and against the necessary work (2 * dim * 25 N1 N2 per pair);
the mutual form scores every pair from both sides, and both figures count both passes.  Beside it: torch.matmul +
masking + pooling + torch.topk per image on the same GPU in the same process (top-k form only: there is no NW on the GPU
to compare with), and limap's own wall time per pair from tests/golden/match_wunsch/ref_time.json (CPU of the machine
that generated the goldens), scaled to the scene.
Writes profiles/match_wunsch_timing.json."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from limap_amd import matching  # noqa: E402
import wunsch_cases as wc  # noqa: E402

PEAK_F32_MFMA = 256 * 4 * 64 * 2.4e9  # CUs x SIMDs x flop/clk/SIMD x Hz
S, DIM, KC = 5, 128, 10


def med(f, n=7):
    return np.median(np.array([f() for _ in range(n)]), axis=0)


def native(parts, valids, pair_off, pair_nb, topk):
    def once():
        t = time.perf_counter()
        matching._match_flat(parts, pair_off, pair_nb, matching.SOLD2, topk, 0, False, valids, S, KC)
        wall = (time.perf_counter() - t) * 1e3
        return np.concatenate([[wall], matching.timers(0), matching.kernel_ms(0)])
    once()
    return med(once)


def torch_roof(parts, valids, pair_off, pair_nb):
    """the same line scores and top-10 with torch's own kernels, one batch per image"""
    import torch
    d = [torch.from_numpy(p).cuda() for p in parts]
    v = [torch.from_numpy(x.astype(bool)).cuda() for x in valids]

    def mean_of_counted(m):  # (b, n1, n2, S): the mean over the last axis of the entries that are not -1
        keep = m != -1
        return (m * keep).sum(-1) / keep.sum(-1)

    def once():
        torch.cuda.synchronize()
        t = time.perf_counter()
        for m in range(len(d)):
            nb = pair_nb[pair_off[m]:pair_off[m + 1]]
            if not len(nb):
                continue
            p = torch.matmul(d[m], torch.stack([d[j] for j in nb]).transpose(1, 2))  # (b, S n1, S n2)
            ok = v[m].reshape(1, -1, 1) & torch.stack([v[j].reshape(-1) for j in nb])[:, None, :]
            p = torch.where(ok, p, torch.full_like(p, -1.0))
            b, n1, n2 = p.shape[0], v[m].shape[0], p.shape[2] // S
            p = p.reshape(b, n1, S, n2, S)
            score = 0.5 * (mean_of_counted(p.amax(4).transpose(2, 3)) + mean_of_counted(p.amax(2)))
            torch.topk(score, min(10, n2), dim=2)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3
    once()
    return float(med(once))


def main():
    rng = np.random.default_rng(0)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "match_wunsch", "ref_time.json")))
    out = {"peak_f32_mfma_flops": PEAK_F32_MFMA, "reference_cpu": {k: v for k, v in ref.items() if k != "fixtures"},
           "cases": {}}
    for name, n, m, nnb in (("scene_100x500", 100, 500, 20), ("pair_1000", 2, 1000, 1)):
        infos = [wc.rand_descinfo(rng, m, S, DIM) for _ in range(n)]
        parts = [np.ascontiguousarray(d[0].T) for d in infos]
        valids = [d[1].astype(np.uint8) for d in infos]
        pair_off = np.arange(n + 1) * nnb if n > 2 else np.array([0, 1, 1])
        pair_nb = np.concatenate([(i + 1 + np.arange(nnb)) % n for i in range(n)]) if n > 2 else np.array([1])
        roof = torch_roof(parts, valids, pair_off, pair_nb)
        for topk, tag in ((10, "top10"), (0, "mutual")):
            t = native(parts, valids, pair_off, pair_nb, topk)
            passes = 2 if topk == 0 else 1  # the mutual form scores every pair from both sides
            necessary = 2.0 * DIM * 25 * m * m * len(pair_nb) * passes  # (per pass, like the padded work)
            padded = 2.0 * DIM * 64 * m * m * len(pair_nb) * passes
            k1 = t[5] * 1e-3
            ref_pair = ref[f"pair_{m}_{tag}"]["seconds_per_pair"]
            case = {"pairs": int(len(pair_nb)), "wall_ms": t[0], "upload_ms": t[1], "kernels_ms": t[2],
                    "download_ms": t[3], "rows_ms": t[4], "k_wunsch_topk_ms": t[5], "k_wunsch_nw_ms": t[6],
                    "padded_flop": padded, "necessary_flop": necessary,
                    "k_wunsch_topk_tflops_padded": padded / k1 / 1e12,
                    "k_wunsch_topk_tflops_necessary": necessary / k1 / 1e12,
                    "share_of_f32_mfma_peak_padded": padded / k1 / PEAK_F32_MFMA,
                    "torch_matmul_pool_topk_ms": roof if topk else None,
                    "reference_cpu_ms": ref_pair * 1e3 * len(pair_nb)}
            out["cases"][f"{name}_{tag}"] = case
            print(f"{name}_{tag}", json.dumps(case), flush=True)
    dst = os.path.join(ROOT, "profiles", "match_wunsch_timing.json")
    if len(sys.argv) > 1:
        dst = sys.argv[1]
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
