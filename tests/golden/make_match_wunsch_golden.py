"""Writes tests/golden/match_wunsch/*.npz: SOLD2 descinfos [desc (dim, S N), valid (N, S)] and what limap's own
WunschLineMatcher returns for them -- the top-k rows and the mutual Needleman-Wunsch matches -- plus ref_time.json (the
reference's wall time on the generating machine, CPU).

Run on a machine that has the limap source tree (LIMAP_SRC, default /root/reference/src); line2d/SOLD2/model/
line_matching.py is loaded from there at generation time only, with stand-ins for its parent packages and for
..misc.geometry_utils.  Nothing of the reference is stored: only inputs, result rows and times.

The analysis half of this file is imported by tests/test_match_wunsch_host.py: it states when a ranking of line scores,
and when a Needleman-Wunsch match, is DECIDED whatever the summation order of the FP32 dot products (DESIGN section 17,
"SOLD2").
"""
import importlib.util
import json
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "match_wunsch")
_spec = importlib.util.spec_from_file_location("make_match_golden", os.path.join(HERE, "make_match_golden.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)
U, gamma, MAX_UNDECIDED = base.U, base.gamma, base.MAX_UNDECIDED
GAP = float(np.float32(0.1))


# ---------------------------------------------------------------------------------------------------------------------
# analysis
def exact_point_scores(d1, d2, S):
    """float64 point scores P (N1, S, N2, S) with -1 where a sample is masked, and the bound Bp on |any FP32 evaluation
    - P|: a dot product of K FP32 products summed in any order errs by at most gamma_K sum |a_k b_k| (0 where masked:
    every evaluation writes the same -1)"""
    a, b = np.asarray(d1[0], np.float64).T, np.asarray(d2[0], np.float64).T  # (S N, K)
    v1, v2 = np.asarray(d1[1], bool), np.asarray(d2[1], bool)
    n1, n2, K = v1.shape[0], v2.shape[0], a.shape[1]
    ok = v1.reshape(-1)[:, None] & v2.reshape(-1)[None, :]
    P = np.where(ok, a @ b.T, -1.0).reshape(n1, S, n2, S)
    Bp = np.where(ok, gamma(K) * (np.abs(a) @ np.abs(b).T), 0.0).reshape(n1, S, n2, S)
    return P, Bp


def _pooled(P, Bp, axis):
    """mean over the other sample axis of the maxima along `axis` that count, and its bound: a maximum of perturbed
    values moves by at most the largest bound among the terms that can win it; the mean of at most 8 such maxima adds
    the roundings of its sum and its division (gamma_9 covers any order of either evaluation)"""
    m = P.max(axis)
    can_win = (P + Bp) >= np.expand_dims((P - Bp).max(axis), axis)
    e = np.where(can_win, Bp, 0.0).max(axis)
    counts = m != -1.0
    cnt = counts.sum(1 if axis == 3 else 2)
    ax = 1 if axis == 3 else 2  # the sample axis that is left: (N1, S, N2) -> 1, (N1, N2, S) -> 2
    cnt = np.maximum(cnt, 1)
    mean = (m * counts).sum(ax) / cnt
    mean_abs = (np.abs(m) * counts).sum(ax) / cnt
    mean_e = (e * counts).sum(ax) / cnt
    return mean, mean_e + gamma(9) * (mean_abs + mean_e)


def exact_line_scores(P, Bp):
    """float64 line scores E (N1, N2) and the bound B on |any FP32 evaluation - E|"""
    l1, b1 = _pooled(P, Bp, 3)  # max over t: (N1, S, N2), mean over s
    l2, b2 = _pooled(P, Bp, 1)  # max over s: (N1, N2, S), mean over t
    E = 0.5 * (l1 + l2)
    return E, 0.5 * (b1 + b2) * (1.0 + U) + U * np.abs(E)


def nw_value(w):
    """the recurrence of needleman_wunsch on one block of gap-corrected scores, float64"""
    n, m = w.shape
    g = np.zeros((n + 1, m + 1))
    for i in range(n):
        for j in range(m):
            g[i + 1, j + 1] = max(max(g[i + 1, j], g[i, j + 1]), g[i, j] + w[i, j])
    return g[n, m]


def nw_match_analysis(P, Bp, E, B, kc):
    """per line i of image 1: (match, decided).  The match is the candidate with the best exact NW value over both
    orientations.  Decided: the candidate SET is decided (every candidate's line score leads every other line's by more
    than the two bounds) and the best NW value leads every other candidate line's values by more than the two NW bounds.
    An NW value is a maximum over alignments of sums of at most 2 S - 1 gap-corrected scores, each within Bp plus the
    FP32 rounding of the subtraction of its FP32 evaluation; the FP64 additions are far below that."""
    n1, S, n2, _ = P.shape
    kc = min(kc, n2)
    match = np.zeros(n1, np.int64)
    decided = np.zeros(n1, bool)
    for i in range(n1):
        order = np.argsort(-E[i], kind="stable")
        top, rest = order[:kc], order[kc:]
        set_ok = (len(rest) == 0) or ((E[i, top] - B[i, top]).min() > (E[i, rest] + B[i, rest]).max())
        val = np.zeros(kc)
        bnd = np.zeros(kc)
        for c, j in enumerate(top):
            w = P[i, :, j, :] - GAP
            val[c] = max(nw_value(w), nw_value(w[:, ::-1]))
            bnd[c] = (2 * S - 1) * float((Bp[i, :, j, :] + 2.0 * U * (np.abs(P[i, :, j, :]) + GAP)).max())
        c1 = int(np.argmax(val))
        match[i] = top[c1]
        others = np.arange(kc) != c1
        lead = (not others.any()) or bool(((val[c1] - val[others]) > (bnd[c1] + bnd[others])).all())
        decided[i] = set_ok and lead
    return match, decided


def mutual_analysis(d1, d2, S, kc):
    """-> (match of every line of image 1, or -1 where the cross check drops it; decided per line of image 1)"""
    P, Bp = exact_point_scores(d1, d2, S)
    E, B = exact_line_scores(P, Bp)
    f, fd = nw_match_analysis(P, Bp, E, B, kc)
    Pt, Bpt = P.transpose(2, 3, 0, 1), Bp.transpose(2, 3, 0, 1)
    b, bd = nw_match_analysis(Pt, Bpt, E.T, B.T, kc)
    keep = b[f] == np.arange(len(f))
    return np.where(keep, f, -1), fd & bd[f]


def undecided_share(descs, pairs, topk, S, kc):
    rows = bad = 0
    for a, b in pairs:
        if descs[a][1].shape[0] == 0 or descs[b][1].shape[0] == 0:
            continue
        if topk == 0:
            dec = mutual_analysis(descs[a], descs[b], S, kc)[1]
        else:
            dec = base.row_analysis(*exact_line_scores(*exact_point_scores(descs[a], descs[b], S)), topk)[1]
        rows += len(dec)
        bad += int((~dec).sum())
    return (bad / rows) if rows else 0.0


def load_fixture(path):
    """-> topk, num_samples, top_k_candidates, descinfos, pairs, reference rows per pair"""
    z = np.load(path, allow_pickle=False)
    n = int(z["n_img"])
    descs = [[z[f"desc_{m}"], z[f"valid_{m}"]] for m in range(n)]
    pairs = [tuple(int(x) for x in p) for p in z["pairs"]]
    ref = [z[f"ref_{p}"] for p in range(len(pairs))]
    return int(z["topk"]), int(z["num_samples"]), int(z["top_k_candidates"]), descs, pairs, ref


# ---------------------------------------------------------------------------------------------------------------------
# generation
def _load_reference(src):
    root = os.path.join(src, "limap")
    for pkg in ("limap", "limap.line2d", "limap.line2d.SOLD2", "limap.line2d.SOLD2.model", "limap.line2d.SOLD2.misc"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(root, *pkg.split(".")[1:])]
        sys.modules[pkg] = m
    g = types.ModuleType("limap.line2d.SOLD2.misc.geometry_utils")
    g.keypoints_to_grid = None  # (compute_descriptors only: not run here)
    sys.modules[g.__name__] = g
    name = "limap.line2d.SOLD2.model.line_matching"
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "line2d", "SOLD2", "model", "line_matching.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod.WunschLineMatcher


def reference_rows(matcher, d1, d2, topk):
    """what SOLD2LineDetector.match_segs_with_descinfo / _topk make of the matcher's answer, as (n, 2) int32"""
    import torch
    if d1[1].shape[0] == 0 or d2[1].shape[0] == 0:
        return np.zeros((0, 2), np.int32)
    t1, t2 = [torch.tensor(d1[0], dtype=torch.float), d1[1]], [torch.tensor(d2[0], dtype=torch.float), d2[1]]
    if topk == 0:
        m = matcher.compute_matches(t1, t2)
        keep = m != -1
        return np.stack([np.arange(len(m))[keep], m[keep]], 1).astype(np.int32)
    m = matcher.compute_matches_topk_gpu(t1, t2, topk=topk)
    n, k = m.shape
    return np.concatenate([np.stack([np.arange(n), m[:, c]], 1) for c in range(k)], 0).astype(np.int32)


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    import wunsch_cases as wc
    Wunsch = _load_reference(os.environ.get("LIMAP_SRC", "/root/reference/src"))
    rng = np.random.default_rng(20240923)
    os.makedirs(OUT, exist_ok=True)
    S, KC = 5, 10
    mk = lambda ns: [wc.rand_descinfo(rng, n, S, 128) for n in ns]
    allp = lambda n: [(a, b) for a in range(n) for b in range(n) if a != b]
    fixtures = {  # name: (topk, descinfos, pairs)
        "top10_33_47": (10, mk([33, 47]), allp(2)),
        "top10_64_65": (10, mk([64, 65]), allp(2)),
        "top10_130_97": (10, mk([130, 97]), allp(2)),
        "top10_40_9": (10, mk([40, 9]), allp(2)),  # N2 < topk one way
        "top1_17_16": (1, mk([17, 16]), allp(2)),
        "top10_empty": (10, mk([0, 20]), allp(2)),
        "mutual_33_47_64": (0, mk([33, 47, 64]), allp(3)),
        "mutual_130_97": (0, mk([130, 97]), allp(2)),
        "mutual_40_9": (0, mk([40, 9]), allp(2)),  # N2 < top_k_candidates one way
        "mutual_empty": (0, mk([0, 20]), allp(2)),
    }
    times = {"machine": "generator's CPU (no GPU), limap's WunschLineMatcher as it is, torch on the CPU", "fixtures": {}}
    matcher = Wunsch(cross_check=True, num_samples=S, top_k_candidates=KC)
    for name, (topk, descs, prs) in fixtures.items():
        share = undecided_share(descs, prs, topk, S, KC)
        assert share <= MAX_UNDECIDED, f"{name}: {share:.1%} of the rows are undecided"
        t0 = time.perf_counter()
        ref = [reference_rows(matcher, descs[a], descs[b], topk) for a, b in prs]
        dt = time.perf_counter() - t0
        times["fixtures"][name] = {"pairs": len(prs), "seconds": dt, "undecided_share": share}
        arrays = {"topk": np.array(topk), "num_samples": np.array(S), "top_k_candidates": np.array(KC),
                  "n_img": np.array(len(descs)), "pairs": np.array(prs, np.int32).reshape(-1, 2)}
        arrays.update({f"desc_{m}": d[0] for m, d in enumerate(descs)})
        arrays.update({f"valid_{m}": d[1] for m, d in enumerate(descs)})
        arrays.update({f"ref_{p}": r for p, r in enumerate(ref)})
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrays)
        print(f"{name}: {len(prs)} pairs, {sum(len(r) for r in ref)} rows, undecided {share:.2%}, reference {dt * 1e3:.1f} ms")

    # the headline shapes, timed only: pairs of 500 x 500 lines (scaled to 2 000 pairs by the reader) and 1000 x 1000
    for n, reps in ((500, 5), (1000, 1)):
        d = mk([n, n])
        for topk, tag in ((10, "top10"), (0, "mutual")):
            t0 = time.perf_counter()
            for _ in range(reps):
                reference_rows(matcher, d[0], d[1], topk)
            times[f"pair_{n}_{tag}"] = {"seconds_per_pair": (time.perf_counter() - t0) / reps,
                                        "note": "matching only: no descinfo reads, no result file writes"}
    with open(os.path.join(OUT, "ref_time.json"), "w") as f:
        json.dump(times, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
