"""Writes tests/golden/match/*.npz: descriptor inputs and the rows limap's own matchers return for them, plus
match_ref_time.json (the reference's wall time per fixture on the generating machine, CPU).

Run on a machine that has the limap source tree (LIMAP_SRC, default /root/reference/src); the two matcher modules are
loaded from there at generation time only, with stand-ins for the imports they do not need here.  Nothing of the
reference is stored: only inputs, result rows and times.

The analysis half of this file (exact_scores, bounds, decided_rows, ...) is imported by tests/test_match_host.py: it
states when a ranking is DECIDED whatever the summation order of an FP32 dot product.
"""
import importlib.util
import json
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "match")
U = 2.0 ** -24
MAX_UNDECIDED = 0.10


# ---------------------------------------------------------------------------------------------------------------------
# analysis: exact scores, error bounds, decided rankings
def gamma(n):
    return n * U / (1.0 - n * U)


def exact_scores(kind, d1, d2):
    """float64 scores E and the bound B on |any FP32 evaluation - E| (M1, M2).  kind "l2d2": d (M, K); "endpoints":
    d (K, 2 M).  A dot product of K FP32 products summed in any order errs by at most gamma_K sum |a_k b_k|; the line
    score of the endpoints matcher adds one rounding (the sum of two dot products: gamma_{K+1}), the maximum of two
    perturbed values moves by at most the larger perturbation, and the halving is exact."""
    if kind == "l2d2":
        a, b = np.asarray(d1, np.float64), np.asarray(d2, np.float64)
        K = a.shape[1] if a.size else 1
        return a @ b.T, gamma(K) * (np.abs(a) @ np.abs(b).T)
    a, b = np.asarray(d1, np.float64).T, np.asarray(d2, np.float64).T  # (2 M, K)
    K = a.shape[1]
    S, A = a @ b.T, np.abs(a) @ np.abs(b).T
    m1, m2 = a.shape[0] // 2, b.shape[0] // 2
    S, A = S.reshape(m1, 2, m2, 2), A.reshape(m1, 2, m2, 2)
    E = 0.5 * np.maximum(S[:, 0, :, 0] + S[:, 1, :, 1], S[:, 0, :, 1] + S[:, 1, :, 0])
    B = 0.5 * gamma(K + 1) * np.maximum(A[:, 0, :, 0] + A[:, 1, :, 1], A[:, 0, :, 1] + A[:, 1, :, 0])
    return E, B


def row_analysis(E, B, k):
    """per row: order (columns by exact score, best first), decided (its best k columns are each separated from every
    other column by more than the two bounds: any evaluation ranks them the same), mandatory (columns fewer than k
    others can possibly outrank: every evaluation returns them)"""
    m1, m2 = E.shape
    k = min(k, m2)
    order = np.argsort(-E, axis=1, kind="stable")
    decided = np.ones(m1, bool)
    mandatory = []
    for i in range(m1):
        e, b = E[i], B[i]
        gap = e[:, None] - e[None, :]            # gap[c, c'] = E_c - E_c'
        tol = b[:, None] + b[None, :]
        beats = gap > tol                         # c is above c' in every evaluation
        top = order[i, :k]
        sep = beats[top, :] | beats[:, top].T     # (k, m2): decided either way
        sep[np.arange(k), top] = True
        decided[i] = bool(sep.all())
        not_below = (~beats).sum(1) - 1           # others that c does not certainly beat
        mandatory.append(np.nonzero(not_below < k)[0])
    return order, decided, mandatory


def forbidden_order(E, B, i, cols):
    """True when two of `cols` (a returned ranking of row i) stand in an order every evaluation contradicts"""
    e, b = E[i, cols], B[i, cols]
    later_better = (e[None, :] - e[:, None]) > (b[None, :] + b[:, None])  # [p, q]: q certainly above p
    return bool(np.triu(later_better, 1).any())


def undecided_share(kind, descs, pairs, topk):
    rows = bad = 0
    for a, b in pairs:
        E, B = exact_scores(kind, descs[a], descs[b])
        if E.size == 0:
            continue
        if topk == 0:
            dec = mutual_decided(E, B)
        else:
            dec = row_analysis(E, B, topk)[1]
        rows += len(dec)
        bad += int((~dec).sum())
    return (bad / rows) if rows else 0.0


def mutual_decided(E, B):
    """per row i: its arg-max column j is decided, and so is the arg-max row of column j"""
    _, drow, _ = row_analysis(E, B, 1)
    _, dcol, _ = row_analysis(E.T.copy(), B.T.copy(), 1)
    return drow & dcol[np.argmax(E, axis=1)]


def load_fixture(path):
    z = np.load(path, allow_pickle=False)
    kind, topk, n = str(z["kind"]), int(z["topk"]), int(z["n_img"])
    descs = [z[f"desc_{m}"] for m in range(n)]
    pairs = [tuple(int(x) for x in p) for p in z["pairs"]]
    ref = [z[f"ref_{p}"] for p in range(len(pairs))] if int(z["has_ref"]) else None
    return kind, topk, descs, pairs, ref


# ---------------------------------------------------------------------------------------------------------------------
# generation
def _load_reference(src):
    def stub(name, **attrs):
        if name in sys.modules:
            return
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    for pkg in ("limap", "limap.util", "limap.point2d", "limap.line2d", "limap.line2d.L2D2", "limap.line2d.endpoints"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(src, *pkg.split("."))]
        sys.modules[pkg] = m
    stub("limap.util.io")
    stub("limap.point2d.superglue", SuperGlue=object)
    for name in ("joblib", "tqdm"):
        try:
            __import__(name)
        except ImportError:
            stub(name, tqdm=lambda x: x)

    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(src, "limap", *rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    load("limap.line2d.base_matcher", ("line2d", "base_matcher.py"))
    l2d2 = load("limap.line2d.L2D2.matcher", ("line2d", "L2D2", "matcher.py"))
    ep = load("limap.line2d.endpoints.matcher", ("line2d", "endpoints", "matcher.py"))
    return l2d2.L2D2Matcher, ep.NNEndpointsMatcher


def _unit(rng, shape, axis):
    d = rng.standard_normal(shape)
    return (d / np.linalg.norm(d, axis=axis, keepdims=True)).astype(np.float32)


def main():
    src = os.environ.get("LIMAP_SRC", "/root/reference/src")
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from limap_amd import synthetic as syn
    L2D2, NNE = _load_reference(src)
    rng = np.random.default_rng(20240617)
    os.makedirs(OUT, exist_ok=True)

    def l2(ms, dim=128):
        return [_unit(rng, (m, dim), 1) if m else np.zeros((0, dim), np.float32) for m in ms]

    def ep(ms, dim=256):
        return [_unit(rng, (dim, 2 * m), 0) for m in ms]

    allp = lambda n: [(a, b) for a in range(n) for b in range(n) if a != b]
    fixtures = {
        "l2d2_top10": ("l2d2", 10, l2([150, 200, 97]), allp(3)),
        "l2d2_mutual": ("l2d2", 0, l2([120, 90, 131]), allp(3)),
        "l2d2_top1": ("l2d2", 1, l2([64, 65]), allp(2)),
        "l2d2_empty": ("l2d2", 10, l2([0, 50]), [(0, 1), (1, 0)]),
        "l2d2_one_vs_many": ("l2d2", 10, l2([1, 300]), [(0, 1)]),
        "l2d2_ragged": ("l2d2", 10, l2([33, 10, 63, 129, 12]), allp(5)),  # (limap's L2D2 top-k needs M2 >= topk)
        "endpoints_top10": ("endpoints", 10, ep([80, 100, 61]), allp(3)),
        "endpoints_m2_below_topk": ("endpoints", 10, ep([40, 4]), [(0, 1), (1, 0)]),
    }
    sc = syn.make_scene(n_views=5, n_segs=50, n_neighbors=3, seed=11)
    pairs = [(k, int(np.searchsorted(sc.img_ids, j))) for k, i in enumerate(sc.img_ids) for j in sc.neighbors[int(i)]]
    for kind, key in (("l2d2", "line_descriptors"), ("endpoints", "endpoints_desc")):
        di = syn.make_descriptors(sc, kind, noise=0.05, seed=5)
        fixtures[f"{kind}_synthetic"] = (kind, 10, [di[int(i)][key] for i in sc.img_ids], pairs)

    times = {"machine": "generator's CPU (no GPU), limap's matchers as they are, torch on the CPU for the endpoints",
             "fixtures": {}}
    for name, (kind, topk, descs, prs) in fixtures.items():
        share = undecided_share(kind, descs, prs, topk)
        assert share <= MAX_UNDECIDED, f"{name}: {share:.1%} of the rows are undecided"
        ref = []
        t0 = time.perf_counter()
        for a, b in prs:
            if kind == "l2d2":
                obj = types.SimpleNamespace(topk=topk)
                d1, d2 = {"line_descriptors": descs[a]}, {"line_descriptors": descs[b]}
                if topk == 0:
                    r = L2D2.match_segs_with_descinfo(obj, d1, d2)
                else:
                    r = L2D2.match_segs_with_descinfo_topk(obj, d1, d2, topk=topk)
            else:
                obj = types.SimpleNamespace(device="cpu", topk=topk)
                r = NNE.match_segs_with_descinfo_topk(obj, {"endpoints_desc": descs[a]}, {"endpoints_desc": descs[b]},
                                                      topk=topk)
            ref.append(np.asarray(r).reshape(-1, 2).astype(np.int32))
        dt = time.perf_counter() - t0
        times["fixtures"][name] = {"pairs": len(prs), "seconds": dt, "undecided_share": share}
        arrays = {"kind": np.array(kind), "topk": np.array(topk), "n_img": np.array(len(descs)),
                  "pairs": np.array(prs, np.int32).reshape(-1, 2), "has_ref": np.array(1)}
        arrays.update({f"desc_{m}": d for m, d in enumerate(descs)})
        arrays.update({f"ref_{p}": r for p, r in enumerate(ref)})
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrays)
        print(f"{name}: {len(prs)} pairs, {sum(len(r) for r in ref)} rows, undecided {share:.2%}, reference {dt * 1e3:.1f} ms")

    # the headline shape, timed only (nothing stored but the time): 20 pairs of 500 x 500, scaled to 2 000 pairs
    for kind, mk in (("l2d2", lambda: l2([500, 500])), ("endpoints", lambda: ep([500, 500]))):
        d = mk()
        t0 = time.perf_counter()
        for _ in range(20):
            if kind == "l2d2":
                L2D2.match_segs_with_descinfo_topk(None, {"line_descriptors": d[0]}, {"line_descriptors": d[1]}, topk=10)
            else:
                NNE.match_segs_with_descinfo_topk(types.SimpleNamespace(device="cpu"), {"endpoints_desc": d[0]},
                                                  {"endpoints_desc": d[1]}, topk=10)
        dt = (time.perf_counter() - t0) / 20
        times[f"headline_{kind}"] = {"seconds_per_pair_500x500_top10": dt, "seconds_2000_pairs": dt * 2000,
                                     "note": "matching only: no descriptor file reads, no result file writes"}
    d = l2([1000, 1000])
    t0 = time.perf_counter()
    L2D2.match_segs_with_descinfo_topk(None, {"line_descriptors": d[0]}, {"line_descriptors": d[1]}, topk=10)
    times["pair_1000_l2d2"] = {"seconds": time.perf_counter() - t0}
    d = ep([1000, 1000])
    t0 = time.perf_counter()
    NNE.match_segs_with_descinfo_topk(types.SimpleNamespace(device="cpu"), {"endpoints_desc": d[0]},
                                      {"endpoints_desc": d[1]}, topk=10)
    times["pair_1000_endpoints"] = {"seconds": time.perf_counter() - t0}
    with open(os.path.join(OUT, "match_ref_time.json"), "w") as f:
        json.dump(times, f, indent=1)


if __name__ == "__main__":
    main()
