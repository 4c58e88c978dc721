"""Golden files of limap.structures.PL_Bipartite2d, written by THE REFERENCE'S OWN CODE: bpt_ref_driver.cpp (next to
this file) is compiled into a temporary directory against the objects `make -C oracle ref` builds
(oracle/_ref/obj/**/*.o: structures/pl_bipartite{,_base}.o, base/linebase.o, base/graph.o, util/kd_tree.o) and the
stand-in headers of oracle/ref_shim, and called through ctypes.  Run where the reference sources exist (their path is
the REF of oracle/Makefile), like make_eval_golden.py; tests/test_bpt_host.py and tests/test_gpu_bpt.py read the outputs.

  (all under tests/golden/bpt/)
  bpt_<name>.npz     inputs (lines, points with their point3D ids and ids, keypoints, the three thresholds) and the
                     reference's outputs: per point the CSR of its line ids after add_keypoints_with_point3D_ids, and
                     the junctions of compute_intersection_with_points on a bipartite of the lines alone (point ids,
                     coordinates, CSR of line ids).  intersect() and the parents array are private to the reference's
                     class, so the intermediate lists are not recorded; tests/bpt_oracle.py restates them.
  bpt_ref_time.json  the reference's wall times on the inputs of tools/time_bipartite.py, and its thread count (1)

The generator asserts, for every merged junction of every fixture, that the kd-tree's nearest distance equals the
brute-force minimum (tests/bpt_oracle.py): the contract is the exact minimum.

usage: python tests/golden/make_bpt_golden.py [--no-timing] [--timing-only]
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(HERE, "bpt")

import bpt_oracle as bo  # noqa: E402
import time_bipartite as tb  # noqa: E402


def ref_src():
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        return re.search(r"^REF \?= (\S+)", f.read(), re.M).group(1)


def build_driver(tmp):
    objs = []
    for root, _, names in os.walk(os.path.join(ROOT, "oracle", "_ref", "obj")):
        objs += [os.path.join(root, n) for n in names if n.endswith(".o") and n != "ref_driver.o"]
    if not any(o.endswith("pl_bipartite.o") for o in objs):
        raise SystemExit("oracle/_ref/obj has no pl_bipartite.o: run `make -C oracle ref` first")
    import pybind11
    out = os.path.join(tmp, "libbpt_ref.so")
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-w", "-shared",
           "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + ref_src(), "-I" + pybind11.get_include(),
           "-I" + sysconfig.get_paths()["include"], "-I" + os.path.join(ROOT, "oracle"),
           os.path.join(HERE, "bpt_ref_driver.cpp")] + sorted(objs) + ["-o", out]
    subprocess.run(cmd, check=True)
    L = C.CDLL(out)
    dp, ip, vp, i64 = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p, C.c_int64
    L.bpt_create.restype = vp
    L.bpt_create.argtypes = [C.c_double] * 3
    L.bpt_free.argtypes = [vp]
    L.bpt_init_lines.argtypes = [vp, dp, i64]
    L.bpt_add_keypoints.restype = C.c_double
    L.bpt_add_keypoints.argtypes = [vp, dp, ip, ip, i64]
    L.bpt_intersection_with_points.restype = C.c_double
    L.bpt_intersection_with_points.argtypes = [vp, dp, i64]
    L.bpt_count_points.restype = i64
    L.bpt_count_points.argtypes = [vp]
    L.bpt_count_edges.restype = i64
    L.bpt_count_edges.argtypes = [vp]
    L.bpt_get_junctions.argtypes = [vp, ip, dp, ip, C.POINTER(i64), ip]
    L.bpt_kdtree_dists.argtypes = [dp, i64, dp, i64, dp]
    return L


def P(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def f64(a, w):
    a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, w))
    return a if a.shape[0] else np.zeros((0, w))


def buf(a):  # a pointer is needed even for no rows
    return a if a.size else np.zeros((1,) + a.shape[1:], a.dtype)


def new_bpt(L, cfg, lines):
    c = bo.config(cfg)
    h = L.bpt_create(c["threshold_keypoints"], c["threshold_intersection"], c["threshold_merge_junctions"])
    L.bpt_init_lines(h, P(buf(lines)), lines.shape[0])
    return h


def read_junctions(L, h):
    n, e = L.bpt_count_points(h), L.bpt_count_edges(h)
    pid, xy, p3d = np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 2)), np.zeros(max(n, 1), np.int32)
    off, ids = np.zeros(n + 1, np.int64), np.zeros(max(e, 1), np.int32)
    L.bpt_get_junctions(h, P(pid, C.c_int), P(xy), P(p3d, C.c_int), P(off, C.c_int64), P(ids, C.c_int))
    return pid[:n], xy[:n], p3d[:n], off, ids[:e]


def run_reference(L, sc):
    lines, pts, kps = f64(sc["lines"], 4), f64(sc["points"], 2), f64(sc["keypoints"], 2)
    p3d = np.ascontiguousarray(sc["point3D_ids"], np.int32)
    ids = np.ascontiguousarray(sc["point_ids"], np.int32)
    out = {}
    h = new_bpt(L, sc["cfg"], lines)
    L.bpt_add_keypoints(h, P(buf(pts)), P(buf(p3d), C.c_int), P(buf(ids), C.c_int), pts.shape[0])
    pid, xy, q3d, off, lid = read_junctions(L, h)
    L.bpt_free(h)
    order = np.argsort(ids, kind="stable")  # get_all_junctions runs in point-id order
    assert np.array_equal(pid, ids[order]) and np.array_equal(xy, pts[order]) and np.array_equal(q3d, p3d[order])
    out.update(assoc_point_ids=pid, assoc_off=off, assoc_line_ids=lid)
    if lines.shape[0]:  # (without lines the reference's loops wrap around)
        h = new_bpt(L, sc["cfg"], lines)
        L.bpt_intersection_with_points(h, P(buf(kps)), kps.shape[0])
        pid, xy, _, off, lid = read_junctions(L, h)
        L.bpt_free(h)
        out.update(junc_point_ids=pid, junc_xy=xy, junc_off=off, junc_line_ids=lid)
        # the contract: the kd-tree's nearest distance is the exact minimum, for every merged junction
        o = bo.junctions(lines, kps, sc["cfg"])
        if kps.shape[0] and o["merged_xy"].shape[0]:
            q = np.ascontiguousarray(o["merged_xy"])
            kd = np.zeros(q.shape[0])
            L.bpt_kdtree_dists(P(kps), kps.shape[0], P(q), q.shape[0], P(kd))
            bf = bo.nearest_dists(kps, q)
            assert np.array_equal(kd, bf), f"{sc['name']}: kd-tree nearest distance differs from the brute-force " \
                f"minimum on {int((kd != bf).sum())} junctions: change the scene"
    return out


def scene(name, lines, points=None, keypoints=None, cfg=None, point3D_ids=None, point_ids=None):
    points = np.zeros((0, 2)) if points is None else np.asarray(points, np.float64).reshape(-1, 2)
    n = points.shape[0]
    return dict(name=name, lines=np.asarray(lines, np.float64).reshape(-1, 4), points=points,
                keypoints=np.zeros((0, 2)) if keypoints is None else np.asarray(keypoints, np.float64).reshape(-1, 2),
                cfg=bo.config(cfg), point3D_ids=np.arange(n) + 100 if point3D_ids is None else np.asarray(point3D_ids),
                point_ids=np.arange(n) if point_ids is None else np.asarray(point_ids))


def scenes():
    rng = np.random.default_rng(20261016)
    out = []
    # (a) random clutter: 300 lines, 3000 points (shuffled, sparse ids), 2500 keypoints
    lines = tb.rand_lines(rng, 300, 20.0, 200.0)
    pts = tb.rand_points(rng, 3000)
    near = lines[rng.integers(0, 300, 800)]
    t = rng.uniform(-0.1, 1.1, (800, 1))
    pts[:800] = near[:, :2] + t * (near[:, 2:] - near[:, :2]) + rng.normal(0, 1.5, (800, 2))
    out.append(scene("clutter", lines, pts, tb.rand_points(rng, 2500), point_ids=rng.permutation(6000)[:3000]))
    # (b) the same kind of scene under other thresholds
    lines = tb.rand_lines(rng, 120, 20.0, 200.0)
    pts = tb.rand_points(rng, 1500)
    out.append(scene("thresholds", lines, pts, tb.rand_points(rng, 800),
                     cfg=dict(threshold_keypoints=3.5, threshold_intersection=0.75, threshold_merge_junctions=4.25,
                              unknown_key=1.0)))
    # (c) distances exactly at the threshold (`>`: 2.0 connects), beyond both segment ends, zero-length lines
    nx = float(np.nextafter(2.0, 3.0))
    lines = [[0, 0, 100, 0], [200, 0, 200, 100], [300, 300, 300, 300], [400, 400, 400, 400], [500, 10, 560, 90]]
    pts = [[50, 2.0], [50, -2.0], [50, nx], [50, -nx], [202.0, 50], [198.0, 50], [200 + nx, 50], [200 - nx, 50],
           [-2.0, 0], [-nx, 0], [102.0, 0], [100 + nx, 0], [-1.2, -1.6], [101.2, 1.6], [-1.5, 1.5], [200, -2.0],
           [200, 102.0], [200, 100 + nx], [201.2, 101.6], [300, 300], [302.0, 300], [300, 298.0], [300 + nx, 300],
           [301.2, 301.6], [401, 401], [402, 402], [498.8, 8.4], [561.2, 91.6], [530, 50], [531.6, 48.8], [0, 0]]
    out.append(scene("edges", lines, pts, [[0.0, 2.0], [100.0, 1.5], [200.0, 50.0]]))
    # (d) intersect(): each endpoint-proximity test alone, one pair that satisfies two, crossings on and off the
    # segments, near-parallel pairs (z + EPS small), collinear and identical lines
    lines = [[0, 0, 50, 0], [1, 1, 20, 40],            # start-start
             [100, 0, 150, 0], [151, 1, 170, 40],      # end-start
             [200, 0, 250, 0], [220, 40, 201, 1],      # start-end
             [300, 0, 350, 0], [320, 40, 351, 1],      # end-end
             [400, 0, 401, 0], [400.5, 0.5, 401.5, 0.5],  # short lines: all four hold, the first wins
             [500, 0, 500.5, 0], [480, 30, 501, 0.5],  # end-start and end-end hold (not start-start): end-start wins
             [0, 100, 60, 160], [0, 160, 60, 100],     # a crossing inside both
             [100, 100, 160, 160], [100, 190, 128, 162],  # a crossing 1.41 beyond the end of the second: accepted
             [200, 100, 260, 160], [200, 190, 226, 164],  # 2.83 beyond: rejected
             [0, 300, 400, 300.0001], [0, 300.5, 400, 300.4999],  # near-parallel, crossing inside
             [0, 400, 400, 400], [0, 401, 400, 401.000001],       # near-parallel, crossing far outside
             [0, 500, 100, 500], [150, 500, 300, 500],            # collinear, disjoint
             [0, 600, 100, 600], [0, 600, 100, 600],              # identical
             [0, 700, 100, 700], [0, 703, 100, 703]]              # parallel
    out.append(scene("intersect", lines, keypoints=[[30.0, 130.0], [1000.0, 1000.0]]))
    # (e) the re-parenting chain: candidates 1.5 apart along a row (each within 2.0 of the next, not of the one
    # after), in a scrambled line order, so that a candidate leaves an earlier cluster for a later one
    order = rng.permutation(12)
    lines = [[1.5 * k, 1000.0, 1.5 * k + 40.0 * np.cos(0.25 * n + 0.1), 1000.0 + 300.0 + 25.0 * n]
             for n, k in enumerate(order)]
    out.append(scene("chain", lines, keypoints=[[5000.0, 5000.0]]))
    lines = [[3.0 * k, 0.0, 3.0 * k, 1.9] for k in (4, 0, 3, 1, 2)] + [[1.5 + 3.0 * k, 0.95, 40.0 + k, 60.0] for k in (2, 0, 3, 1)]
    out.append(scene("chain2", lines))
    # (f) one line only: its two endpoints; a keypoint exactly at the threshold keeps the junction (`<`), one
    # inside drops it
    out.append(scene("one_line", [[0, 0, 100, 0]], [[10.0, 1.0]], [[0.0, 2.0], [100.0, 1.5]]))
    out.append(scene("one_line_short", [[0, 0, 1.0, 1.0]], keypoints=[[50.0, 50.0]]))
    # (g) no keypoints: tree.empty()
    lines = tb.rand_lines(rng, 60, 30.0, 250.0)
    out.append(scene("no_keypoints", lines, tb.rand_points(rng, 100)))
    # (h) no lines: association only (every point without a neighbour)
    out.append(scene("no_lines", np.zeros((0, 4)), tb.rand_points(rng, 5), tb.rand_points(rng, 5)))
    return out


def timing(L):
    cfg = bo.config()
    res = dict(threads=1, note="structures/pl_bipartite.cc is serial; wall ms inside the reference's calls",
               cpu=os.popen("lscpu | grep 'Model name'").read().split(":")[-1].strip())
    sc = tb.assoc_scene()
    ms = []
    for lines, pts in sc:
        h = new_bpt(L, cfg, f64(lines, 4))
        p3d = np.arange(pts.shape[0], dtype=np.int32)
        ms.append(L.bpt_add_keypoints(h, P(f64(pts, 2)), P(p3d, C.c_int), P(p3d, C.c_int), pts.shape[0]))
        L.bpt_free(h)
    n, m, p = tb.ASSOC_SHAPE
    res["association"] = dict(images=n, lines_per_image=m, keypoints_per_image=p, total_ms=float(np.sum(ms)),
                              per_image_ms=float(np.median(ms)))
    res["junctions"] = []
    for m in tb.JUNCTION_LINES:
        lines, kps = tb.junction_scene(m)
        h = new_bpt(L, cfg, f64(lines, 4))
        t = L.bpt_intersection_with_points(h, P(f64(kps, 2)), kps.shape[0])
        res["junctions"].append(dict(lines=m, keypoints=int(kps.shape[0]), junctions=int(L.bpt_count_points(h)),
                                     per_image_ms=float(t)))
        L.bpt_free(h)
        print(res["junctions"][-1], flush=True)
    return res


def main():
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        if "--timing-only" not in sys.argv:
            for sc in scenes():
                res = run_reference(L, sc)
                arrays = {k: np.asarray(v) for k, v in sc.items() if k not in ("name", "cfg")}
                np.savez_compressed(os.path.join(OUT, f"bpt_{sc['name']}.npz"), **arrays,
                                    **{"cfg_" + k: np.float64(v) for k, v in sc["cfg"].items()},
                                    **{"out_" + k: v for k, v in res.items()})
                print(f"bpt_{sc['name']}.npz: {res.get('junc_xy', np.zeros(0)).shape[0]} junctions, "
                      f"{res['assoc_line_ids'].shape[0]} edges")
        if "--no-timing" not in sys.argv:
            t = timing(L)
            with open(os.path.join(OUT, "bpt_ref_time.json"), "w") as f:
                json.dump(t, f, indent=1)
            print(json.dumps(t))


if __name__ == "__main__":
    main()
