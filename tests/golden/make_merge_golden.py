"""Golden files of limap.merging.merging (MergeToLineTracks) and the steps after it in runners/line_fitnmerge.py,
written by THE REFERENCE'S OWN CODE: merge_ref_driver.cpp (next to this file) is compiled into a temporary directory
against the objects `make -C oracle ref` builds from the reference's sources (oracle/_ref/obj/**/*.o) and the
stand-in headers of oracle/ref_shim, and called through ctypes.  Run where the reference sources exist, like
make_io_golden.py; tests/test_gpu_merge.py and tests/test_merge_host.py read the outputs.

  (all under tests/golden/merge/)
  merge_<name>.npz   inputs (cameras, 2D / 3D segments, neighbours as CSR, linker configs as JSON) and outputs: graph
                     nodes, edges in insertion order, greedy labels, the tracks after the merge, the first
                     filter_tracks_by_reprojection, the remerge and the second filter (num_outliers 0 throughout)
  merge_e_digests.json  scene (e), 60 x 300: its inputs are regenerated from limap_amd.synthetic, so only digests
  merge_ref_time.json   the reference's wall time of MergeToLineTracks on 100 x 500 x nn 20 and its thread count

usage: python tests/golden/make_merge_golden.py [--no-timing]
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "merge")  # (not tests/golden/*.npz: those are the triangulation fixtures)
REF_SRC = "/root/reference/src"

from limap_amd import synthetic as syn  # noqa: E402

L2_DEFAULT = dict(score_th=0.5, th_angle=8.0, th_overlap=0.1, th_smartoverlap=0.2, th_smartangle=1.0, th_perp=5.0,
                  th_innerseg=5.0, use_angle=True, use_overlap=True, use_smartangle=True, use_perp=True,
                  use_innerseg=False)  # base/line_linker.h:23-45
L3_DEFAULT = dict(score_th=0.5, th_angle=10.0, th_overlap=0.01, th_smartoverlap=0.1, th_smartangle=1.0, th_perp=0.02,
                  th_innerseg=0.02, th_scaleinv=0.01, use_angle=True, use_overlap=True, use_smartangle=True,
                  use_perp=False, use_innerseg=True, use_scaleinv=False)  # base/line_linker.h:85-111
L2_ORDER = ["score_th", "th_angle", "th_overlap", "th_smartoverlap", "th_smartangle", "th_perp", "th_innerseg",
            "use_angle", "use_overlap", "use_smartangle", "use_perp", "use_innerseg"]
L3_ORDER = L2_ORDER[:7] + ["th_scaleinv"] + L2_ORDER[7:] + ["use_scaleinv"]
REMERGE_L3 = dict(score_th=0.5, th_angle=5.0, th_overlap=0.001, th_smartoverlap=0.1, th_smartangle=1.0, th_perp=0.5,
                  th_innerseg=0.5)  # cfgs/fitnmerge/default.yaml:77-86
FILTER2D = (8.0, 5.0)  # cfgs/fitnmerge/default.yaml:87-89
SCENE_E = dict(n_views=60, n_segs=300, n_neighbors=10, seed=5)


def build_driver(tmp):
    objs = []
    for root, _, names in os.walk(os.path.join(ROOT, "oracle", "_ref", "obj")):
        objs += [os.path.join(root, n) for n in names if n.endswith(".o") and n != "ref_driver.o"]
    if not any(o.endswith("merging.o") for o in objs):
        raise SystemExit("oracle/_ref/obj has no merging.o: run `make -C oracle ref` first")
    import pybind11
    out = os.path.join(tmp, "libmerge_ref.so")
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-w", "-shared",
           "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + REF_SRC, "-I" + pybind11.get_include(),
           "-I" + sysconfig.get_paths()["include"], "-I" + os.path.join(ROOT, "oracle"),
           os.path.join(HERE, "merge_ref_driver.cpp")] + sorted(objs) + ["-o", out]
    subprocess.run(cmd, check=True)
    L = C.PyDLL(out)
    L.mrg_run.restype = C.c_void_p
    L.mrg_merge_ms.restype = C.c_double
    L.mrg_merge_ms.argtypes = [C.c_void_p]
    for f in ("mrg_free", "mrg_graph_size", "mrg_graph_get", "mrg_stage_size", "mrg_stage_get"):
        getattr(L, f).restype = None
    return L


def cfg_vec(d, default, order):
    full = dict(default)
    full.update(d)
    return np.array([float(full[k]) for k in order])


def scene_inputs(sc, fit, linker, var2d=5.0):
    ids = [int(i) for i in sc.img_ids]
    return dict(ids=ids, kvec=sc.kvec.copy(), qvec=sc.qvec.copy(), tvec=sc.tvec.copy(),
                segs2={i: sc.segs_of(n).copy() for n, i in enumerate(ids)},
                segs3={i: fit[i].reshape(-1, 6).copy() for i in ids},
                neighbors={i: list(sc.neighbors[i]) for i in ids}, linker=linker, var2d=var2d)


def pack(inp):
    """arrays of an input set, images in ascending id order"""
    order = np.argsort(inp["ids"], kind="stable")
    ids = [inp["ids"][n] for n in order]
    seg_off = np.zeros(len(ids) + 1, np.int64)
    nb_off = np.zeros(len(ids) + 1, np.int64)
    s2, s3, nb = [], [], []
    for n, i in enumerate(ids):
        s2.append(np.asarray(inp["segs2"][i], float).reshape(-1, 4))
        s3.append(np.asarray(inp["segs3"][i], float).reshape(-1, 6))
        nb += [int(j) for j in inp["neighbors"][i]]
        seg_off[n + 1] = seg_off[n] + len(s2[-1])
        nb_off[n + 1] = len(nb)
    return dict(img_ids=np.array(ids, np.int32), kvec=inp["kvec"][order], qvec=inp["qvec"][order],
                tvec=inp["tvec"][order], seg_off=seg_off, segs2=np.concatenate(s2, 0), segs3=np.concatenate(s3, 0),
                nb_off=nb_off, nb=np.array(nb, np.int32), var2d=float(inp["var2d"]),
                linker=json.dumps(inp["linker"], sort_keys=True))


def run_reference(L, a, n_threads=0):
    f64 = lambda x: np.ascontiguousarray(x, np.float64)  # noqa: E731
    P = lambda x, t: x.ctypes.data_as(C.POINTER(t))  # noqa: E731
    lk = json.loads(str(a["linker"]))
    l2 = cfg_vec(lk.get("linker2d", {}), L2_DEFAULT, L2_ORDER)
    l3 = cfg_vec(lk.get("linker3d", {}), L3_DEFAULT, L3_ORDER)
    rm = cfg_vec(REMERGE_L3, L3_DEFAULT, L3_ORDER)
    ids, k, q, t = np.ascontiguousarray(a["img_ids"], np.int32), f64(a["kvec"]), f64(a["qvec"]), f64(a["tvec"])
    so, s2, s3 = np.ascontiguousarray(a["seg_off"], np.int64), f64(a["segs2"]), f64(a["segs3"])
    no, nb = np.ascontiguousarray(a["nb_off"], np.int64), np.ascontiguousarray(a["nb"], np.int32)
    nb_buf = nb if nb.size else np.zeros(1, np.int32)
    h = L.mrg_run(C.c_int(len(ids)), P(ids, C.c_int32), P(k, C.c_double), P(q, C.c_double), P(t, C.c_double),
                  P(so, C.c_int64), P(s2, C.c_double), P(s3, C.c_double), P(no, C.c_int64), P(nb_buf, C.c_int32),
                  P(l2, C.c_double), P(l3, C.c_double), C.c_double(float(a["var2d"])), C.c_double(FILTER2D[0]),
                  C.c_double(FILTER2D[1]), P(rm, C.c_double), C.c_int(n_threads))
    out = {}
    N, E = C.c_int64(), C.c_int64()
    L.mrg_graph_size(C.c_void_p(h), C.byref(N), C.byref(E))
    ni, nl, lab = (np.zeros(max(N.value, 1), np.int32) for _ in range(3))
    e1, e2, sim = np.zeros(max(E.value, 1), np.int32), np.zeros(max(E.value, 1), np.int32), np.zeros(max(E.value, 1))
    L.mrg_graph_get(C.c_void_p(h), P(ni, C.c_int32), P(nl, C.c_int32), P(lab, C.c_int32), P(e1, C.c_int32),
                    P(e2, C.c_int32), P(sim, C.c_double))
    out.update(node_img=ni[:N.value], node_line=nl[:N.value], labels=lab[:N.value], edge_n1=e1[:E.value],
               edge_n2=e2[:E.value], edge_sim=sim[:E.value])
    for s, name in enumerate(("merge", "filter1", "remerge", "filter2")):
        T, M = C.c_int64(), C.c_int64()
        L.mrg_stage_size(C.c_void_p(h), s, C.byref(T), C.byref(M))
        T, M = T.value, M.value
        line7, off = np.zeros((max(T, 1), 7)), np.zeros(T + 1, np.int64)
        img, lid, nid = (np.zeros(max(M, 1), np.int32) for _ in range(3))
        sc, l2d, l3d = np.zeros(max(M, 1)), np.zeros((max(M, 1), 4)), np.zeros((max(M, 1), 10))
        L.mrg_stage_get(C.c_void_p(h), s, P(line7, C.c_double), P(off, C.c_int64), P(img, C.c_int32),
                        P(lid, C.c_int32), P(nid, C.c_int32), P(sc, C.c_double), P(l2d, C.c_double),
                        P(l3d, C.c_double))
        out.update({f"{name}_line": line7[:T], f"{name}_off": off, f"{name}_img": img[:M], f"{name}_lid": lid[:M],
                    f"{name}_nid": nid[:M], f"{name}_score": sc[:M], f"{name}_line2d": l2d[:M],
                    f"{name}_line3d": l3d[:M]})
    ms = L.mrg_merge_ms(C.c_void_p(h))
    L.mrg_free(C.c_void_p(h))
    return out, ms


def digest(*arrays):
    h = hashlib.sha256()
    for x in arrays:
        x = np.ascontiguousarray(x)
        h.update(str(x.dtype).encode() + str(x.shape).encode() + x.tobytes())
    return h.hexdigest()[:32]


def scene_e_inputs():
    sc = syn.make_scene(**SCENE_E)
    return pack(scene_inputs(sc, syn.make_fit_segs(sc, seed=SCENE_E["seed"]), syn.default_merging_cfg()))


def scenes():
    cfg = syn.default_merging_cfg()
    linker = dict(linker2d=cfg["linker2d"], linker3d=cfg["linker3d"])
    out = {}
    # (a) 12 x 80, nn 5, with zero-length lines (failed fits and clutter)
    sc = syn.make_scene(n_views=12, n_segs=80, n_neighbors=5, seed=11)
    out["a"] = scene_inputs(sc, syn.make_fit_segs(sc, seed=11, fail_frac=0.15), linker)
    # (b) non-contiguous ids, asymmetric unsorted neighbour lists, an image without neighbours, one without lines
    sc = syn.make_scene(n_views=10, n_segs=60, n_neighbors=6, seed=12)
    inp = scene_inputs(sc, syn.make_fit_segs(sc, seed=12), linker)
    remap = {i: v for i, v in zip(inp["ids"], [3, 7, 8, 15, 16, 40, 41, 42, 100, 257])}
    rng = np.random.default_rng(12)
    nbs = {}
    for i in inp["ids"]:
        others = [j for j in inp["ids"] if j != i and j not in inp["neighbors"][i]]
        extra = [int(j) for j in rng.choice(others, size=3, replace=False)]
        lst = [remap[j] for j in inp["neighbors"][i] + extra if rng.uniform() > 0.25]  # drops: asymmetric lists
        lst = [lst[k] for k in rng.permutation(len(lst))]
        nbs[remap[i]] = lst
    nbs[remap[inp["ids"][4]]] = []
    inp = dict(inp, ids=[remap[i] for i in inp["ids"]], segs2={remap[i]: v for i, v in inp["segs2"].items()},
               segs3={remap[i]: v for i, v in inp["segs3"].items()}, neighbors=nbs)
    inp["segs2"][remap[6]] = np.zeros((0, 4))
    inp["segs3"][remap[6]] = np.zeros((0, 6))
    out["b"] = inp
    # (c) a duplicated neighbour entry, and an image listed as its own neighbour
    sc = syn.make_scene(n_views=8, n_segs=60, n_neighbors=4, seed=13)
    inp = scene_inputs(sc, syn.make_fit_segs(sc, seed=13), linker)
    ids = inp["ids"]
    inp["neighbors"][ids[0]] = inp["neighbors"][ids[0]] + [inp["neighbors"][ids[0]][0]]
    inp["neighbors"][ids[3]] = [ids[3]] + inp["neighbors"][ids[3]]
    out["c"] = inp
    # (d) non-default linkers: 2D use_perp and use_innerseg on, smart angle off, a tight th_angle
    sc = syn.make_scene(n_views=12, n_segs=80, n_neighbors=5, seed=14)
    lk = dict(linker2d=dict(cfg["linker2d"], use_perp=True, use_innerseg=True, th_innerseg=3.0,
                            use_smartangle=False, th_angle=2.0),
              linker3d=dict(cfg["linker3d"], th_angle=3.0))
    out["d"] = scene_inputs(sc, syn.make_fit_segs(sc, seed=14, depth_noise=0.001), lk)
    return out


def main():
    timing = "--no-timing" not in sys.argv
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for name, inp in scenes().items():
            a = pack(inp)
            res, _ = run_reference(L, a)
            np.savez_compressed(os.path.join(OUT, f"merge_{name}.npz"), **a, **res)
            print(name, "nodes", len(res["node_img"]), "edges", len(res["edge_n1"]), "tracks",
                  [len(res[f"{s}_off"]) - 1 for s in ("merge", "filter1", "remerge", "filter2")])
        a = scene_e_inputs()
        res, _ = run_reference(L, a)
        d = dict(scene=SCENE_E, inputs=digest(a["img_ids"], a["kvec"], a["qvec"], a["tvec"], a["seg_off"], a["segs2"],
                                              a["segs3"], a["nb_off"], a["nb"]),
                 n_nodes=len(res["node_img"]), n_edges=len(res["edge_n1"]),
                 nodes=digest(res["node_img"], res["node_line"]),
                 edges=digest(res["edge_n1"], res["edge_n2"], res["edge_sim"]), labels=digest(res["labels"]))
        for s in ("merge", "filter1", "remerge", "filter2"):
            d[f"{s}_tracks"] = len(res[f"{s}_off"]) - 1
            d[f"{s}_members"] = digest(res[f"{s}_off"], res[f"{s}_img"], res[f"{s}_lid"], res[f"{s}_nid"])
            d[f"{s}_line"] = digest(res[f"{s}_line"])
        with open(os.path.join(OUT, "merge_e_digests.json"), "w") as f:
            json.dump(d, f, indent=1, sort_keys=True)
        print("e", d["n_nodes"], d["n_edges"], d["merge_tracks"])
        if timing:
            sc = syn.make_scene(n_views=100, n_segs=500, n_neighbors=20, seed=0)
            a = pack(scene_inputs(sc, syn.make_fit_segs(sc, seed=0), syn.default_merging_cfg()))
            threads = int(os.environ.get("MERGE_REF_THREADS", "0")) or L.mrg_max_threads()
            res, ms = run_reference(L, a, threads)
            t = dict(scene=dict(n_views=100, n_segs=500, n_neighbors=20, seed=0, fit_seed=0), threads=threads,
                     merge_ms=ms, n_nodes=len(res["node_img"]), n_edges=len(res["edge_n1"]),
                     n_tracks=len(res["merge_off"]) - 1)
            with open(os.path.join(OUT, "merge_ref_time.json"), "w") as f:
                json.dump(t, f, indent=1, sort_keys=True)
            print("reference MergeToLineTracks 100 x 500 x 20:", t)


if __name__ == "__main__":
    main()
