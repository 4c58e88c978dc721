"""Golden files of limap.vplib's JLinkage detector, written by THE REFERENCE'S OWN CODE around its two calls into the
J-Linkage third party: vp_ref_driver.cpp (next to this file) is compiled in a temporary directory together with the
reference's vplib/base_vp_detector.cc and vplib/JLinkage/JLinkage.cc where they lie (their path is the REF of
oracle/Makefile), against the stand-in headers of oracle/ref_shim and the objects `make -C oracle ref` builds
(base/linebase.o, base/infinite_line.o, base/graph.o).  The third party's two headers are not on disk (the
progress bar's is, next to the reference's sources); this generator writes stand-ins into the temporary directory
whose run() functions record what they receive and return the Labels / LabelCount injected here -- tests/vp_oracle.py's clustering, or
labels set by hand where a fixture aims at the reference's tail.  Nothing of the reference is stored, only data.

  (all under tests/golden/vp/)
  vp_<name>.npz      lines, the configuration, the injected Labels of the valid lines (from_oracle: they are the
                     oracle's clustering, so the golden is also the whole detector's output), what the clustering call
                     received (FP32 points, threshold, call counts), and the reference's labels and vps
  vp_recovery.json   the Manhattan scenes: per true direction the angular error (degrees) of the fitted vanishing point's
                     camera-frame direction and the share of the direction's lines that carry its label, from
                     tests/vp_oracle.py; the generator refuses a scene in which a direction gets no vanishing point

usage: python tests/golden/make_vp_golden.py
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
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "vp")

import vp_oracle as vo  # noqa: E402

STANDINS = {
    "JLinkage/include/VPSample.h": """#pragma once
#include <vector>
namespace vp_inject {
extern std::vector<unsigned int> labels, counts;
extern std::vector<float> seen_pts;
extern float seen_threshold;
extern int sample_calls, cluster_calls;
}
struct VPSample {
  static std::vector<std::vector<float> *> *run(std::vector<std::vector<float> *> *, int, int, int, int) {
    ++vp_inject::sample_calls;
    return new std::vector<std::vector<float> *>();
  }
};
""",
    "JLinkage/include/VPCluster.h": """#pragma once
#include <JLinkage/include/VPSample.h>
struct VPCluster {
  static int run(std::vector<unsigned int> &Labels, std::vector<unsigned int> &LabelCount,
                 std::vector<std::vector<float> *> *pts, std::vector<std::vector<float> *> *, float th, int) {
    ++vp_inject::cluster_calls;
    vp_inject::seen_threshold = th;
    for (auto *p : *pts) vp_inject::seen_pts.insert(vp_inject::seen_pts.end(), p->begin(), p->end());
    Labels = vp_inject::labels;
    LabelCount = vp_inject::counts;
    return (int)LabelCount.size();
  }
};
""",
}


def ref_src():
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        return re.search(r"^REF \?= (\S+)", f.read(), re.M).group(1)


def build_driver(tmp):
    objs = []
    for root, _, names in os.walk(os.path.join(ROOT, "oracle", "_ref", "obj")):
        objs += [os.path.join(root, n) for n in names if n.endswith(".o") and n != "ref_driver.o"]
    if not any(o.endswith("infinite_line.o") for o in objs):
        raise SystemExit("oracle/_ref/obj has no infinite_line.o: run `make -C oracle ref` first")
    for rel, text in STANDINS.items():
        os.makedirs(os.path.dirname(os.path.join(tmp, rel)), exist_ok=True)
        with open(os.path.join(tmp, rel), "w") as f:
            f.write(text)
    import pybind11
    out = os.path.join(tmp, "libvp_ref.so")
    ref = ref_src()
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-w", "-shared",
           "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + tmp, "-I" + ref, "-I" + pybind11.get_include(),
           "-I" + sysconfig.get_paths()["include"], "-I" + os.path.join(ROOT, "oracle"),
           os.path.join(HERE, "vp_ref_driver.cpp"), os.path.join(ref, "limap", "vplib", "base_vp_detector.cc"),
           os.path.join(ref, "limap", "vplib", "JLinkage", "JLinkage.cc")] + sorted(objs) + ["-o", out]
    subprocess.run(cmd, check=True)
    L = C.CDLL(out)
    up, dp, ip = C.POINTER(C.c_uint), C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.vp_set_injection.argtypes = [up, C.c_int64, up, C.c_int64]
    L.vp_associate.restype = C.c_int64
    L.vp_associate.argtypes = [C.c_double, C.c_double, C.c_int, C.c_double, dp, C.c_int64, ip, dp, C.c_int64]
    L.vp_seen_threshold.restype = C.c_float
    L.vp_seen_points.restype = C.c_int64
    L.vp_seen_points.argtypes = [C.POINTER(C.c_float)]
    return L


def run_reference(L, lines, cfg, injected):
    """AssociateVPs of the reference with `injected` as the third party's Labels"""
    lines = np.ascontiguousarray(lines, np.float64).reshape(-1, 4)
    n = lines.shape[0]
    lab = np.ascontiguousarray(injected, np.uint32)
    cnt = np.ascontiguousarray(np.bincount(lab) if lab.size else np.zeros(0), np.uint32)
    L.vp_set_injection((lab if lab.size else np.zeros(1, np.uint32)).ctypes.data_as(C.POINTER(C.c_uint)), lab.size,
                       (cnt if cnt.size else np.zeros(1, np.uint32)).ctypes.data_as(C.POINTER(C.c_uint)), cnt.size)
    labels = np.full(max(n, 1), -7, np.int32)
    cap = n // 3 + 1
    vps = np.zeros((cap, 3))
    buf = lines if n else np.zeros((1, 4))
    nv = L.vp_associate(cfg["min_length"], cfg["inlier_threshold"], cfg["min_num_supports"], cfg["th_perp_supports"],
                        buf.ctypes.data_as(C.POINTER(C.c_double)), n, labels.ctypes.data_as(C.POINTER(C.c_int)),
                        vps.ctypes.data_as(C.POINTER(C.c_double)), cap)
    assert nv <= cap
    npts = L.vp_seen_points(None)
    seen = np.zeros((max(npts, 1), 4), np.float32)
    L.vp_seen_points(seen.ctypes.data_as(C.POINTER(C.c_float)))
    return dict(labels=labels[:n], vps=vps[:nv], seen_pts=seen[:npts], seen_threshold=np.float32(L.vp_seen_threshold()),
                sample_calls=L.vp_sample_calls(), cluster_calls=L.vp_cluster_calls())


# ---- scenes --------------------------------------------------------------------------------------------------------------
W_IMG, H_IMG = 1024.0, 768.0


def rand_lines(rng, n, lo=45.0, hi=200.0):
    c = rng.uniform([0, 0], [W_IMG, H_IMG], (n, 2))
    ang = rng.uniform(0, np.pi, n)
    h = 0.5 * rng.uniform(lo, hi, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    return np.concatenate([c - h, c + h], 1)


def pencil(rng, n, point, lo=60.0, hi=200.0, noise=0.0):
    """n segments on lines through `point`"""
    ang = rng.uniform(0, np.pi, n)
    d = np.stack([np.cos(ang), np.sin(ang)], 1)
    r0 = rng.uniform(80.0, 500.0, n)[:, None]
    ln = rng.uniform(lo, hi, n)[:, None]
    p = np.asarray(point, np.float64)
    return np.concatenate([p + r0 * d, p + (r0 + ln) * d], 1) + rng.normal(0, noise, (n, 4)) if noise else \
        np.concatenate([p + r0 * d, p + (r0 + ln) * d], 1)


def manhattan(seed, noise=0.3, per_dir=60, clutter=0.2):
    """segments of three orthogonal 3D directions seen by a pinhole, endpoint noise, a share of clutter lines"""
    rng = np.random.default_rng([20261017, seed])
    K = np.array([[800.0, 0, 512.0], [0, 800.0, 384.0], [0, 0, 1.0]])
    a, b, c = 0.35 + 0.2 * seed, -0.5 + 0.15 * seed, 0.1
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    R = Rz @ Rx @ Ry
    lines, dirs = [], []
    for d in range(3):
        while sum(1 for x in dirs if x == d) < per_dir:
            p = rng.uniform([-4, -3, 6], [4, 3, 14])  # camera frame
            q = p + R[:, d] * rng.uniform(1.0, 3.0)
            if q[2] < 1.0:
                continue
            u, v = K @ p, K @ q
            seg = np.array([u[0] / u[2], u[1] / u[2], v[0] / v[2], v[1] / v[2]])
            if np.hypot(seg[0] - seg[2], seg[1] - seg[3]) < 50.0 or seg.min() < -200 or seg.max() > 1400:
                continue
            lines.append(seg + rng.normal(0, noise, 4))
            dirs.append(d)
    n_cl = int(round(clutter * len(lines) / (1.0 - clutter)))
    lines = np.concatenate([np.array(lines), rand_lines(rng, n_cl)], 0)
    dirs = np.array(dirs + [-1] * n_cl)
    perm = rng.permutation(len(dirs))
    return dict(lines=lines[perm], dirs=dirs[perm], K=K, R=R, noise=noise, clutter=clutter)


def scenes():
    rng = np.random.default_rng(20261017)
    out = []

    def add(name, lines, cfg=None, injected=None, **extra):
        out.append(dict(name=name, lines=np.asarray(lines, np.float64).reshape(-1, 4), cfg=cfg, injected=injected,
                        extra=extra))

    # (a) the guard at 2 * max(min_num_supports, 10) - 1 and at that value: 19 / 20 lines through one point
    p20 = pencil(rng, 20, (500.0, 300.0))
    add("guard19", p20[:19])
    add("guard20", p20)
    add("guard_cfg", pencil(rng, 27, (100.0, 700.0)), cfg=dict(min_num_supports=14))  # guard 28: one short
    # (b) lengths exactly at min_length (`<`: 40.0 stays): the twentieth valid line is exactly 40 long, or one ulp under
    at = np.array([[500.0 + 120.0, 300.0, 500.0 + 160.0, 300.0]])  # on the pencil's point's row: length 40 exactly
    under = at.copy()
    under[0, 2] = np.nextafter(under[0, 2], 0.0)
    short = np.array([[10.0, 10.0, 34.0, 42.0 - 1e-9], [0.0, 0.0, 39.0, 0.0]])
    add("len_at", np.concatenate([short[:1], p20[:19], at, short[1:]], 0))
    add("len_under", np.concatenate([short[:1], p20[:19], under, short[1:]], 0))
    add("len_345", np.concatenate([p20[:19], [[500.0 + 24.0 * 5, 300.0 + 32.0 * 5, 500.0 + 24.0 * 6, 300.0 + 32.0 * 6]]], 0))
    # (c) the tail on hand-set labels: collinear fragments (one infinite line), parallels at and just over
    # th_perp_supports, a union-find chain whose result depends on the evolving roots, equal-length pairs
    nx = float(np.nextafter(3.0, 4.0))
    L = []
    lab = []
    L += [[100.0 * k, 50.0, 100.0 * k + 60.0, 50.0] for k in range(6)]; lab += [0] * 6          # 6 fragments of one line
    L += [[0.0, 100.0 + 3.0 * k, 80.0 + k, 100.0 + 3.0 * k] for k in range(6)]; lab += [1] * 6  # 3.0 apart: a chain
    L += [[0.0, 200.0 + nx * 2 * k, 80.0 + k, 200.0 + nx * 2 * k] for k in range(6)]; lab += [2] * 6   # clearly apart
    L += [[0.0, 300.0 + nx * k, 90.0, 300.0 + nx * k] for k in range(5)]; lab += [3] * 5        # just over, equal lengths
    chain_y = [2.5 * k for k in (3, 0, 5, 1, 4, 2, 6, 9, 7, 8)]                                 # each within 3.0 of the next
    L += [[10.0 * n, 400.0 + y, 10.0 * n + 60.0 + 7.0 * ((3 * n) % 5), 400.0 + y + 0.4 * (n % 3)]
          for n, y in enumerate(chain_y)]; lab += [4] * 10
    L += [[600.0, 20.0 * k, 660.0, 20.0 * k + 80.0] for k in range(5)]; lab += [5] * 5           # equal lengths, distinct
    L += [[700.0 + 30.0 * k, 0.0, 700.0 + 30.0 * k, 45.0] for k in range(4)]; lab += [6] * 4     # too few lines
    L += [[5.0, 5.0, 20.0, 20.0]]                                                               # below min_length
    add("tail", L, injected=np.array(lab))
    # th_perp_supports = 8 is configured; parallels 5 apart stay distinct supports only under the 3.0 actually used
    L2 = [[0.0, 5.0 * k, 100.0 + k, 5.0 * k] for k in range(6)] + [[300.0, 40.0 * k, 380.0, 40.0 * k + 10.0] for k in range(7)] + \
        [[500.0 + 4.0 * k, 0.0, 500.0 + 4.0 * k, 70.0] for k in range(8)] + [[0.0, 600.0, 30.0, 600.0]]
    add("tail_cfg", L2, cfg=dict(min_length=35.0, inlier_threshold=1.5, min_num_supports=4, th_perp_supports=8.0,
                                 unknown_key=3), injected=np.array([0] * 6 + [1] * 7 + [2] * 8))
    # (d) all lines parallel: the vanishing point at infinity
    add("parallel", [[10.0 + 3.0 * k, 20.0 + 12.0 * k, 300.0 + 5.0 * k, 20.0 + 12.0 * k] for k in range(24)])
    # (e) empty input
    add("empty", np.zeros((0, 4)))
    # (f) two pencils and clutter under a non-default configuration with an unknown key
    add("two_pencils", np.concatenate([pencil(rng, 30, (2000.0, 400.0), noise=0.2), pencil(rng, 25, (300.0, -900.0), noise=0.2),
                                       rand_lines(rng, 25)], 0)[rng.permutation(80)],
        cfg=dict(min_length=50.0, inlier_threshold=2.0, min_num_supports=6, th_perp_supports=1.0, num_hypotheses=700,
                 seed=11, unknown_key="x"))
    # (g) duplicated lines
    d = pencil(rng, 15, (400.0, 400.0))
    add("duplicates", np.concatenate([d, d, rand_lines(rng, 10)], 0))
    # (h) Manhattan scenes
    for s in range(2):
        m = manhattan(s)
        add(f"manhattan{s}", m["lines"], dirs=m["dirs"], K=m["K"], R=m["R"], noise=m["noise"], clutter=m["clutter"])
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    recovery = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for sc in scenes():
            cfg = vo.config(sc["cfg"])
            lines = sc["lines"]
            ids, go = (np.zeros(0, np.int64), False) if lines.shape[0] == 0 else vo.valid_lines(lines, cfg)
            from_oracle = sc["injected"] is None
            if from_oracle:
                injected = vo.renumber(vo.cluster(vo.preference(lines[ids], cfg))) if go else np.zeros(0, np.int64)
            else:
                injected = np.asarray(sc["injected"], np.int64)
                assert go and injected.shape[0] == len(ids), (sc["name"], go, injected.shape, len(ids))
            ref = run_reference(L, lines, cfg, injected)
            assert ref["sample_calls"] == ref["cluster_calls"] == (1 if go else 0), (sc["name"], ref["sample_calls"], go)
            extra = {k: np.asarray(v) for k, v in sc["extra"].items()}
            np.savez_compressed(os.path.join(OUT, f"vp_{sc['name']}.npz"), lines=lines, injected=injected,
                                from_oracle=np.bool_(from_oracle), **{"cfg_" + k: np.asarray(v) for k, v in cfg.items()},
                                **{"ref_" + k: np.asarray(v) for k, v in ref.items()}, **extra)
            print(f"vp_{sc['name']}.npz: {lines.shape[0]} lines, {len(ids)} valid, guard {'passed' if go else 'returned'}, "
                  f"{ref['vps'].shape[0]} vps")
            if "dirs" in sc["extra"]:
                o = vo.detect(lines, cfg)
                rec = vo.recovery(sc["extra"]["dirs"], o["labels"], o["vps"], sc["extra"]["K"], sc["extra"]["R"])
                if any(r["vp"] < 0 for r in rec):
                    raise SystemExit(f"{sc['name']}: a true direction got no vanishing point: change noise / clutter")
                recovery[sc["name"]] = rec
                print(json.dumps(rec))
    with open(os.path.join(OUT, "vp_recovery.json"), "w") as f:
        json.dump(recovery, f, indent=1)


if __name__ == "__main__":
    main()
