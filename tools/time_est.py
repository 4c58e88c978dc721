"""Times the minimal pose solvers (limap_amd.estimators.minimal_solver).  Per solver kind, planted
samples (random rotation, t ~ N(0, I), points and line endpoints at depth 2..6): one call of 100 samples (the hypotheses
of one RANSAC round of one query) and one of 25 600 (100 for each of 256 queries), warm process, median of repeated
calls of lt_est_minimal with the stages of lt_est_minimal_get_timers (host ms of validation + table + upload, kernel,
download; device ms of k_est_minimal by HIP events), and lt_fn_est_minimal_host on 16 threads, checked to give the same
bits.  Then the hybrid estimator itself: 256 queries of 500 points and 200 line matches (40 % outliers, half a pixel of
noise, thresholds 10 px, cfgs/localization/default.yaml's block) in ONE batch call of lt_est_solve, against lt_fn_est_host
on 16 threads on the same machine, checked to give the same bits; the three kernels of a round are timed by HIP events
in a call of their own with one round per poll.  There is no PoseLib or RansacLib to time against and the parent commit
has no such step: the figures are a record.  Not measured: hardware counters, the share of scratch traffic, the split of
k_est_replay between its refinements and its scoring passes.
Writes profiles/est_timing.json.

usage: python tools/time_est.py [--repeat 5] [--out profiles/est_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("p3p", "p2p1ll", "p1p2ll", "p3ll")


def _rot(q):
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = np.moveaxis(q, -1, 0)
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def samples(kind, n, seed=0):
    """n planted samples of a kind as the five arrays of minimal_solver, built with array operations"""
    rng = np.random.default_rng(seed)
    nl = KINDS.index(kind)
    npts = 3 - nl
    R, t = _rot(rng.normal(size=(n, 4))), rng.normal(size=(n, 3))

    def cam(m):
        d = rng.uniform(2, 6, (n, m, 1))
        return np.concatenate([rng.uniform(-1, 1, (n, m, 2)), np.ones((n, m, 1))], -1) * d

    def world(Y):
        return np.einsum("nji,nmj->nmi", R, Y - t[:, None, :])

    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)  # noqa: E731
    pc = cam(npts)
    a, b = cam(nl), cam(nl)
    A, B = world(a), world(b)
    V = unit(B - A)
    c = np.ascontiguousarray
    return (c(unit(pc)), c(world(pc)), c(unit(np.cross(unit(a), unit(b)))), c(A + rng.uniform(-2, 2, (n, nl, 1)) * V), c(V)), (R, t)


def measure(kind, n, repeat):
    from limap_amd import _capi, estimators as est
    arrays, (R, t) = samples(kind, n)
    ctx = _capi.Context()
    est.minimal_solver(kind, *arrays, ctx=ctx)  # warm: code object, buffers
    rows = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        poses, counts, tm = est.minimal_solver(kind, *arrays, ctx=ctx, return_timers=True)
        rows.append([1e3 * (time.perf_counter() - t0), tm["prepare_ms"], tm["kernel_ms"], tm["download_ms"], tm["solve_device_ms"]])
    med = np.median(np.array(rows), 0).tolist()
    est.minimal_solver(kind, *arrays, host_threads=16)
    t0 = time.perf_counter()
    hp, hc = est.minimal_solver(kind, *arrays, host_threads=16)
    host_ms = 1e3 * (time.perf_counter() - t0)
    assert hp.tobytes() == poses.tobytes() and np.array_equal(hc, counts), "host and device disagree"
    Rs = _rot(poses[..., :4] + (poses[..., :4] == 0).all(-1, keepdims=True))
    err = np.linalg.norm(Rs - R[:, None], axis=(-2, -1)) + np.linalg.norm(poses[..., 4:] - t[:, None], axis=-1)
    err[np.arange(8)[None, :] >= counts[:, None]] = np.inf
    return dict(kind=kind, samples=n, repeat=repeat,
                device=dict(call_ms=med[0], prepare_ms=med[1], kernel_ms=med[2], download_ms=med[3], k_est_minimal_ms=med[4]),
                host_16_threads_call_ms=host_ms, poses=int(counts.sum()), counts=np.bincount(counts, minlength=9).tolist(),
                planted_pose_found_share=float((err.min(1) < 1e-6).mean()))


def loop_queries(n_query, n_pts=500, n_segs=200, seed=0):
    """planted queries for the estimator: 40 % outliers of each type, half a pixel of noise, one segment per 3D line"""
    rng = np.random.default_rng(seed)
    kvec = np.array([600.0, 590.0, 400.0, 300.0])
    out = []
    for _ in range(n_query):
        R, t = _rot(rng.normal(size=(1, 4)))[0], rng.normal(size=3)

        def cam(m):
            d = rng.uniform(2, 6, (m, 1))
            return np.concatenate([rng.uniform(-1.2, 1.2, (m, 1)), rng.uniform(-0.9, 0.9, (m, 1)), np.ones((m, 1))], -1) * d

        def pix(Y):
            return np.stack([kvec[0] * Y[:, 0] / Y[:, 2] + kvec[2], kvec[1] * Y[:, 1] / Y[:, 2] + kvec[3]], -1)

        pc = cam(n_pts)
        p2 = pix(pc) + rng.normal(0, 0.5, (n_pts, 2))
        p2[:int(0.4 * n_pts)] = pix(cam(int(0.4 * n_pts)))
        a = cam(n_segs)
        b = a + rng.normal(0, 0.8, a.shape)
        b[:, 2] = np.maximum(b[:, 2], 1.5)
        sg = np.concatenate([pix(a), pix(b)], -1) + rng.normal(0, 0.5, (n_segs, 4))
        no = int(0.4 * n_segs)
        sg[:no] = np.concatenate([pix(cam(no)), pix(cam(no))], -1)
        out.append(dict(l3ds=np.concatenate([(a - t) @ R, (b - t) @ R], -1).reshape(-1, 2, 3), l3d_ids=np.arange(n_segs),
                        l2ds=sg.reshape(-1, 2, 2), p3ds=(pc - t) @ R, p2ds=p2, camera=kvec, R=R, t=t))
    return out


def measure_loop(n_query, repeat):
    from limap_amd import _capi, estimators as est
    cfg = dict(ransac=dict(method="hybrid", thres_point=10.0, thres_line=10.0, weight_point=1.0, weight_line=1.0,
                           final_least_squares=True, min_num_iterations=100, solver_flags=[True] * 4),
               optimize=dict(loss_func="TrivialLoss", loss_func_args=[]), line_cost_func="PerpendicularDist", line_weight=1.0)
    qs = loop_queries(n_query)
    csr = est._query_arrays(qs)
    st = est._hybrid_options(cfg, None, 1)._struct()
    ctx = _capi.Context()
    est.hybrid_arrays(csr, st, ctx=ctx)  # warm
    rows = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = est.hybrid_arrays(csr, st, ctx=ctx)
        tm = r["timers"]
        rows.append([1e3 * (time.perf_counter() - t0), tm["prepare_ms"], tm["rounds_ms"], tm["download_ms"], tm["rounds_device_ms"], tm["rounds"]])
    med = np.median(np.array(rows), 0).tolist()
    t0 = time.perf_counter()
    h = est.hybrid_arrays(csr, st, host_threads=16)
    host_ms = 1e3 * (time.perf_counter() - t0)
    for key in ("qvec", "tvec", "dstats", "istats", "inliers"):
        assert h[key].tobytes() == r[key].tobytes(), f"host and device disagree on {key}"
    st.poll_interval = 1  # a call of its own: one round per poll, so the events bracket single rounds
    r1 = est.hybrid_arrays(csr, st, ctx=ctx)
    Rm = _rot(r["qvec"])
    err = np.array([np.linalg.norm(Rm[i] - q["R"]) + np.linalg.norm(r["tvec"][i] - q["t"]) for i, q in enumerate(qs)])
    its = r["istats"][:, 0]
    return dict(queries=n_query, points=500, line_matches=200, repeat=repeat,
                device=dict(call_ms=med[0], prepare_ms=med[1], rounds_ms=med[2], download_ms=med[3], rounds_device_ms=med[4], rounds=med[5]),
                one_round_per_poll=dict(rounds=r1["timers"]["rounds"], rounds_device_ms=r1["timers"]["rounds_device_ms"],
                                        rounds_host_ms=r1["timers"]["rounds_ms"]),
                host_16_threads_call_ms=host_ms, iterations_median=float(np.median(its)), iterations_max=int(its.max()),
                lo_median=float(np.median(r["istats"][:, 7])), pose_error_median=float(np.median(err)),
                pose_error_max=float(err.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "est_timing.json"))
    args = ap.parse_args()
    out = dict(method="warm process; median of `repeat` calls; stages from lt_est_minimal_get_timers; call_ms includes the "
                      "Python marshalling; the host twin timed once after a warm call; no upstream binary and no parent step to "
                      "compare with; hardware counters not collected",
               runs=[measure(k, n, args.repeat) for k in KINDS for n in (100, 25600)],
               estimator=measure_loop(256, args.repeat))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
