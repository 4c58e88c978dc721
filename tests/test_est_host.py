"""The minimal pose solvers (limap_amd.estimators) on the host, without a GPU: the host twin
(lt_fn_est_minimal_host) on planted poses and against the NumPy restatement of tests/est_oracle.py, the degenerate
samples, determinism, and the Python surface; the hybrid loop's twin (lt_fn_est_host): its decisions replayed, its
numbers replayed bit for bit (every iteration record's models and score, the statistics of the returned pose, the final
least squares through the public refinement), and the device's configuration matrix on the twin first."""
import numpy as np
import pytest

import est_oracle as eo
import est_scenes as es
import loc_scenes as ls
from limap_amd import estimators as est
from limap_amd import hybrid_localization as hl

N_SAMPLES = 300
SEEDS = {"p3p": 7, "p2p1ll": 8, "p1p2ll": 9, "p3ll": 10}


def sols_of(poses, counts, i):
    return [(poses[i, j, :4], poses[i, j, 4:]) for j in range(int(counts[i]))]


def worst_residual(sols, s):
    return max([float(np.abs(eo.residuals(q, t, *(s[k] for k in es.FIELDS))).max()) for q, t in sols], default=0.0)


def paired(a, b, tol=1e-6):
    """the two solution sets have the same size and pair up one to one within tol"""
    if len(a) != len(b):
        return False
    free = list(range(len(b)))
    for q, t in a:
        R = eo.rotation(q)
        d = [eo.pose_error(b[j][0], b[j][1], R, t) for j in free]
        if not d or min(d) > tol:
            return False
        free.pop(int(np.argmin(d)))
    return True


_CACHE = {}


def solved(kind):
    """the planted batch of a kind with the twin's and the restatement's solutions, computed once"""
    if kind not in _CACHE:
        S = es.planted_batch(kind, N_SAMPLES, SEEDS[kind])
        poses, counts = est.minimal_solver(kind, *es.stack(S), host=True)
        twin = [sols_of(poses, counts, i) for i in range(N_SAMPLES)]
        ref = [eo.solve_minimal(*(s[k] for k in es.FIELDS)) for s in S]
        _CACHE[kind] = (S, twin, ref, poses, counts)
    return _CACHE[kind]


# ---- 1. planted poses ----
@pytest.mark.parametrize("kind", eo.KINDS)
def test_the_planted_pose_is_among_the_solutions(kind):
    S, twin, ref, _, _ = solved(kind)
    share = {}
    for name, sets in (("twin", twin), ("restatement", ref)):
        err = [min([eo.pose_error(q, t, s["R"], s["t"]) for q, t in sols], default=np.inf) for s, sols in zip(S, sets)]
        share[name] = float(np.mean(np.array(err) < 1e-6))
        print(f"{kind}: {name} finds the planted pose in {100 * share[name]:.1f} % of {N_SAMPLES} samples, "
              f"median error {np.median(err):.2e}")
    assert share["twin"] >= 0.95 and share["restatement"] >= 0.95, share


# ---- 2. every returned pose solves its problem ----
@pytest.mark.parametrize("kind", eo.KINDS)
def test_every_returned_pose_solves_its_problem(kind):
    S, twin, ref, poses, counts = solved(kind)
    e_twin = max(worst_residual(sols, s) for s, sols in zip(S, twin))
    e_ref = max(worst_residual(sols, s) for s, sols in zip(S, ref))
    agree = float(np.mean([paired(a, b) for a, b in zip(twin, ref)]))
    print(f"{kind}: largest normalised constraint {e_twin:.2e} (twin), {e_ref:.2e} (restatement); solution sets agree "
          f"in {100 * agree:.1f} % of samples; counts {np.bincount(counts, minlength=9).tolist()}")
    assert e_twin <= 4.0 * e_ref, (e_twin, e_ref)
    # three Newton steps from a root of the octic end at rounding level: eps times the condition of the 6 x 6 system
    # (up to some 1e4 on these samples) -- the acceptance test's own 1e-9 must not be what bounds it
    assert e_twin <= 1e-11, e_twin
    assert agree >= 0.95, agree
    assert counts.min() >= 0 and counts.max() <= est.MAX_SOLUTIONS
    for s, sols, i in zip(S, twin, range(N_SAMPLES)):
        assert not poses[i, len(sols):].any()  # zeros past the count
        for q, t in sols:
            assert abs(np.linalg.norm(q) - 1.0) < 1e-14 and q[0] > 0.0
            R = eo.rotation(q)
            assert abs(np.linalg.det(R) - 1.0) < 1e-12
            for x, X in zip(s["xs"], s["Xs"]):
                assert x @ (R @ X + t) > 0.0
        z = [q[3] / q[0] for q, _ in sols]
        assert z == sorted(z)  # ascending in the root


# ---- 3. degenerate samples ----
@pytest.mark.parametrize("name", sorted(es.degenerate_samples()))
def test_degenerate_samples_return_without_nan(name):
    s = es.degenerate_samples()[name]
    poses, counts = est.minimal_solver(s["kind"], *es.stack([s]), host=True)
    print(name, "->", int(counts[0]), "poses")
    assert 0 <= counts[0] <= est.MAX_SOLUTIONS
    assert np.isfinite(poses).all() and not poses[0, counts[0]:].any()
    for q, t in sols_of(poses, counts, 0):
        assert abs(np.linalg.norm(q) - 1.0) < 1e-14
        assert worst_residual([(q, t)], s) <= 1e-8  # a returned pose is a solution even here


def test_degenerate_samples_with_no_answer_return_none():
    D = es.degenerate_samples()
    for name in ("collinear_points", "zero_bearing", "zero_normal_and_direction", "identical_points", "half_turn_p3ll"):
        _, counts = est.minimal_solver(D[name]["kind"], *es.stack([D[name]]), host=True)
        assert counts[0] == 0, name


def test_counts_from_0_to_8():
    seen = set()
    for kind in eo.KINDS:
        seen |= set(solved(kind)[4].tolist())
    D = es.degenerate_samples()
    _, c = est.minimal_solver("p3p", *es.stack([D["half_turn_p3p"]]), host=True)
    seen |= set(c.tolist())
    print("solution counts seen:", sorted(seen))
    assert {0, 1, 2, 3, 4, 6, 8} <= seen and max(seen) == 8  # p3ll's real solutions come in pairs


# ---- 7. determinism ----
@pytest.mark.parametrize("kind", eo.KINDS)
def test_two_runs_and_thread_counts_give_identical_bits(kind):
    a = es.stack(es.planted_batch(kind, 97, 123))
    p1, c1 = est.minimal_solver(kind, *a, host_threads=1)
    p4, c4 = est.minimal_solver(kind, *a, host_threads=4)
    p4b, c4b = est.minimal_solver(kind, *a, host_threads=4)
    assert p1.tobytes() == p4.tobytes() == p4b.tobytes() and np.array_equal(c1, c4) and np.array_equal(c4, c4b)
    # a sample's result does not depend on its neighbours in the batch
    pr, cr = est.minimal_solver(kind, *(x[::-1] for x in a), host_threads=3)
    assert pr[::-1].tobytes() == p1.tobytes() and np.array_equal(cr[::-1], c1)


# ---- 8. the Python surface ----
def _K(kvec):
    return np.array([[kvec[0], 0, kvec[2]], [0, kvec[1], kvec[3]], [0, 0, 1.0]])


def test_minimal_inputs_build_the_sample_as_upstream_does():
    rng = np.random.default_rng(5)
    K = _K([600.0, 590.0, 400.0, 300.0])
    R, t = es.random_rotation(rng), rng.normal(size=3)
    Xc = [np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 1.0]) * rng.uniform(2, 6) for _ in range(5)]
    px = [(K @ (x / x[2]))[:2] for x in Xc]
    Xw = [R.T @ (x - t) for x in Xc]
    p2ds, p3ds = px[:1], Xw[:1]
    l2ds = [np.concatenate([px[1], px[2]]), np.concatenate([px[3], px[4]])]
    l3ds = [np.concatenate([Xw[1], Xw[2]]), np.concatenate([Xw[3], Xw[4]])]
    xs, Xs, lns, Cs, Vs = est.minimal_inputs(K, p2ds, p3ds, l2ds, l3ds)
    assert np.allclose(np.linalg.norm(xs, axis=1), 1) and np.allclose(np.linalg.norm(lns, axis=1), 1)
    assert np.allclose(np.linalg.norm(Vs, axis=1), 1) and np.array_equal(Cs[0], Xw[1])
    poses, counts = est.minimal_solver("p1p2ll", xs, Xs, lns, Cs, Vs, host=True)  # one sample without the leading axis
    assert poses.shape == (1, 8, 7)
    assert min(eo.pose_error(q, tt, R, t) for q, tt in sols_of(poses, counts, 0)) < 1e-9
    # a camera object and a kvec serve as K does
    class Cam:
        def K(self):
            return K
    for cam in (Cam(), [600.0, 590.0, 400.0, 300.0]):
        assert all(np.array_equal(a, b) for a, b in zip(est.minimal_inputs(cam, p2ds, p3ds, l2ds, l3ds), (xs, Xs, lns, Cs, Vs)))


def test_kinds_by_name_and_by_number_and_argument_errors():
    S = es.planted_batch("p2p1ll", 3, 1)
    a = es.stack(S)
    p0, c0 = est.minimal_solver("p2p1ll", *a, host=True)
    p1, c1 = est.minimal_solver(1, *a, host=True)
    assert p0.tobytes() == p1.tobytes() and np.array_equal(c0, c1)
    with pytest.raises(ValueError, match="unknown minimal solver"):
        est.minimal_solver("p4p", *a, host=True)
    with pytest.raises(ValueError, match="needs ls"):
        est.minimal_solver("p2p1ll", a[0], a[1], host=True)
    with pytest.raises(ValueError, match="shape"):
        est.minimal_solver("p3p", a[0], a[1], host=True)
    with pytest.raises(ValueError, match="differ in length"):
        est.minimal_solver("p2p1ll", a[0][:2], *a[1:], host=True)
    bad = a[1].copy()
    bad[1, 0, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        est.minimal_solver("p2p1ll", a[0], bad, *a[2:], host=True)
    p, c = est.minimal_solver("p3p", np.zeros((0, 3, 3)), np.zeros((0, 3, 3)), host=True)
    assert p.shape == (0, 8, 7) and c.shape == (0,)


def test_pl_estimate_absolute_pose_refuses_the_loops_by_name_and_keeps_the_null_path():
    pr = ls.make_problem(10, 20, seed=8)
    cfg = dict(ransac=dict(method=None), line_cost_func="PerpendicularDist", line_weight=2.0,
               optimize=dict(loss_func="HuberLoss", loss_func_args=[3.0]))
    start = hl.CameraPose(pr["qvec"], pr["tvec"])
    args = (pr["l3ds"], pr["l3d_ids"], pr["l2ds_flat"], pr["p3ds"], pr["p2ds"], _K(pr["kvec"]), start)
    for method in ("ransac", "solver"):
        with pytest.raises(NotImplementedError, match=method):
            est.pl_estimate_absolute_pose(dict(cfg, ransac=dict(method=method)), *args)
    with pytest.raises(ValueError, match="unknown ransac method"):
        est.pl_estimate_absolute_pose(dict(cfg, ransac=dict(method="prosac")), *args)
    in_p = np.ones(20, bool); in_p[[1, 5]] = False
    got, stats = est.pl_estimate_absolute_pose(cfg, *args, inliers_point=in_p, host=True)
    want, _ = hl.pl_estimate_absolute_pose(cfg, *args, inliers_point=in_p, host=True)
    assert stats is None and got.qvec.tobytes() == want.qvec.tobytes() and got.tvec.tobytes() == want.tvec.tobytes()


def test_the_package_exposes_the_module():
    import limap_amd
    assert limap_amd.estimators is est and "estimators" in limap_amd.__all__


def test_sanitizer_program_of_the_host_twin():
    """tools/est_host_asan.cpp + lt_est.cpp (host-only) under AddressSanitizer and UBSan, a program of its own"""
    from helpers import run_host_asan
    run_host_asan("est_asan", "est_host_asan")


# ======== the hybrid loop (host twin lt_fn_est_host) ========
import ctypes as C

from limap_amd import _capi

THR2 = 100.0


def run_twin(scenes, cfg=None, seed=1, trace_cap=400, threads=4, loc=None, **fields):
    """the twin on scenes (est_scenes.planted_scene) -> hybrid_arrays' dict; fields: lt_est_config members to set, loc:
    members of its loc block"""
    st = est._hybrid_options(cfg or es.loc_cfg(), None, seed)._struct()
    for k, v in fields.items():
        setattr(st, k, v)
    for k, v in (loc or {}).items():
        setattr(st.loc, k, v)
    return est.hybrid_arrays(est._query_arrays([es.query_of(s) for s in scenes]), st, host_threads=threads, trace_cap=trace_cap), st


def gt_score(sc, cfg):
    """the MSAC score of the planted pose under the estimator's thresholds and weights"""
    o = est._hybrid_options(cfg, None, 0).ransac_options
    r = hl.score_poses(cfg["line_cost_func"], sc["l3ds"], sc["l3d_ids"], sc["l2ds"], sc["p3ds"], sc["p2ds"], sc["camera"],
                       np.concatenate([sc["qvec"], sc["t"]])[None], thresholds=o.squared_inlier_thresholds_,
                       weights=o.data_type_weights_, host=True)
    return float(r["scores"][0])


def check6(sc, cfg, stats, what):
    """check 6: the score is below the planted pose's, and at least 90 % of the planted inliers are found"""
    planted = int(sc["inlier_points"].sum() + sc["inlier_lines"].sum())
    found = int(np.isin(np.flatnonzero(sc["inlier_points"]), stats.inlier_indices[0]).sum() +
                np.isin(np.flatnonzero(sc["inlier_lines"]), stats.inlier_indices[1]).sum())
    gt = gt_score(sc, cfg)
    print(f"{what}: score {stats.best_model_score:.2f} (planted pose {gt:.2f}), planted inliers found {found}/{planted}, "
          f"iterations {stats.num_iterations_total} {stats.num_iterations_per_solver}, LO {stats.number_lo_iterations}")
    assert stats.best_model_score < gt, what
    assert found >= 0.9 * planted, what


# ---- 4. the loop's arithmetic ----
def test_solver_probabilities_against_the_restatement():
    L = _capi.load_library()
    cases = [((0.0, 0.0), (0, 0, 0, 0), (1, 1, 1, 1), 40, 30),     # all-zero ratios: the priors
             ((0.6, 0.5), (60, 100, 64, 12), (1, 1, 1, 1), 40, 30),
             ((0.6, 0.5), (160, 300, 64, 0), (1, 0, 1, 1), 40, 30),  # a solver switched off
             ((0.6, 0.5), (5, 5, 5, 5), (1, 1, 1, 1), 40, 2),      # too few lines for p3ll
             ((0.6, 0.0), (200, 5, 5, 5), (1, 1, 1, 1), 40, 30),
             ((1.0, 1.0), (150, 150, 5, 5), (1, 1, 1, 1), 3, 0)]
    for ratios, its, flags, n_pts, n_lines in cases:
        prior, prob = np.zeros(4), np.zeros(4)
        rc = L.lt_fn_est_probabilities(_capi.ptr(np.array(ratios, float)), _capi.ptr(np.array(its, np.uint32), C.c_uint32),
                                       _capi.ptr(np.array(flags, np.int32), C.c_int32), n_pts, n_lines, 100, _capi.ptr(prior),
                                       _capi.ptr(prob))
        want_prior = eo.priors(flags, n_pts, n_lines)
        assert rc == int(any(p > 0 for p in want_prior))
        assert np.array_equal(prior, want_prior)
        assert np.allclose(prob, eo.probabilities(ratios, its, want_prior, 100), rtol=1e-12, atol=0.0)
    assert L.lt_fn_est_probabilities(_capi.ptr(np.zeros(2)), _capi.ptr(np.zeros(4, np.uint32), C.c_uint32),
                                     _capi.ptr(np.ones(4, np.int32), C.c_int32), 2, 0, 100, _capi.ptr(prior), _capi.ptr(prob)) == 0


def test_num_required_iterations_and_the_logarithm():
    L = _capi.load_library()
    for x in (1e-300, 1e-9, 0.1, 0.5, 0.7071067811865476, 0.9999, 1.0, 1.4142135623730951, 2.0, 1e4, 1e300):
        assert abs(L.lt_fn_est_log(x) - math.log(x)) <= 4e-16 * max(1.0, abs(math.log(x))), x
    n = 0
    for r0 in (0.0, 1e-6, 0.05, 0.3, 0.6, 0.95, 1.0):
        for r1 in (0.0, 0.2, 0.55, 1.0):
            for solver in range(4):
                for lo, hi in ((100, 10000), (0, 50), (10, 10)):
                    got = L.lt_fn_est_num_required(_capi.ptr(np.array([r0, r1])), 0.9999, solver, lo, hi)
                    want, frac = eo.num_required((r0, r1), 0.9999, solver, lo, hi)
                    assert got == want or frac < 1e-9, (r0, r1, solver, lo, hi, got, want)
                    n += 1
    # the ends: p -> 0 gives the maximum, p -> 1 the minimum
    assert L.lt_fn_est_num_required(_capi.ptr(np.array([0.0, 0.9])), 0.9999, 0, 100, 10000) == 10000
    assert L.lt_fn_est_num_required(_capi.ptr(np.array([1.0, 0.0])), 0.9999, 0, 100, 10000) == 100
    assert L.lt_fn_est_num_required(_capi.ptr(np.array([1e-200, 0.9])), 0.9999, 0, 100, 10000) == 10000


import math  # noqa: E402


def replay(res, st, q=0):
    """the trace of query q replayed under the restatement: the draws, the frozen probabilities, the caps, the LO rules"""
    tr = res["trace"][q][:res["istats"][q][11]]
    it_rec = tr[tr[:, 0] == 0]
    lo_rec = tr[tr[:, 0] == 1]
    fin = tr[tr[:, 0] == 2]
    assert len(fin) == 1 and fin[0] is not None and tr[-1, 0] == 2
    csr_q = res["query_sizes"][q]
    prior = eo.priors([bool(f) for f in st.solver_flags], *csr_q)
    R, min_it = st.round_size, st.min_num_iterations
    max_it = max(st.max_num_iterations, min_it)
    cap0 = max(st.max_num_iterations_per_solver, min_it)
    its, ratios, caps = [0] * 4, [0.0, 0.0], [cap0] * 4
    frozen = None
    best_prev, n_new_best, lo_flags, had_best = np.inf, 0, 0, False
    for n, r in enumerate(it_rec):
        it, solver, flags = int(r[1]), int(r[2]), int(r[5])
        assert it == n and it < max_it
        if n % R == 0:  # a round starts: the probabilities freeze (no break inside a run's earlier rounds)
            frozen = eo.probabilities(ratios, its, prior, min_it)
        u = eo.Rng(st.random_seed, q, it, 0).unit()
        assert solver == eo.select(frozen, prior, u), (n, solver)
        its[solver] += 1
        assert int(r[10]) == its[solver]
        if flags & 4:  # the LO at lo_starting_iterations_: exactly there, and only with a model
            assert it == st.lo_starting_iterations and had_best
        if it == st.lo_starting_iterations and had_best:
            assert flags & 4
        if flags & 1:
            had_best = True
        if flags & 2:  # LO in the loop: a new best or the starting iteration, never before it
            assert it >= st.lo_starting_iterations and (flags & 1 or it == st.lo_starting_iterations)
        if (flags & 1) and it >= st.lo_starting_iterations:
            assert flags & 2
        assert r[6] <= best_prev
        best_prev = r[6]
        if flags & 7:  # the termination criteria were updated: the caps follow from the ratios
            ratios = [r[7], r[8]]
            for s in range(4):
                want, frac = eo.num_required(ratios, st.success_probability, s, min_it, st.max_num_iterations_per_solver)
                caps[s] = want if s != solver or frac < 1e-9 else int(r[9])
            want, frac = eo.num_required(ratios, st.success_probability, solver, min_it, st.max_num_iterations_per_solver)
            assert int(r[9]) == want or frac < 1e-9
        else:
            assert [r[7], r[8]] == ratios and int(r[9]) == caps[solver]
        assert bool(flags & 8) == (its[solver] >= int(r[9]))  # the break at the per-solver cap
        if flags & 8:
            assert n == len(it_rec) - 1
    total = int(fin[0][1])
    assert total == res["istats"][q][0]
    ended_by_cap = len(it_rec) and int(it_rec[-1][5]) & 8
    assert total == (len(it_rec) - 1 if ended_by_cap else len(it_rec))  # the breaking iteration does not count
    if not ended_by_cap:
        assert total == max_it
    # the local optimisations: sample sizes and the threshold schedule
    for r in lo_rec:
        n_base = int(r[3] + r[4])
        assert int(r[5]) == eo.lo_sizes(n_base, st.non_min_sample_multiplier)
        rel, upd = eo.lo_thresholds(st.squared_inlier_thresholds[0], st.threshold_multiplier, st.num_lsq_iterations)
        assert abs(r[6] - rel) <= 1e-12 * rel and abs(r[7] - upd) <= 1e-12 * max(upd, 1e-300)
        assert r[9] <= r[8]  # never worse than the model it started from
    n_lo_loop = int(sum(bool(int(r[5]) & 2) + bool(int(r[5]) & 4) for r in it_rec))
    after = 1 if (total <= st.lo_starting_iterations and had_best) else 0  # the LO after a run shorter than that
    assert len(lo_rec) == n_lo_loop + after == res["istats"][q][7]
    assert int(fin[0][2]) == st.final_least_squares
    if not st.final_least_squares:
        assert fin[0][3] == 0.0
    return dict(total=total, ended_by_cap=bool(ended_by_cap), n_lo=len(lo_rec), after=after, final_applied=fin[0][3])


def twin_with_sizes(scenes, **kw):
    res, st = run_twin(scenes, **kw)
    res["query_sizes"] = [(len(s["p3ds"]), len(s["l2ds"])) for s in scenes]
    return res, st


def test_the_trace_replays_under_the_restatement():
    sc = es.planted_scene(seed=1)
    res, st = twin_with_sizes([sc])
    info = replay(res, st)
    assert info["n_lo"] >= 2 and not info["after"]
    lo_at_start = [r for r in res["trace"][0] if r[0] == 0 and int(r[5]) & 4]
    assert len(lo_at_start) == 1 and int(lo_at_start[0][1]) == st.lo_starting_iterations  # exactly once
    # a solver switched off, and too little data for two more
    res, st = twin_with_sizes([es.planted_scene(n_pts=40, n_segs=2, n_l3d=2, seed=2)], cfg=es.loc_cfg(flags=(True, False, True, True)))
    replay(res, st)
    assert res["istats"][0][2] == 0 and res["istats"][0][4] == 0  # p2p1ll is off, p3ll lacks a third line
    assert eo.priors((True, False, True, True), 40, 2) == [9880.0, 0.0, 40.0, 0.0]


def test_the_break_at_the_per_solver_cap_and_the_end_at_max_iterations():
    sc = es.planted_scene(seed=1)
    res, st = twin_with_sizes([sc], cfg=es.loc_cfg(min_num_iterations=10), max_num_iterations_per_solver=37)
    info = replay(res, st)
    assert info["ended_by_cap"] and 37 in res["istats"][0][1:5] and info["total"] % 64 != 63  # inside a round
    res, st = twin_with_sizes([es.planted_scene(outliers=0.9, seed=4)], max_num_iterations=150)
    info = replay(res, st)
    assert not info["ended_by_cap"] and info["total"] == 150


def test_lo_after_a_short_run_and_final_least_squares_on_and_off():
    sc = es.planted_scene(seed=3)
    res, st = twin_with_sizes([sc], cfg=es.loc_cfg(min_num_iterations=5), max_num_iterations=30)  # shorter than lo_starting_iterations_
    info = replay(res, st)
    assert info["total"] == 30 and info["after"] == 1 and info["n_lo"] == 1
    on, st_on = twin_with_sizes([sc], cfg=es.loc_cfg(final_least_squares=True))
    off, st_off = twin_with_sizes([sc], cfg=es.loc_cfg(final_least_squares=False))
    a, b = replay(on, st_on), replay(off, st_off)
    assert b["final_applied"] == 0.0 and a["total"] == b["total"]
    assert on["dstats"][0][0] <= off["dstats"][0][0]  # the refined model is taken only where it scores lower
    if a["final_applied"]:
        assert on["dstats"][0][0] < off["dstats"][0][0]


def test_lo_sample_sizes_of_6_and_of_more_than_64():
    res, st = twin_with_sizes([es.planted_scene(n_pts=8, n_segs=6, n_l3d=5, outliers=0.2, seed=6)])
    replay(res, st)
    assert 6 in [int(r[5]) for r in res["trace"][0] if r[0] == 1]
    res, st = twin_with_sizes([es.planted_scene(n_pts=200, n_segs=100, n_l3d=60, outliers=0.2, seed=5)],
                              non_min_sample_multiplier=30, min_sample_multiplicator=30)
    replay(res, st)
    assert max(int(r[5]) for r in res["trace"][0] if r[0] == 1) > 64


# ---- 5. round_size 1 against 64 ----
def test_round_size_1_is_the_sequential_loop_and_64_serves_as_well():
    sc, cfg = es.planted_scene(seed=1), es.loc_cfg()
    for rs in (1, 64):
        res, st = twin_with_sizes([sc], cfg=cfg, round_size=rs)
        replay(res, st)  # with round_size 1 the probabilities of every iteration come from the state before it
        check6(sc, cfg, res["stats"][0], f"round_size {rs}")


# ---- 6. end to end ----
FLAG_SETS = [(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
             (True, True, True, True)]


@pytest.mark.parametrize("flags", FLAG_SETS, ids=["p3p", "p2p1ll", "p1p2ll", "p3ll", "all"])
def test_planted_scenes_end_to_end(flags):
    errs = []
    for seed in (1, 2, 3):
        sc, cfg = es.planted_scene(seed=seed), es.loc_cfg(flags=flags)
        pose, stats = est.pl_estimate_absolute_pose(cfg, sc["l3ds"], sc["l3d_ids"], sc["l2ds"], sc["p3ds"], sc["p2ds"],
                                                    sc["camera"], host=True, seed=1)
        check6(sc, cfg, stats, f"flags {flags} scene {seed}")
        errs.append(eo.pose_error(pose.qvec, pose.tvec, sc["R"], sc["t"]))
        off = [i for i, f in enumerate(flags) if not f]
        assert all(stats.num_iterations_per_solver[i] == 0 for i in off)
    print(f"flags {flags}: pose errors {['%.2e' % e for e in errs]}")


def test_points_only_lines_only_and_too_few_correspondences():
    cfg = es.loc_cfg()
    sc = es.planted_scene(n_pts=40, n_segs=0, n_l3d=0, seed=11)
    pose, stats = est.pl_estimate_absolute_pose(cfg, [], [], [], sc["p3ds"], sc["p2ds"], sc["camera"], host=True, seed=1)
    check6(sc, cfg, stats, "points only")
    assert stats.num_iterations_per_solver[1:] == [0, 0, 0] and stats.inlier_ratios[1] == 0.0
    sc = es.planted_scene(n_pts=0, n_segs=30, n_l3d=20, seed=12)
    pose, stats = est.pl_estimate_absolute_pose(cfg, sc["l3ds"], sc["l3d_ids"], sc["l2ds"], [], [], sc["camera"], host=True, seed=1)
    check6(sc, cfg, stats, "lines only")
    assert stats.num_iterations_per_solver[:3] == [0, 0, 0]
    # VerifyData false: the input pose back, zero iterations
    sc = es.planted_scene(n_pts=1, n_segs=1, n_l3d=1, seed=13)
    start = hl.CameraPose([0.9, 0.1, -0.2, 0.3], [0.5, -1.0, 2.0])
    pose, stats = est.pl_estimate_absolute_pose(cfg, sc["l3ds"], sc["l3d_ids"], sc["l2ds"], sc["p3ds"], sc["p2ds"], sc["camera"],
                                                campose=start, host=True)
    assert not stats.ran and stats.num_iterations_total == 0 and stats.number_lo_iterations == 0 and stats.best_num_inliers == 0
    assert np.array_equal(pose.qvec, start.qvec) and np.array_equal(pose.tvec, start.tvec)
    sc = es.planted_scene(n_pts=3, n_segs=0, n_l3d=0, seed=13)  # three points with p3p switched off
    _, stats = est.pl_estimate_absolute_pose(es.loc_cfg(flags=(False, True, True, True)), [], [], [], sc["p3ds"], sc["p2ds"],
                                             sc["camera"], host=True)
    assert not stats.ran


@pytest.mark.parametrize("cost", ["MidpointDist2", "PerpendicularDist2", "PerpendicularDist4", "3DLineLineDist2", "3DPlaneLineDist2"])
def test_each_line_cost_function_of_the_scoring(cost):
    thres = 10.0 if not cost.startswith("3D") else 0.1  # the 3D costs are distances in the scene's units
    sc, cfg = es.planted_scene(seed=2), es.loc_cfg(cost=cost, thres=thres)
    pose, stats = est.pl_estimate_absolute_pose(cfg, sc["l3ds"], sc["l3d_ids"], sc["l2ds"], sc["p3ds"], sc["p2ds"], sc["camera"],
                                                host=True, seed=1)
    check6(sc, cfg, stats, cost)
    with pytest.raises(ValueError, match="MidpointAngle"):
        est.pl_estimate_absolute_pose(es.loc_cfg(cost="MidpointAngleDist"), sc["l3ds"], sc["l3d_ids"], sc["l2ds"], sc["p3ds"],
                                      sc["p2ds"], sc["camera"], host=True)


# ---- 7. determinism ----
def test_the_loop_is_deterministic_and_seeded():
    scenes = [es.planted_scene(n_pts=20 + i, n_segs=12 + i, n_l3d=8, seed=20 + i) for i in range(5)]
    a, _ = run_twin(scenes, threads=1)
    b, _ = run_twin(scenes, threads=4)
    c, _ = run_twin(scenes, threads=4)
    for k in ("qvec", "tvec", "dstats", "istats", "inliers", "trace"):
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k
    d, _ = run_twin(scenes, seed=2)
    assert not np.array_equal(a["trace"][0][:50, 2], d["trace"][0][:50, 2])  # other seeds, other draws
    # a query's draws are keyed by its index: the same scene at two places of a batch runs two different sample sequences
    e, _ = run_twin([scenes[0], scenes[0]])
    assert not np.array_equal(e["trace"][0][:50, 2], e["trace"][1][:50, 2])


# ---- 8. the Python surface of the loop ----
def test_the_runners_call_with_the_default_localization_block():
    from limap_amd.base import Line2d, Line3d
    sc = es.planted_scene(seed=7)
    cfg = es.loc_cfg()  # cfgs/localization/default.yaml's block
    l3ds = [Line3d(a[0], a[1]) for a in sc["l3ds"]]
    l2ds = [Line2d(a[0], a[1]) for a in sc["l2ds"]]

    class Cam:
        def K(self):
            k = sc["camera"]
            return _K(k)
    final_pose, ransac_stats = est.pl_estimate_absolute_pose(cfg, l3ds, sc["l3d_ids"], l2ds, sc["p3ds"], sc["p2ds"], Cam(),
                                                             campose=None, inliers_line=None, inliers_point=None, silent=True,
                                                             logger=None, host=True)
    check6(sc, cfg, ransac_stats, "the runner's call")
    assert eo.pose_error(final_pose.qvec, final_pose.tvec, sc["R"], sc["t"]) < 0.05
    assert ransac_stats.num_iterations_total >= 100 and len(ransac_stats.inlier_ratios) == 2
    # the threshold-weighted data_type_weights_ of _pl_estimate_absolute_pose.py:114-128
    o = est._hybrid_options(dict(cfg, ransac=dict(cfg["ransac"], thres_point=3.0, thres_line=4.0, weight_line=2.0)), None, None)
    assert o.ransac_options.squared_inlier_thresholds_ == [9.0, 16.0]
    assert np.allclose(o.ransac_options.data_type_weights_, [16.0 / 25.0, 2.0 * 9.0 / 25.0])
    # the batch call and the options route give the same bits
    batch = est.pl_estimate_absolute_pose_batch(cfg, [es.query_of(sc)], host=True)
    assert batch[0][0].qvec.tobytes() == final_pose.qvec.tobytes() and batch[0][1].best_model_score == ransac_stats.best_model_score
    opts = est._hybrid_options(cfg, None, None)
    pose2, st2 = est.EstimateAbsolutePose_PointLine_Hybrid(sc["l3ds"], sc["l3d_ids"], sc["l2ds"], sc["p3ds"], sc["p2ds"],
                                                           sc["camera"], opts, host=True)
    assert pose2.tvec.tobytes() == final_pose.tvec.tobytes() and st2.inlier_indices == ransac_stats.inlier_indices
    opts.random = True
    assert opts._struct().random_seed != opts._struct().random_seed


# ---- 9. the twin's numbers: every record's values, the statistics, the final least squares ----
def numeric_cases():
    d = es.planted_scene
    return {
        "default": dict(scenes=[d(seed=1)], cfg=es.loc_cfg()),
        "3DLineLineDist2": dict(scenes=[d(seed=2)], cfg=es.loc_cfg(cost="3DLineLineDist2", thres=0.1)),
        "lines-only": dict(scenes=[d(n_pts=0, n_segs=30, n_l3d=20, seed=12)], cfg=es.loc_cfg()),
        "round-size-1": dict(scenes=[d(seed=3)], cfg=es.loc_cfg(final_least_squares=False), fields=dict(round_size=1)),
        "two-queries": dict(scenes=[d(n_pts=20, n_segs=12, n_l3d=8, seed=20), d(n_pts=25, n_segs=16, n_l3d=8, seed=21)], cfg=es.loc_cfg()),
        "points-only": dict(scenes=[d(n_pts=40, n_segs=0, n_l3d=0, seed=11)], cfg=es.loc_cfg()),
        # three pixels of noise: squared errors on both sides of each threshold, so the two cannot be exchanged unseen
        "unequal-thresholds": dict(scenes=[d(noise=3.0, seed=1)], cfg=es._ransac(es.loc_cfg(), thres_point=4.0, thres_line=12.0, weight_line=2.0)),
        "groups-of-three": dict(scenes=[d(n_pts=50, n_segs=45, n_l3d=15, seed=5)], cfg=es.loc_cfg()),
    }


REPLAYED = ["default", "3DLineLineDist2", "lines-only", "round-size-1", "two-queries"]
_NUMERIC = {}


def numeric(name, **over):
    """a numeric case with the twin's result and the configuration it ran under, computed once"""
    key = (name, tuple(sorted(over.items())))
    if key not in _NUMERIC:
        case = numeric_cases()[name]
        cfg = dict(case["cfg"], ransac=dict(case["cfg"]["ransac"], **over))
        res, st = run_twin(case["scenes"], cfg=cfg, trace_cap=600, **case.get("fields", {}))
        assert (res["istats"][:, 11] <= 600).all()
        _NUMERIC[key] = (dict(case, cfg=cfg), res, st)
    return _NUMERIC[key]


def score_at(sc, cfg, st, poses):
    """hl.score_poses on the host under the estimator's thresholds, weights and cheirality bounds"""
    return hl.score_poses(cfg["line_cost_func"], sc["l3ds"], sc["l3d_ids"], sc["l2ds"], sc["p3ds"], sc["p2ds"], sc["camera"],
                          np.asarray(poses, float).reshape(-1, 7), cheirality_min_depth=st.cheirality_min_depth,
                          cheirality_overlap_pixels=st.cheirality_overlap_pixels, thresholds=tuple(st.squared_inlier_thresholds),
                          weights=tuple(st.data_type_weights), host=True)


@pytest.mark.parametrize("name", REPLAYED)
def test_every_iteration_record_replays_numerically(name):
    """The values of the trace, not only its decisions: the restated draws (est_oracle.sample_picks) and sample
    (est_oracle.loop_sample) of every iteration record, solved by the twin's minimal solver and scored by the host
    scoring, give the record's number of models and its best local score, with == on the doubles."""
    case, res, st = numeric(name)
    for q, sc in enumerate(case["scenes"]):
        tr = res["trace"][q][:res["istats"][q][11]]
        it_rec = tr[tr[:, 0] == 0]
        n_pts, n_lines = len(sc["p3ds"]), len(sc["l2ds"])
        by_solver = {s: [] for s in range(4)}
        for n, r in enumerate(it_rec):
            solver = int(r[2])
            rng = eo.Rng(st.random_seed, q, int(r[1]), 0)
            rng.unit()  # the solver's draw
            pp = eo.sample_picks(rng, 3 - solver, n_pts)
            pl = eo.sample_picks(rng, solver, n_lines)
            assert len(set(pp)) == len(pp) and len(set(pl)) == len(pl), (name, n)
            assert all(0 <= i < n_pts for i in pp) and all(0 <= i < n_lines for i in pl), (name, n)
            by_solver[solver].append((n, eo.loop_sample(sc, sc["camera"], solver, pp, pl)))
        counts = np.zeros(len(it_rec), int)
        best = np.full(len(it_rec), np.inf)
        for solver, items in by_solver.items():
            if not items:
                continue
            arrays = [np.array([s[k] for _, s in items]) if items[0][1][k].size else None for k in range(5)]
            poses, cnt = est.minimal_solver(solver, *arrays, host=True)
            flat = [(n, poses[i, j]) for i, (n, _) in enumerate(items) for j in range(int(cnt[i]))]
            for i, (n, _) in enumerate(items):
                counts[n] = cnt[i]
            if flat:
                scores = score_at(sc, case["cfg"], st, np.array([p for _, p in flat]))["scores"]
                for (n, _), s in zip(flat, scores):
                    best[n] = min(best[n], float(s))
        has = counts > 0
        bad = np.flatnonzero(counts != it_rec[:, 3].astype(int))
        assert not len(bad), (name, q, "n_models", bad[:5])
        bad = np.flatnonzero(best[has] != it_rec[has, 4])
        assert not len(bad), (name, q, "best_local", bad[:5], best[has][bad[:5]], it_rec[has, 4][bad[:5]])
        print(f"{name}, query {q}: {len(it_rec)} iteration records checked, {int(has.sum())} with poses")
        assert has.sum() >= 10


@pytest.mark.parametrize("name", sorted(numeric_cases()))
def test_the_returned_statistics_belong_to_the_returned_pose(name):
    case, res, st = numeric(name)
    thr2 = tuple(st.squared_inlier_thresholds)
    for q, sc in enumerate(case["scenes"]):
        s = res["stats"][q]
        r = score_at(sc, case["cfg"], st, np.concatenate([res["qvec"][q], res["tvec"][q]]))
        n_pts, n_lines = len(sc["p3ds"]), len(sc["l2ds"])
        inl = [np.flatnonzero(r["residuals"][0][:n_pts] < thr2[0]).tolist(), np.flatnonzero(r["residuals"][0][n_pts:] < thr2[1]).tolist()]
        assert r["scores"][0] == s.best_model_score, (name, q)
        assert inl == s.inlier_indices, (name, q)
        assert s.inlier_ratios == [len(inl[0]) / n_pts if n_pts else 0.0, len(inl[1]) / n_lines if n_lines else 0.0], (name, q)
        assert s.best_num_inliers == len(inl[0]) + len(inl[1]) > 0, (name, q)
        assert r["inliers"][0].tolist() == [len(inl[0]), len(inl[1])]


@pytest.mark.parametrize("name", ["default", "3DLineLineDist2", "groups-of-three"])
def test_the_final_least_squares_is_the_public_refinement_of_the_inliers(name):
    """final_least_squares_: pose A and its inliers from a run without it, refined by solve_jointloc_batch over exactly
    those inliers and passed through eh_refine's round trip (est_oracle.pose_round_trip), is bit for bit the pose the
    final record of the run with it implies: its score is the record's, and where the record says applied it is the
    returned pose.  Bit equality held on all three scenes; the fallback of 2^-50 on qvec was not needed."""
    case, on, st = numeric(name, final_least_squares=True)
    _, off, _ = numeric(name, final_least_squares=False)
    sc, cfg = case["scenes"][0], case["cfg"]
    A, inl_p, inl_l = (off["qvec"][0], off["tvec"][0]), *off["stats"][0].inlier_indices
    lc = est._hybrid_options(cfg, None, 1).lineloc_config
    out = hl.solve_jointloc_batch(cfg["line_cost_func"], dict(weight_line=lc.weight_line, weight_point=lc.weight_point,
                                                              loss_function=lc.loss_function),
                                  [dict(l3ds=sc["l3ds"], l3d_ids=sc["l3d_ids"][inl_l], l2ds=sc["l2ds"][inl_l], p3ds=sc["p3ds"][inl_p],
                                        p2ds=sc["p2ds"][inl_p], K=sc["camera"], qvec=A[0], tvec=A[1])], host=True)
    usable = int(out["codes"][0]) <= 2  # IsSolutionUsable; else the pose is kept
    want = eo.pose_round_trip(out["qvec"][0], out["tvec"][0]) if usable else A
    tr = on["trace"][0][:on["istats"][0][11]]
    fin = tr[tr[:, 0] == 2][0]
    assert fin[2] == 1.0 and usable
    assert score_at(sc, cfg, st, np.concatenate(want))["scores"][0] == fin[4], name
    got = (on["qvec"][0], on["tvec"][0])
    print(f"{name}: applied {fin[3]}, refined score {fin[4]!r}, score without {off['dstats'][0][0]!r}, code {out['codes'][0]}")
    for a, b in zip(got, want if fin[3] == 1.0 else A):
        assert a.tobytes() == np.asarray(b, float).tobytes(), (name, a, b)


# ---- 10. the device's configuration matrix on the twin first ----
LOOP_CASES = es.loop_cases()


@pytest.mark.parametrize("case", LOOP_CASES, ids=[c["name"] for c in LOOP_CASES])
def test_the_twin_runs_the_device_matrix(case):
    """every case of tests/test_gpu_est.py's matrix on the twin: finite poses, the decisions replay, and the property
    the case is there for -- the device is never the first to run an input"""
    how = dict(cfg=case["cfg"], seed=case["seed"], loc=case["loc"], **case["fields"])
    full, st = twin_with_sizes(case["scenes"], trace_cap=max(400, case["trace_cap"]), **how)
    assert (full["istats"][:, 11] <= 400).all()
    for q in range(len(case["scenes"])):
        if full["istats"][q][10]:
            replay(full, st, q)
    res = full if case["trace_cap"] >= 400 else run_twin(case["scenes"], trace_cap=case["trace_cap"], **how)[0]
    print(es.case_property(case, res))
    if res is not full:  # a short trace buffer holds the first records, and nothing else changes
        cap = case["trace_cap"]
        for k in ("qvec", "tvec", "dstats", "istats", "inliers"):
            assert res[k].tobytes() == full[k].tobytes(), k
        for q in range(len(case["scenes"])):
            assert res["trace"][q].tobytes() == full["trace"][q][:cap].tobytes()


def test_the_matrix_reaches_the_refinement_configuration():
    """the weight, the loss and the block weights of a case arrive in the refinements: the four (weight, loss) pairs of
    a cost end at four different poses, and the struct holds what the case set"""
    for cost, _ in es.LOOP_COSTS:
        poses = set()
        for case in (c for c in LOOP_CASES if c["name"].startswith(cost + "-w")):
            res, st = run_twin(case["scenes"], cfg=case["cfg"], seed=case["seed"], loc=case["loc"], **case["fields"])
            assert all(getattr(st.loc, k) == v for k, v in case["loc"].items()), case["name"]
            assert st.loc.cost_function == hl.get_lineloc_cost_func(cost)
            poses.add(res["qvec"][0].tobytes() + res["tvec"][0].tobytes())
        assert len(poses) == len(es.LOSS_PAIRS), cost
