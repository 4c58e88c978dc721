"""The minimisers' shared loop (lt_lm.h, DESIGN.md sections 19 and 28) on the host, without a GPU: every named case of
tests/lm_cases.py through the host twins (lt_fn_refine_host, lt_fn_loc_host, lt_fn_ba_host with constant_pose) equals the
NumPy restatement of the loop (tests/lm_oracle.py) bit for bit, ends with its declared code and takes its declared
branches; the damped step alone (lt_fn_lm_step) equals the restated step bit for bit on injected sums and solves the
damped system within the Cholesky backward-error bound; the loop on scripted reductions (lt_fn_lm_loop_script); the
feature term's tracks against the replay; the free-pose bundle adjustment's decisions (lt_fn_ba_host_trace) against the
restated ba_decide_step."""
import ctypes as C

import numpy as np
import pytest

import lm_cases as lc
import lm_oracle as lo
from limap_amd import _capi

p = _capi.ptr
U = 2.0 ** -53


@pytest.fixture(scope="module")
def L():
    return _capi.load_library()


@pytest.fixture(scope="module")
def replays():
    """every case's replay, computed once"""
    return {c.name: lc.replay(c) for c in lc.CASES}


# ---- the replay ----
@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.name)
def test_replay_equals_the_host_twin_bit_for_bit(case, replays):
    host, rep = lc.run_host(case), replays[case.name]
    assert len(host) == len(rep) == 1
    for h, r in zip(host, rep):
        assert lc.same(h, r), (case.name, {k: (h[k], r[k]) for k in lc.FIELDS})


def test_case_table(replays):
    """the declared code and branch set of every case are the replay's, and the cases together take every branch"""
    union = set()
    for c in lc.CASES:
        r = replays[c.name][0]
        b = lo.branches(r, c.cfg["max_num_iterations"])
        assert (r["code"], b) == (c.code, c.branches), c.name
        assert c.cfg["max_num_iterations"] <= 200
        union |= b
    assert lc.BRANCHES <= union, sorted(lc.BRANCHES - union)
    assert not (lc.UNREACHED & union)
    assert {c.code for c in lc.CASES} == set(range(8))
    for kernel, codes in (("refine", {0, 1, 2, 3, 4, 5}), ("refine_terms", {1, 3, 5, 6}), ("loc", {0, 1, 2, 3, 4, 6, 7}), ("ba_point", {0, 1, 2, 3, 4, 6})):
        assert codes <= {c.code for c in lc.CASES if c.kernel == kernel}, kernel
    # the counts the radius exit pins: 15 rejections from 1e4 take the radius below 1e-32, and the exit counts its own
    # iteration; on the cap it is still the radius that is reported, one below the cap it is the cap
    assert [replays[n][0]["iterations"] for n in ("line_radius_cap_14", "line_radius_cap_15", "line_radius_cap_16")] == [14, 15, 15]
    t = replays["line_ordinary"][0]["trace"]
    k = next(i for i in range(1, len(t)) if t[i]["accepted"] and t[i - 1]["accepted"] is False)
    assert t[k]["nu"] > 2.0 and t[k + 1]["nu"] == 2.0


def test_the_solver_evaluates_retracted_quaternions_as_they_are(replays):
    """lt_fn_loc_eval normalises the quaternion it is given, the solver only its input: on the iterates of the ordinary
    pose case the normalisation is not the identity, which is why the replay reads lt_fn_loc_eval_at"""
    case = lc.BY_NAME["pose_ordinary"]
    pr, cfg = case.build(), lc.loc_cfg(**case.cfg)
    seen = []

    def ev(q):
        seen.append(np.array(q[:4]))
        return lc.loc_eval_at(cfg, pr, q)
    p0 = np.concatenate([lo.normalise_q(pr["qvec"]), pr["tvec"]])
    lo.solve("lc_lm", ev, p0, 200, n_blocks=1)
    moved = sum(not np.array_equal(lo.normalise_q(q), q) for q in seen)
    print("iterates whose renormalisation changes bits:", moved, "of", len(seen))
    assert len(seen) > 20 and moved > 0


def test_feature_term_tracks_follow_the_replay():
    """the four tracks of the k_refine_lm_feat workgroup test through lt_fn_refine_host_feature, which runs rf_lm_terms
    over the feature term's group, against the replay over lt_fn_refine_eval_feature"""
    import refine_feature_scenes as fs
    maps, scenes, codes = lc.feat_mix()
    rf = fs.refine_cfg(max_num_iterations=lc.FEAT_ITERATIONS)
    L = _capi.load_library()
    ends = []
    for s, code in zip(scenes, codes):
        h = fs.run(s, rf, "map", maps, host_threads=1)
        grids = {i: (maps[i], np.eye(2), np.zeros(2)) for i in fs.sorted_ids(s, 0)}

        def ev(q, s=s, grids=grids):
            e = fs.eval_ours(s, 0, rf, grids, q)
            return np.float64(e["cost"]), e["g"], e["H"]
        p0 = np.zeros(6)
        assert L.lt_fn_refine_minimal(p(np.ascontiguousarray(s["line6"][0]), C.c_double), p(p0, C.c_double)) == 0
        r = lo.solve("rf_lm_terms", ev, p0, lc.FEAT_ITERATIONS, constant=len(fs.sorted_ids(s, 0)) < 4)
        host = dict(p=h["params"][0], cost0=h["cost"][0, 0], cost1=h["cost"][0, 1], iterations=int(h["iterations"][0]),
                    code=int(h["codes"][0]))
        assert lc.same(host, r), {k: (host[k], r[k]) for k in lc.FIELDS}
        assert code is None or r["code"] == code
        ends.append((r["code"], r["iterations"]))
    print("feature-term tracks end by (code, iterations):", ends)
    assert len(set(ends)) == 4


# ---- the loop on scripted reductions ----
def scripted(L, F, max_iter, costs, accs, p0):
    """lt_fn_lm_loop_script and the restated loop on the same script -> (ours, restated)"""
    costs, accs = np.ascontiguousarray(costs, np.float64), np.ascontiguousarray(accs, np.float64).reshape(-1, 14)
    p3, cost1, it, code, used = np.array(p0, np.float64), np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(2, np.int64)
    rc = L.lt_fn_lm_loop_script(float(F), int(max_iter), len(costs), p(costs, C.c_double), len(accs), p(accs, C.c_double),
                                p(p3, C.c_double), p(cost1, C.c_double), p(it, C.c_int32), p(code, C.c_int32), p(used, C.c_int64))
    assert rc == 0
    n = [0, 0]

    def lin(_):
        a = accs[n[1]]
        n[1] += 1
        H = np.zeros((4, 4))
        H[np.triu_indices(4)] = a[:10]
        return None, a[10:], H + np.triu(H, 1).T

    def cost(_):
        n[0] += 1
        return costs[n[0] - 1]
    r = lo.lm_loop("point", lin, p0, F, max_iter, cost=cost)
    assert n == used.tolist()
    return dict(p=p3, cost0=F, cost1=cost1[0], iterations=int(it[0]), code=int(code[0])), dict(r, cost0=F)


def test_a_ratio_equal_to_the_minimum_rejects_the_step(L):
    """min_relative_decrease is a strict bound: with (F - Fn) / md == 1e-3 exactly the step is rejected"""
    H = np.diag([1.0, 1.0, 1.0, 0.0])
    found = None
    for g0 in np.arange(1.0, 200.0):
        g = np.array([g0, 0.0, 0.0, 0.0])
        rc, dl, md = lo.step(H, g, lo.MU0)
        for F in (np.float64(1e-3) * md, np.nextafter(np.float64(1e-3) * md, 0.0), np.nextafter(np.float64(1e-3) * md, np.inf)):
            if rc == 0 and (F - 0.0) / md == lo.MIN_RATIO:
                found = (g, F)
        if found:
            break
    assert found is not None
    g, F = found
    acc = lo.sums_of(H, g)
    ours_, rest = scripted(L, F, 3, [0.0, 0.5 * F, 0.25 * F, 0.125 * F], [acc] * 4, np.zeros(3))
    t = rest["trace"]
    assert t[0]["ratio"] == lo.MIN_RATIO and t[0]["accepted"] is False and t[1]["mu"] == lo.MU0 / 2 and t[1]["nu"] == 4.0
    assert lc.same(ours_, rest), (ours_, rest)


@pytest.mark.parametrize("seed", range(6))
def test_loop_on_scripted_sums_equals_the_restatement(L, seed):
    """costs that rise and fall against well-posed sums: accepted and rejected steps in an order no scene gives"""
    rng = np.random.default_rng(seed)
    n = 80
    accs = []
    for _ in range(n):
        H = np.zeros((4, 4))
        H[:3, :3] = spd(rng, 3, 10.0 ** rng.uniform(0, 6))
        accs.append(lo.sums_of(H, np.concatenate([rng.normal(size=3), [0.0]])))
    costs = np.exp(-0.1 * np.arange(n)) * (1.0 + 0.4 * rng.normal(size=n))
    ours_, rest = scripted(L, 1.0, [80, 40, 7, 1, 0, 23][seed], costs, accs, rng.normal(size=3))
    assert lc.same(ours_, rest), (ours_, rest)
    if seed == 0:
        b = lo.branches(rest, 80)
        assert {"accept", "reject_then_accept"} <= b, b


def test_a_bad_model_after_an_accepted_step(L):
    """no scene found reaches it: an accepted step, then sums whose model decrease underflows to zero"""
    H = np.diag([1.0, 1.0, 1.0, 0.0])
    g = np.array([1.0, -2.0, 0.5, 0.0])
    tiny = lo.sums_of(H * 1e-200, g * 1e-200)
    ours_, rest = scripted(L, 10.0, 20, [1.0, 0.5], [lo.sums_of(H, g), tiny], np.zeros(3))
    assert rest["code"] == lo.BAD_MODEL and rest["iterations"] == 1
    assert lo.branches(rest, 20) >= {"accept", "bad_model_after_accept"}
    assert lc.same(ours_, rest), (ours_, rest)


# ---- the free-pose bundle adjustment's own decision ----
@pytest.mark.parametrize("name", sorted(lc.BA_SCENES))
def test_free_pose_ba_follows_the_restated_decisions(name):
    """every attempt of the host twin hands (failed factorisation, cost total, model-decrease total) to ba_decide_step;
    the restated decisions on those values give the twin's radius and linearisation flag before every attempt, and its
    iterations, code and final cost"""
    import ba_scenes as bs
    scale, code = lc.BA_SCENES[name]
    s, cfg = lc.ba_scene(scale), bs.cfg_of(**lc.BA_CFG)
    total0, rec, cost, iters, end = lc.ba_trace(s, cfg)
    rc, host = bs.run_host(s, cfg, 2)
    assert rc == 0 and (int(host["iterations"][0]), int(host["code"][0])) == (iters, end) and np.array_equal(host["cost"], cost)
    assert end == code
    st = lo.ba_decide_init(total0, lc.BA_CFG["max_num_iterations"])
    outcomes = []
    for mu, bad, fresh, total, md in rec:
        assert not st["done"] and (st["mu"], st["fresh"]) == (mu, int(fresh))
        if bad < 0:  # the attempt met a zero gradient on a fresh linearisation: no decision
            assert st["fresh"] == 1
            st["done"], st["code"] = 1, lo.ZERO_GRAD
            continue
        st["bad"] = int(bad)
        outcomes.append("failed" if bad else ("accepted" if lo.ba_decide_step(st, total, md) else "rejected"))
        if bad:
            lo.ba_decide_step(st, total, md)
    assert st["done"] and (st["iters"], st["code"]) == (iters, end)
    assert st["F0"] == cost[0] and st["F"] == cost[1]
    if name == "zero_gradient":
        assert iters == 0 and len(rec) == 1
    else:
        assert lc.ba_step_is_nan(s, cfg, 1e4) and outcomes[0] == "failed"
        assert {"failed", "accepted", "rejected"} <= set(outcomes) and iters == len(rec) > 15
        k = outcomes.index("accepted")
        assert outcomes[k - 1] != "accepted" and rec[k + 1][0] > rec[k][0] and st["nu"] > 2.0


# ---- the step alone ----
def ours(L, H, g, mu):
    n = len(g)
    acc = lo.sums_of(H, g)
    dl, md = np.zeros(n), np.zeros(1)
    rc = L.lt_fn_lm_step(n, p(acc, C.c_double), float(mu), p(dl, C.c_double), p(md, C.c_double))
    return rc, dl, md[0]


def agree(L, H, g, mu):
    with np.errstate(all="ignore"):
        rc, dl, md = lo.step(H, g, mu)
    orc, odl, omd = ours(L, H, g, mu)
    assert orc == rc, (rc, orc, mu)
    if rc == lo.BAD_PIVOT:
        assert np.all(np.isnan(odl)) and np.isnan(omd)
    else:
        assert np.array_equal(dl, odl, equal_nan=True) and np.array_equal(md, omd, equal_nan=True), (dl, odl, md, omd)
    return rc


def spd(rng, n, cond, scale=1.0):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    H = (Q * np.geomspace(1.0, 1.0 / cond, n)) @ Q.T * scale
    return (H + H.T) / 2


MUS = [1e-32, 1e-20, 1e-8, 1.0, 1e4, 1e10, 1e16]


@pytest.mark.parametrize("n", [4, 6])
def test_lm_step_equals_the_restatement_bit_for_bit(L, n):
    rng = np.random.default_rng(n)
    codes = []
    for cond in (1.0, 1e3, 1e6, 1e9, 1e12):
        for scale in (1.0, 1e-30, 1e30, 1e140):  # diagonals below 1e-12 and above 1e64: both clamps of the damping
            H, g = spd(rng, n, cond, scale), rng.normal(size=n) * np.sqrt(scale)
            if scale == 1e-30:
                assert np.all(np.sqrt(np.diag(H)) < lo.D_MIN)
            if scale == 1e140:
                assert np.all(np.sqrt(np.diag(H)) > lo.D_MAX)
            for mu in MUS:
                codes.append(agree(L, H, g, mu))
    assert codes.count(0) > len(codes) // 2
    # a zero, negative, infinite and NaN pivot in each position.  Under the damping the first pivot is h + D^2 / mu > 0 for
    # every h >= 0 and finite mu, so its zero needs an infinite radius; a later pivot loses its value to the row above
    base = np.diag(np.arange(1.0, n + 1.0))
    g = rng.normal(size=n)
    for i in range(n):
        for what in ("zero", "negative", "inf", "nan"):
            H, mu = base.copy(), 1e16
            if what == "zero" and i == 0:
                H[0, 0], mu = 0.0, np.inf
            elif what in ("zero", "negative"):
                if i == 0:
                    H[0, 0] = -1.0  # sqrt(-1): the damping is not a number
                else:
                    H[i - 1, i - 1], H[i, i] = 1.0, 4.0
                    H[i - 1, i] = H[i, i - 1] = 2.0 if what == "zero" else 3.0
            else:
                H[i, i] = np.inf if what == "inf" else np.nan
            assert agree(L, H, g, mu) == lo.BAD_PIVOT, (i, what)
        H = base.copy()
        H[i, i] = 1e-300  # a pivot the clamp keeps positive: no failure
        assert agree(L, H, g, 1e4) == 0
    # a model decrease of 0 (g = 0: -0.0 is not positive), infinite and NaN.  dl' (A - H / 2) dl with A = H + D^2 / mu
    # positive definite is positive, so a negative one is not reachable with pivots that pass
    H = spd(rng, n, 10.0)
    assert agree(L, H, np.zeros(n), 1e4) == lo.BAD_MODEL
    assert agree(L, H, np.full(n, 1e200), 1e4) == lo.BAD_MODEL
    assert agree(L, H, np.concatenate([[np.inf], np.ones(n - 1)]), 1e4) == lo.BAD_MODEL
    assert agree(L, H * 1e-200, g * 1e-200, 1e4) == lo.BAD_MODEL  # the decrease underflows to 0
    assert L.lt_fn_lm_step(5, p(np.zeros(20), C.c_double), 1.0, p(np.zeros(5), C.c_double), p(np.zeros(1), C.c_double)) == -1


@pytest.mark.parametrize("n", [4, 6])
def test_lm_step_solves_the_damped_system(L, n):
    """||A dl + g|| <= 4 N (3 N + 1) 2^-53 ||A|| ||dl|| with A = H + D^2 / mu (Higham, Accuracy and Stability of Numerical
    Algorithms, Theorem 10.4: the backward error of a Cholesky solve), and md = -(g' dl + dl' H dl / 2) to a relative
    8 N 2^-53 of the sum of the terms' magnitudes; both evaluated in longdouble, first for the restatement"""
    rng = np.random.default_rng(10 + n)
    ld = np.longdouble
    worst = [0.0, 0.0]
    for cond in (1.0, 1e3, 1e6, 1e9, 1e12):
        for mu in (1e-8, 1.0, 1e4, 1e10, 1e16):
            H, g = spd(rng, n, cond), rng.normal(size=n)
            with np.errstate(all="ignore"):
                rc, dl, md = lo.step(H, g, mu)
            orc, odl, omd = ours(L, H, g, mu)
            assert rc == 0 and orc == 0
            A = H.astype(ld)
            for i in range(n):
                d = min(max(np.sqrt(ld(H[i, i])), ld(lo.D_MIN)), ld(lo.D_MAX))
                A[i, i] = ld(H[i, i]) + d * d / ld(mu)
            normA = float(np.linalg.norm(A.astype(np.float64), 2))
            for x, m in ((dl, md), (odl, omd)):
                res = float(np.sqrt(np.sum((A @ x.astype(ld) + g.astype(ld)) ** 2)))
                bound = 4 * n * (3 * n + 1) * U * normA * float(np.linalg.norm(x))
                worst[0] = max(worst[0], res / bound)
                assert res <= bound, (cond, mu, res, bound)
                xl, Hl, gl = x.astype(ld), H.astype(ld), g.astype(ld)
                exact = -(np.sum(gl * xl) + ld(0.5) * (xl @ Hl @ xl))
                mag = np.sum(np.abs(gl * xl)) + ld(0.5) * np.sum(np.abs(xl[:, None] * Hl * xl[None, :]))
                worst[1] = max(worst[1], float(abs(ld(m) - exact) / (8 * n * U * mag)))
                assert abs(ld(m) - exact) <= 8 * n * U * mag, (cond, mu)
    print(f"lm_step<{n}>: residual at most {worst[0]:.3g} of its bound, model decrease at most {worst[1]:.3g} of its bound")
