"""-m gpu: the decisions of candidate generation at their thresholds and bands (cases: tests/gate_cases.py, whose
predictions tests/test_gate_cases_host.py asserts on the CPU oracle).

End to end: every case of the families U (one ulp), B (bands), R (regimes) and C (conditioning) against
OracleTriangulator, in every generation form -- line slots, row slots (LT_GEN_ROW_SLOTS=1), rows permuted inside a block,
exhaustive matching, and use_endpoints_triangulation for the gates of stage B -- and each form again with the fast gates
switched off (LT_TEST_NO_FAST_GATES=1), which must not change a bit.

Direct (with the test switches out of the environment: LT_TEST_NO_FAST_GATES opens the bands of sensitivity3 in the
context's configuration): lt_fn_gate_outcomes evaluates every decision function on the same connections; the three-way gates may only
decide what the reference-exact expressions decide, the IoU is the oracle's bit for bit, and the exact stage-A gate is
the reference's decision on the oracle's values.

The only tolerance is helpers.compare_candidates' 1e-12 on scores (acos / exp); decisions, candidate sets, coordinates
and IoU bits are exact.  No threshold comes nearer than 1e-10 relative to a value that passes through acos."""
import os

import numpy as np
import pytest

import gate_cases as gc
from helpers import compare_best, compare_candidates, compare_valid_edges

pytestmark = pytest.mark.gpu

FORMS = ("line_slots", "row_slots", "permuted", "exhaustive")
_ENV = ("LT_TEST_NO_FAST_GATES", "LT_GEN_ROW_SLOTS")


@pytest.fixture
def env_clean():
    saved = {k: os.environ.pop(k, None) for k in _ENV}
    yield
    for k in _ENV:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


def _feed(T, case, exhaustive, init):
    sc = case.scene
    if sc.ranges is not None:
        T.SetRanges(sc.ranges)
    init(T)
    for i in (sc.img_ids if case.images is None else case.images):
        if exhaustive:
            T.TriangulateImageExhaustiveMatch(int(i), sc.neighbors[int(i)])
        else:
            T.TriangulateImage(int(i), case.matches_of(i))
    return T


def _device(case, exhaustive):
    from limap_amd import triangulation as tri
    sc = case.scene
    T = _feed(tri.GlobalLineTriangulator(case.cfg), case, exhaustive,
              lambda T: T.InitArrays(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, [sc.segs_of(i) for i in range(sc.n_images)]))
    ctx = T.context()
    return ctx.get_all_tris(), ctx.get_best(), ctx.get_valid_edges(), ctx.timers()["line_slots"]


def _oracle(oracle, case, exhaustive):
    sc = case.scene
    O = _feed(oracle.OracleTriangulator(case.cfg, faithful=False), case, exhaustive,
              lambda O: O.Init(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, sc.seg_off, sc.segs))
    return O.get_all_tris(), O.get_best(), O.get_valid_edges()


def _end_to_end(oracle, case, forms=FORMS):
    """The case in each form against the oracle, and again without the fast gates: bit for bit the same candidates."""
    for form in forms:
        c = gc.permuted(case) if form == "permuted" else case
        ex = form == "exhaustive"
        want = _oracle(oracle, c, ex)
        if form == "row_slots":
            os.environ["LT_GEN_ROW_SLOTS"] = "1"
        try:
            fast = _device(c, ex)
            os.environ["LT_TEST_NO_FAST_GATES"] = "1"
            exact = _device(c, ex)
        finally:
            os.environ.pop("LT_TEST_NO_FAST_GATES", None)
            os.environ.pop("LT_GEN_ROW_SLOTS", None)
        try:
            compare_candidates(fast[0], want[0])
            compare_best(fast[1], want[1])
            compare_valid_edges(fast[2], want[2])
            for k in ("off", "src", "line", "score"):
                assert np.array_equal(fast[0][k], exact[0][k]), f"all_tris[{k}] changes without the fast gates"
            # the run took the form it is meant to test (timers["line_slots"]: 1 when stage A ran in the line-slot form;
            # the exhaustive mode has kernels of its own)
            if not ex:
                ln = 1.0 if form == "line_slots" else 0.0
                assert fast[3] == ln and exact[3] == ln, f"stage A ran with line_slots = {fast[3]}, {exact[3]}"
            if case.target is not None:
                n = gc.is_member(fast[0], c.scene, c.target)
                assert n == (1 if case.keep else 0), f"the device holds the target {n} times, the oracle keeps it: {case.keep}"
        except AssertionError as e:
            raise AssertionError(f"case {case.name}, form {form}: {e}") from e


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", gc.U_GATES)
def test_one_ulp_end_to_end(gpu_lib, oracle, env_clean, gate):
    for case in gc.family_u(oracle, gate):
        _end_to_end(oracle, case)


@pytest.mark.parametrize("gate", gc.RANGE_GATES)
def test_one_ulp_end_to_end_endpoint_triangulation(gpu_lib, oracle, env_clean, gate):
    for case in gc.family_u(oracle, gate, by_endpoints=True):
        _end_to_end(oracle, case, forms=("line_slots", "exhaustive"))


@pytest.mark.parametrize("sign", ["below", "above"])
@pytest.mark.parametrize("gate", gc.B_GATES)
def test_bands_end_to_end(gpu_lib, oracle, env_clean, gate, sign):
    cases = [c for c in gc.family_b(oracle, gate) if ("-+" in c.name) == (sign == "above")]
    assert len(cases) == gc.N_TARGETS * len(gc.DELTAS)
    for case in cases:
        _end_to_end(oracle, case)


@pytest.mark.parametrize("sign", ["below", "above"])
def test_bands_end_to_end_endpoint_triangulation(gpu_lib, oracle, env_clean, sign):
    cases = [c for c in gc.family_b(oracle, "sens", by_endpoints=True) if ("-+" in c.name) == (sign == "above")]
    assert len(cases) == gc.N_TARGETS * len(gc.DELTAS)
    for case in cases:
        _end_to_end(oracle, case, forms=("line_slots", "exhaustive"))


@pytest.mark.parametrize("key", ["line_tri_angle_threshold", "sensitivity_threshold", "min_length_2d", "IoU_threshold"])
def test_regimes_end_to_end(gpu_lib, oracle, env_clean, key):
    cases = gc.family_r(key)
    assert len(cases) in (8, 3, 4)
    for case in cases:
        _end_to_end(oracle, case)
        if key == "sensitivity_threshold":
            import dataclasses
            ep = dataclasses.replace(case, cfg=dict(case.cfg, use_endpoints_triangulation=True))
            _end_to_end(oracle, ep, forms=("line_slots",))


@pytest.mark.parametrize("offset", gc.OFFSETS)
def test_conditioning_end_to_end(gpu_lib, oracle, env_clean, offset):
    import dataclasses
    case = gc.family_c(offset)
    _end_to_end(oracle, case)
    ep = dataclasses.replace(case, cfg=dict(case.cfg, use_endpoints_triangulation=True))
    _end_to_end(oracle, ep, forms=("line_slots", "exhaustive"))


# ---------------------------------------------------------------------------------------------------------------
# direct, through lt_fn_gate_outcomes
# ---------------------------------------------------------------------------------------------------------------
def _outcomes(cfg, ranges, c30):
    from limap_amd import _capi
    ctx = _capi.Context(cfg_dict=cfg)
    try:
        if ranges is not None:
            ctx.set_ranges(*ranges)
        return ctx.fn_gate_outcomes(c30)
    finally:
        ctx.close()


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _check_outcomes(out, v, cfg, ranges, what, check_tri=None):
    """The properties every connection must have, whatever the thresholds."""
    fast, exact = out["fast"], out["exact"]
    assert set(np.unique(fast)) <= {0, 1, 2} and set(np.unique(exact)) <= {0, 1}
    bad = np.nonzero(((fast == 0) & (exact != 0)) | ((fast == 1) & (exact != 1)))[0]
    assert bad.size == 0, f"{what}: gate3 decided against gen_gates at connections {bad[:8]}: fast {fast[bad[:8]]}"
    tri = out["tri_ok"] == 1
    for view in ("1", "2"):
        s3, gt = out["sens3_" + view], out["sens_gt_" + view]
        assert np.all(s3[~tri] == -1) and set(np.unique(s3[tri])) <= {0, 1, 2}
        bad = np.nonzero(tri & (((s3 == 1) & (gt != 1)) | ((s3 == 0) & (gt != 0))))[0]
        assert bad.size == 0, f"{what}: sensitivity3 decided against sensitivity_gt in view {view} at {bad[:8]}"
    bad = np.nonzero((out["pretest"] == 0) & (out["finish"] != 0))[0]
    assert bad.size == 0, f"{what}: gen_pretest is false where gen_finish is true at {bad[:8]}"
    # the IoU is the oracle's, bit for bit (two NaNs count as equal)
    dev = out["iou_bits"].view(np.float64)
    same = (out["iou_bits"] == _bits(v["iou"])) | (np.isnan(dev) & np.isnan(v["iou"]))
    assert np.all(same), f"{what}: IoU bits differ at {np.nonzero(~same)[0][:8]}"
    # the exact stage-A gate is the reference's decision, except within 1e-10 of an angle threshold (acos)
    ref = gc.stage_a_reference(v, cfg)
    clear = gc.angle_clearance(v, cfg) >= 1e-10
    bad = np.nonzero(clear & (exact != ref))[0]
    assert bad.size == 0, f"{what}: gen_gates differs from the reference decision at {bad[:8]}"
    # the triangulation succeeds where the oracle's does (all connections, or the given ones)
    sel = np.ones(len(fast), bool) if check_tri is None else check_tri
    bad = np.nonzero(sel & (tri != v["tri_ok"]))[0]
    assert bad.size == 0, f"{what}: the triangulation's success differs from the oracle's at {bad[:8]}"
    # stage B as a whole, away from the sensitivity threshold by 1e-10
    th = cfg["sensitivity_threshold"]
    with np.errstate(invalid="ignore"):
        near = (np.abs(v["sens1"] - th) < 1e-10 * abs(th)) | (np.abs(v["sens2"] - th) < 1e-10 * abs(th))
    bad = np.nonzero(sel & ~near & ((out["finish"] == 1) != gc.stage_b_reference(v, cfg, ranges)))[0]
    assert bad.size == 0, f"{what}: gen_finish differs from the reference's stage B at {bad[:8]}"


def _counts(x):
    return [int(np.count_nonzero(x == k)) for k in (0, 1, 2)]


def _report(family, fast, s3):
    # a record for DESIGN.md section 5 (not a bar): run with -s to see it
    print(f"GATE-COUNTS {family}: fast 0/1/2 = {_counts(fast)}, sensitivity3 0/1/2 = {_counts(s3)}")


def test_outcomes_base_scene(gpu_lib, oracle, env_clean):
    """Every match row of the base scene under the default thresholds."""
    for ep in (False, True):
        _, c30, v, _, _ = gc.base_table(oracle, ep)
        cfg = gc.base_cfg(use_endpoints_triangulation=ep)
        out = _outcomes(cfg, gc.base_scene().ranges, c30)
        _check_outcomes(out, v, cfg, gc.base_scene().ranges, f"base scene, endpoints={ep}")
        if not ep:
            assert {0, 1} <= set(np.unique(out["fast"])), "the fast gate decides nothing"
            _report("base", out["fast"], np.r_[out["sens3_1"], out["sens3_2"]])


def _family_outcomes(oracle, cases, by_endpoints, what):
    """Every case's thresholds on all connections of the base scene; -> the three-way values of the targets."""
    conns, c30, v, _, _ = gc.base_table(oracle, by_endpoints)
    fast, s3 = [], []
    for c in cases:
        out = _outcomes(c.cfg, c.scene.ranges, c30)
        _check_outcomes(out, v, c.cfg, c.scene.ranges, f"{what} {c.name}")
        t = int(np.nonzero((conns == np.array(c.target)).all(axis=1))[0][0])
        fast.append(out["fast"][t])
        # the view whose sensitivity is the smaller one is the one the threshold sits on
        s3.append(out["sens3_1"][t] if v["sens1"][t] <= v["sens2"][t] else out["sens3_2"][t])
        # the exact decisions follow the oracle on the target itself
        if c.name.split("-")[0] in ("iou", "len1", "len2", "angle"):
            assert out["exact"][t] == (1 if c.keep else 0), f"{what} {c.name}: gen_gates on the target"
        else:
            assert out["exact"][t] == 1 and out["finish"][t] == (1 if c.keep else 0), f"{what} {c.name}: gen_finish on the target"
    return np.array(fast), np.array(s3)


@pytest.mark.parametrize("gate", gc.U_GATES)
def test_outcomes_one_ulp(gpu_lib, oracle, env_clean, gate):
    """... and a threshold within one ulp of the target's IoU or length is inside the gate's error budget (1e-7 on the IoU
    decision, 1e-12 on the squared length): gate3 must leave the target to the exact expression."""
    fast, s3 = _family_outcomes(oracle, gc.family_u(oracle, gate), False, "U")
    _report(f"U {gate}", fast, s3)
    if gate in ("iou", "len1", "len2"):
        assert np.all(fast == 2), f"gate3 decided a target one ulp from its {gate} threshold: {fast}"
    if gate in gc.RANGE_GATES:
        _family_outcomes(oracle, gc.family_u(oracle, gate, by_endpoints=True), True, "U endpoints")


@pytest.mark.parametrize("gate", gc.B_GATES)
def test_outcomes_bands(gpu_lib, oracle, env_clean, gate):
    """... and the three-way gate of the banded threshold takes each of its values on the targets: it decides outside the
    band, on either side, and leaves the inside to the exact expression."""
    cases = gc.family_b(oracle, gate)
    inside = np.array([c.delta <= gc.BAND_INSIDE for c in cases])
    fast, s3 = _family_outcomes(oracle, cases, False, "B")
    _report(f"B {gate}", fast, s3)
    if gate == "angle":
        assert set(np.unique(fast)) == {0, 1, 2}, f"gate3 on the angle targets: 0/1/2 = {_counts(fast)}"
        assert np.all(fast[inside] == 2), "gate3 decided a target inside the 1e-7 band of the angle threshold"
    elif gate == "iou":
        # |num - th den| = num delta <= delta < 1e-7 <= the margin (gate_cases.family_b): undecided, whatever the geometry
        assert np.all(fast[inside] == 2), "gate3 decided a target whose IoU is inside the 1e-7 margin of its threshold"
    else:
        assert set(np.unique(s3)) == {0, 1, 2}, f"sensitivity3 on the sensitivity targets: 0/1/2 = {_counts(s3)}"
        assert np.all(s3[inside] == 2), "sensitivity3 decided a target inside the 1e-7 band of the sensitivity threshold"
        _, s3e = _family_outcomes(oracle, gc.family_b(oracle, gate, by_endpoints=True), True, "B endpoints")
        assert set(np.unique(s3e)) == {0, 1, 2} and np.all(s3e[inside] == 2)


@pytest.mark.parametrize("key", ["line_tri_angle_threshold", "sensitivity_threshold", "min_length_2d", "IoU_threshold"])
def test_outcomes_regimes(gpu_lib, oracle, env_clean, key):
    _, c30, v, _, _ = gc.base_table(oracle)
    for c in gc.family_r(key):
        out = _outcomes(c.cfg, c.scene.ranges, c30)
        _check_outcomes(out, v, c.cfg, c.scene.ranges, f"R {c.name}")
        _report(f"R {c.name}", out["fast"], np.r_[out["sens3_1"], out["sens3_2"]])


def test_outcomes_conditioning(gpu_lib, oracle, env_clean):
    fast, s3 = [], []
    for offset in gc.OFFSETS:
        c = gc.family_c(offset)
        rows = [t for fam in gc.C_FAMILIES for t in c.families[fam]]
        c30 = gc.conn30(c.scene, np.array(rows))
        v = gc.oracle_values(oracle, c30)
        out = _outcomes(c.cfg, c.scene.ranges, c30)
        # the success of the triangulation is compared where it can be observed: behind the reference's stage A
        _check_outcomes(out, v, c.cfg, c.scene.ranges, f"C offset {offset:g}", check_tri=gc.stage_a_reference(v, c.cfg))
        fast.append(out["fast"])
        s3 += [out["sens3_1"], out["sens3_2"]]
        if offset == 0.0:
            # min_length_2d == 0: the band is the single point q == 0 (make_gen: only q == 0 has length <= 0), which a
            # zero-length segment hits exactly, without rounding -- the fast gate itself rejects it.  With the IoU gate
            # opened (a point's epipolar overlap is 0) the length is the only gate that can
            zero = np.array(c.families["zero_l1"] + c.families["zero_l2"])
            cfg0 = dict(c.cfg, IoU_threshold=-1.0)
            out0 = _outcomes(cfg0, c.scene.ranges, gc.conn30(c.scene, zero))
            assert cfg0["min_length_2d"] == 0.0
            assert np.all(out0["fast"] == 0) and np.all(out0["exact"] == 0), f"zero-length segments: fast {out0['fast']}"
    _report("C", np.concatenate(fast), np.concatenate(s3))


def test_gate_outcomes_validates_its_arguments(gpu_lib, env_clean):
    import ctypes as C
    from limap_amd import _capi
    ctx = _capi.Context(cfg_dict=gc.base_cfg())
    out, bits, conn = np.zeros((1, 10), np.int32), np.zeros(1, np.uint64), np.zeros((1, 30))
    p = _capi.ptr
    L = ctx.L
    assert L.lt_fn_gate_outcomes(ctx.h, 0, None, None, None) == 0
    for n, a, b, c in ((-1, conn, out, bits), (1, None, out, bits), (1, conn, None, bits), (1, conn, out, None),
                       ((1 << 24) + 1, conn, out, bits)):
        rc = L.lt_fn_gate_outcomes(ctx.h, n, None if a is None else p(a, C.c_double), None if b is None else p(b, C.c_int32),
                                   None if c is None else p(c, C.c_uint64))
        assert rc == -2 and b"lt_fn_gate_outcomes" in L.lt_last_error(ctx.h)
    assert ctx.fn_gate_outcomes(np.zeros((0, 30)))["fast"].shape == (0,)
    ctx.close()
