"""CPU: the cases of tests/gate_cases.py do what they claim, on the oracle alone.  A case predicts whether the oracle keeps
its target connection as a candidate; only where these predictions hold do the device tests of test_gpu_gate_edges.py
sit on the thresholds they mean to sit on."""
import numpy as np
import pytest

import gate_cases as gc
from helpers import run_oracle


def _run(oracle, case):
    O = oracle.OracleTriangulator(case.cfg, faithful=False)
    sc = case.scene
    if sc.ranges is not None:
        O.SetRanges(sc.ranges)
    O.Init(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, sc.seg_off, sc.segs)
    for i in (sc.img_ids if case.images is None else case.images):
        O.TriangulateImage(int(i), case.matches_of(i))
    return O.get_all_tris()


def _check_targets(oracle, cases, n_expected):
    assert len(cases) == n_expected
    kept = 0
    for c in cases:
        n = gc.is_member(_run(oracle, c), c.scene, c.target)
        assert n == (1 if c.keep else 0), f"{c.name}: the oracle holds the target {n} times, predicted keep={c.keep}"
        kept += n
    assert 0 < kept < len(cases)


@pytest.mark.parametrize("gate", gc.U_GATES)
def test_family_u_targets_flip_at_one_ulp(oracle, gate):
    """pred(v), v, succ(v) of N_TARGETS connections: the oracle's candidate set contains the target exactly as predicted."""
    _check_targets(oracle, gc.family_u(oracle, gate), 3 * gc.N_TARGETS)


@pytest.mark.parametrize("gate", gc.RANGE_GATES)
def test_family_u_ranges_with_endpoint_triangulation(oracle, gate):
    _check_targets(oracle, gc.family_u(oracle, gate, by_endpoints=True), 3 * gc.N_TARGETS)


@pytest.mark.parametrize("gate,by_endpoints", [("angle", False), ("sens", False), ("sens", True), ("iou", False)])
def test_family_b_targets_flip_across_the_bands(oracle, gate, by_endpoints):
    """v (1 +- delta) down to delta = 1e-10: the oracle decides as predicted from the generator's value, which therefore
    lies within 1e-10 relative of the value the oracle compares (for the angle: glibc's acos through math.acos on the
    oracle's normal and ray against the oracle's own evaluation inside triangulateOneNode)."""
    cases = gc.family_b(oracle, gate, by_endpoints)
    assert min(gc.DELTAS) == 1e-10
    _check_targets(oracle, cases, 2 * len(gc.DELTAS) * gc.N_TARGETS)
    # the thresholds stay inside the interval in which the bands are built
    if gate != "iou":
        key = "line_tri_angle_threshold" if gate == "angle" else "sensitivity_threshold"
        assert all(1e-3 < c.cfg[key] < 89.0 for c in cases)


def test_family_b_sensitivity_value_is_the_oracles(oracle):
    """The sensitivity of family B is Line3d::sensitivity of the oracle itself on the oracle's own triangulation: the
    candidate store holds the same line bit for bit."""
    conns, _, v, kept, ok = gc.base_table(oracle)
    sc = gc.base_scene()
    allt = run_oracle(oracle, sc, gc.base_cfg()).get_all_tris()
    for t in np.nonzero(ok)[0][::40]:
        i, a, j, b = conns[t]
        g = int(sc.seg_off[i]) + a
        rows = slice(allt["off"][g], allt["off"][g + 1])
        hit = np.nonzero((allt["src"][rows, 0] == sc.img_ids[j]) & (allt["src"][rows, 1] == b))[0]
        assert len(hit) == 1
        assert np.array_equal(allt["line"][rows][hit[0], :8], v["line"][t, :8])


@pytest.mark.parametrize("by_endpoints", [False, True])
def test_reference_decisions_reproduce_the_candidate_set(oracle, by_endpoints):
    """Stage A as restated in gate_cases.stage_a_reference (lengths > min_length_2d, both angles >= th, not IoU < th) is
    the oracle's candidate membership on the base scene once stage B's gates are opened (sensitivity threshold 90, no
    ranges), wherever the triangulation succeeds; with stage B as restated, it is the membership under the defaults."""
    import dataclasses
    conns, _, v, kept, _ = gc.base_table(oracle, by_endpoints)
    over = dict(use_endpoints_triangulation=True) if by_endpoints else {}
    sc = gc.base_scene()
    assert 300 <= kept.sum() <= len(conns) - 300
    for cfg, scene, want in ((gc.base_cfg(sensitivity_threshold=90.0, **over), dataclasses.replace(sc, ranges=None),
                              gc.stage_a_reference(v, gc.base_cfg()) & v["tri_ok"]),
                             (gc.base_cfg(**over), sc, kept)):
        allt = run_oracle(oracle, scene, cfg).get_all_tris()
        have = set()
        for g in range(len(allt["off"]) - 1):
            for s in allt["src"][allt["off"][g]:allt["off"][g + 1]]:
                have.add((g, int(s[0]), int(s[1])))
        mine = {(int(sc.seg_off[i]) + int(a), int(sc.img_ids[j]), int(b)) for (i, a, j, b), w in zip(conns, want) if w}
        assert have == mine
        # duplicates of a row are stored once each: the counts agree too
        assert int(allt["off"][-1]) == int(np.count_nonzero(want))


def test_base_scene_sits_on_both_sides_of_every_default_gate(oracle):
    _, _, v, kept, ok = gc.base_table(oracle)
    cfg = gc.base_cfg()
    sc = gc.base_scene()
    with np.errstate(invalid="ignore"):
        for below in (v["ang"] < cfg["line_tri_angle_threshold"], v["iou"] < cfg["IoU_threshold"], ~v["tri_ok"],
                      v["sens"] > cfg["sensitivity_threshold"],
                      gc.stage_b_reference(v, cfg, None) & ~gc.stage_b_reference(v, cfg, sc.ranges)):
            assert 50 <= np.count_nonzero(below) <= len(below) - 50
    assert kept.sum() >= 300 and ok.sum() >= 200


def test_family_r_regimes_on_the_oracle(oracle):
    """The outcomes family_r's docstring names."""
    counts = {}
    for c in gc.family_r():
        counts[c.name] = int(_run(oracle, c)["off"][-1])
    default = int(_run(oracle, gc.Case("default", gc.base_scene(), gc.base_cfg(), images=gc.family_r()[0].images))["off"][-1])
    assert default > 100
    for name in ("line_tri_angle_threshold=90.0", "line_tri_angle_threshold=120.0", "IoU_threshold=2.0"):
        assert counts[name] == 0, name
    for name in ("line_tri_angle_threshold=-1.0", "line_tri_angle_threshold=0.0", "IoU_threshold=-1.0", "IoU_threshold=0.0"):
        assert counts[name] > default, name
    assert counts["sensitivity_threshold=90.0"] == counts["sensitivity_threshold=120.0"] >= default
    for name in ("min_length_2d=-1.0", "min_length_2d=0.0", "min_length_2d=5e-324"):
        assert counts[name] == default, name
    for name in ("sensitivity_threshold=-1.0", "sensitivity_threshold=0.0", "sensitivity_threshold=0.001"):
        assert counts[name] < default, name
    assert len(counts) == len(gc.R_SWITCHES) == 23


@pytest.mark.parametrize("offset", gc.OFFSETS)
def test_family_c_runs_through_the_oracle(oracle, offset):
    """Every degenerate family at this offset goes through the oracle without an error; the scene keeps some connections
    and rejects others, and the families the docstring calls rejected are."""
    c = gc.family_c(offset)
    sc = c.scene
    assert sc.n_images == 6 and len(sc.segs) <= 300
    # every block is regular -- its lines ascend in steps of 0 or +1 -- so that the upload can take the line-slot form
    for i in range(sc.n_images):
        for rows in c.matches_of(i).values():
            assert set(np.diff(rows[:, 0]).tolist()) <= {0, 1}
    allt = _run(oracle, c)
    member = {k: [gc.is_member(allt, sc, t) for t in rows] for k, rows in c.families.items()}
    n_rows = sum(len(r) for r in c.families.values())
    assert 0 < int(allt["off"][-1]) < n_rows
    for k, rows in c.families.items():
        want = gc.C_OUTCOME[k]
        want = want(offset) if callable(want) else want
        if want == "all":
            assert sum(member[k]) == len(rows), k
        elif want == "none":
            assert sum(member[k]) == 0, k
        else:
            assert sum(member[k]) > 0, k
    assert np.all(np.isfinite(allt["line"][:, :6]))
    # the values the families are about: a NaN normal and a NaN IoU for a zero-length l2, an angle of exactly zero
    v = gc.oracle_values(oracle, gc.conn30(sc, np.array(c.families["zero_l2"] + c.families["in_plane"])))
    assert (v["ang"][3:] == 0.0).all()
    if offset == 0.0:
        assert np.isnan(v["iou"][:3]).all()
