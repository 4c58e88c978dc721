"""Cases that put the decisions of candidate generation on their thresholds ("Gate edges").

Candidate generation is where the device does not run the reference's arithmetic: the three-way gates (gate3,
sensitivity3) and the stage-B pre-test decide a connection only where the reference's outcome is certain, and hand
everything else to the reference-exact expressions.  The generators below build, from the CPU oracle's own values,
configurations in which a chosen connection ("target") lies one ulp from a threshold (family U), inside or outside the
1e-7 bands around a threshold that passes through acos (family B), at the switches of the band construction (family R),
or in badly conditioned geometry (family C).  Every prediction made here is asserted on the CPU oracle by
tests/test_gate_cases_host.py before tests/test_gpu_gate_edges.py holds the device against it.

All values come from the oracle's free functions and from OracleTriangulator.get_all_tris(); NumPy only computes the
2D segment length (the reference's own expression, norm(start - end)) and the ray/plane angle from the oracle's normal and
ray (the reference's own expression, 90 - acos(|n . r|) 180 / pi, with glibc's acos through math.acos).
"""
import dataclasses
import functools
import math

import numpy as np

from limap_amd import synthetic as syn

# The smallest seeded scene found that has a few hundred candidates, connections on either side of each of the default
# gates that can reject, and images with more than one neighbour: 3200 connections, 572 candidates; 137 below the angle
# threshold, 2057 below the IoU threshold, 1622 not triangulated, 95 too sensitive in both views, 248 outside the ranges
# (4 x 30 x 2 gives no connection at all, 5 x 40 x 3 fewer than 170 candidates; seed 1 of this shape is
# three isolated pairs of images).
BASE_SHAPE = dict(n_views=6, n_segs=40, n_neighbors=3, seed=4)
# relative distances from an acos threshold: inside (<= 5e-8) and outside (>= 2e-7) the 1e-7 (+1e-9) bands, on both sides.
# Never below 1e-10: nearer than that the device's acos against glibc's may decide, which is not this project's arithmetic.
DELTAS = (1e-10, 1e-8, 5e-8, 2e-7, 1e-6, 1e-4)
BAND_INSIDE = 5e-8  # deltas up to this one are inside every band
OFFSETS = (0.0, 1e-12, 1e-9, 1e-6, 1e-3)
N_TARGETS = 3
RANGE_GATES = tuple(f"{b}_{'xyz'[k]}_{e}" for b in ("lo", "hi") for k in range(3) for e in ("start", "end"))
U_GATES = ("iou", "len1", "len2") + RANGE_GATES
B_GATES = ("angle", "sens", "iou")
STAGE_B_GATES = RANGE_GATES + ("sens",)  # decided after the triangulation: also run with use_endpoints_triangulation


@functools.lru_cache(maxsize=None)
def base_scene():
    return syn.make_scene(**BASE_SHAPE)


def base_cfg(**over):
    return syn.default_triangulation_cfg(debug_mode=True, **over)


@dataclasses.dataclass
class Case:
    """One configuration: `scene` (its .ranges are the case's ranges) triangulated for `images` with `cfg`; the oracle
    holds the connection `target` = (img idx, line, neighbour idx, neighbour line) as a candidate iff `keep`."""
    name: str
    scene: object
    cfg: dict
    images: tuple = None
    target: tuple = None
    keep: bool = None
    matches: dict = None  # img id -> matches dict; None: the scene's own (scene.matches_of)
    delta: float = None   # family B: the relative distance of the threshold from the target's value
    families: dict = None  # family C: family -> its connections (view, line, neighbour, neighbour line)

    def matches_of(self, img_id):
        return self.scene.matches_of(int(img_id)) if self.matches is None else self.matches[int(img_id)]


# ---------------------------------------------------------------------------------------------------------------
# connections and the oracle's values of them
# ---------------------------------------------------------------------------------------------------------------
def connections(scene, matches_of=None, images=None):
    """Every match row of the scene as (image idx, line, neighbour idx, neighbour line), in processing order."""
    rows = []
    ids = [int(i) for i in scene.img_ids]
    for n, i in enumerate(ids):
        if images is not None and i not in images:
            continue
        m = (matches_of or scene.matches_of)(i)
        for nb, r in m.items():
            r = np.asarray(r).reshape(-1, 2)
            j = ids.index(int(nb))
            rows.append(np.stack([np.full(len(r), n), r[:, 0], np.full(len(r), j), r[:, 1]], 1))
    return np.concatenate(rows, 0).astype(np.int64) if rows else np.zeros((0, 4), np.int64)


def conn30(scene, conns):
    """(n, 30) seg1[4] cam1[11] seg2[4] cam2[11]: the input of lt_fn_gate_outcomes."""
    out = np.zeros((len(conns), 30))
    for k, (i, a, j, b) in enumerate(conns):
        out[k, 0:4] = scene.segs_of(i)[a]
        out[k, 4:15] = scene.cam11(i)
        out[k, 15:19] = scene.segs_of(j)[b]
        out[k, 19:30] = scene.cam11(j)
    return out


def seg_length(seg):
    """Line2d::length(): norm(start - end), the reference's expression."""
    dx, dy = seg[0] - seg[2], seg[1] - seg[3]
    return math.sqrt(dx * dx + dy * dy)


def _angle(ora, n2, cam1, p):
    """90 - acos(|n2 . ray|) 180 / pi (base_line_triangulator.cc:293-302) from the oracle's normal and ray."""
    r = ora.cam_ray_direction(cam1, p)
    d = abs((n2[0] * r[0] + n2[1] * r[1]) + n2[2] * r[2])
    try:
        return 90 - math.acos(d) * 180.0 / math.pi
    except ValueError:  # |d| > 1 by rounding, or NaN: the reference's acos gives NaN
        return float("nan")


def oracle_values(ora, c30, by_endpoints=False):
    """The oracle's value of everything a gate compares, per connection of c30 (n, 30)."""
    n = len(c30)
    v = dict(len1=np.zeros(n), len2=np.zeros(n), ang_s=np.zeros(n), ang_e=np.zeros(n), iou=np.zeros(n),
             tri_ok=np.zeros(n, bool), line=np.zeros((n, 10)), sens1=np.full(n, np.nan), sens2=np.full(n, np.nan))
    tri = ora.triangulate_line_by_endpoints if by_endpoints else ora.triangulate_line
    with np.errstate(all="ignore"):
        for k in range(n):
            s1, c1, s2, c2 = c30[k, 0:4], c30[k, 4:15], c30[k, 15:19], c30[k, 19:30]
            v["len1"][k], v["len2"][k] = seg_length(s1), seg_length(s2)
            n2 = ora.get_normal_direction(s2, c2)
            v["ang_s"][k], v["ang_e"][k] = _angle(ora, n2, c1, s1[0:2]), _angle(ora, n2, c1, s1[2:4])
            v["iou"][k] = ora.compute_epipolar_IoU(s1, c1, s2, c2)
            line = tri(s1, c1, s2, c2)
            v["line"][k] = line
            v["tri_ok"][k] = line[9] > 0
            if v["tri_ok"][k]:
                v["sens1"][k], v["sens2"][k] = ora.line3d_sensitivity(line, c1), ora.line3d_sensitivity(line, c2)
    v["ang"] = np.fmin(v["ang_s"], v["ang_e"])
    v["sens"] = np.fmin(v["sens1"], v["sens2"])
    return v


def stage_a_reference(v, cfg):
    """The reference's stage-A decision (base_line_triangulator.cc:166,177,293-307) on the oracle's values: lengths
    > min_length_2d, both angles >= th, not IoU < th -- each written as the negation of the reference's own skip test,
    which is the same thing except for a NaN (the reference does not skip on one)."""
    with np.errstate(invalid="ignore"):
        keep = ~(v["len1"] <= cfg["min_length_2d"]) & ~(v["len2"] <= cfg["min_length_2d"])
        keep &= ~(v["ang_s"] < cfg["line_tri_angle_threshold"]) & ~(v["ang_e"] < cfg["line_tri_angle_threshold"])
        keep &= ~(v["iou"] < cfg["IoU_threshold"])
    return keep


def angle_clearance(v, cfg):
    """Relative distance of the nearer endpoint angle from the angle threshold (inf for th == 0 or a NaN angle)."""
    th = cfg["line_tri_angle_threshold"]
    with np.errstate(all="ignore"):
        d = np.fmin(np.abs(v["ang_s"] - th), np.abs(v["ang_e"] - th)) / abs(th) if th != 0 else np.full(len(v["ang"]), np.inf)
    return np.where(np.isnan(d), np.inf, d)


def stage_b_reference(v, cfg, ranges):
    """Triangulated, not too sensitive in both views, inside the ranges."""
    with np.errstate(invalid="ignore"):
        keep = v["tri_ok"] & ~((v["sens1"] > cfg["sensitivity_threshold"]) & (v["sens2"] > cfg["sensitivity_threshold"]))
        if ranges is not None:
            lo, hi = np.asarray(ranges[0], float), np.asarray(ranges[1], float)
            for e in (0, 3):
                p = v["line"][:, e:e + 3]
                keep &= ~((p < lo) | (p > hi)).any(axis=1)
    return keep


def is_member(all_tris, scene, target):
    """How often the oracle's (or the device's) candidate store holds the target connection."""
    i, a, j, b = (int(x) for x in target)
    g = int(scene.seg_off[i]) + a
    src = all_tris["src"][all_tris["off"][g]:all_tris["off"][g + 1]]
    return int(np.count_nonzero((src[:, 0] == int(scene.img_ids[j])) & (src[:, 1] == b)))


# ---------------------------------------------------------------------------------------------------------------
# the base scene's connections with the oracle's values (computed once per process)
# ---------------------------------------------------------------------------------------------------------------
_BASE = {}


def base_table(ora, by_endpoints=False):
    """(conns, conn30, values, default-candidate mask, usable-as-target mask) of the base scene."""
    key = bool(by_endpoints)
    if key not in _BASE:
        sc = base_scene()
        conns = connections(sc)
        c30 = conn30(sc, conns)
        v = oracle_values(ora, c30, by_endpoints)
        cfg = base_cfg()
        kept = stage_a_reference(v, cfg) & stage_b_reference(v, cfg, sc.ranges)
        # a target's row is unique (a distractor may repeat a row: the candidate would then be stored twice)
        _, inv, cnt = np.unique(conns, axis=0, return_inverse=True, return_counts=True)
        unique = cnt[inv.reshape(-1)] == 1
        _BASE[key] = (conns, c30, v, kept, kept & unique)
    return _BASE[key]


def _spread(idx, values, n=N_TARGETS):
    """n of the indices idx, spread over the sorted range of their values (deterministic)."""
    idx = np.asarray(idx)
    assert len(idx) >= n, "the base scene has too few connections for this gate"
    order = idx[np.argsort(values[idx], kind="stable")]
    return [int(order[int(round(q * (len(order) - 1)))]) for q in np.linspace(0.15, 0.85, n)]


def _case(name, target_row, keep, ranges=None, **over):
    sc = base_scene()
    if ranges is not None:
        sc = dataclasses.replace(sc, ranges=ranges)
    t = tuple(int(x) for x in target_row)
    return Case(name=name, scene=sc, cfg=base_cfg(**over), images=(int(sc.img_ids[t[0]]),), target=t, keep=keep)


def _three(v):
    return (("pred", float(np.nextafter(v, -np.inf))), ("at", float(v)), ("succ", float(np.nextafter(v, np.inf))))


def family_u(ora, gate, by_endpoints=False):
    """Family U, one ulp: gates with no transcendental.  For N_TARGETS default candidates of the base scene the threshold
    is the target's own value v, the double below and the double above.  The oracle
      * IoU (skips `IoU < th`): keeps the target at pred(v) and at v, drops it at succ(v);
      * len1 / len2 (skips `length <= min_length_2d`): keeps it at pred(v), drops it at v and at succ(v);
      * a lo bound (rejects `x < lo`): keeps it at pred(v) and at v, drops it at succ(v);
      * a hi bound (rejects `x > hi`): drops it at pred(v), keeps it at v and at succ(v).
    Only the target's image is triangulated.  -> list of Case."""
    conns, _, v, _, ok = base_table(ora, by_endpoints)
    over = dict(use_endpoints_triangulation=True) if by_endpoints else {}
    sc = base_scene()
    out = []
    if gate == "iou":
        idx = np.nonzero(ok & (v["iou"] > 0.15) & (v["iou"] < 0.9))[0]
        for t in _spread(idx, v["iou"]):
            for tag, th in _three(v["iou"][t]):
                out.append(_case(f"iou-{t}-{tag}", conns[t], tag != "succ", IoU_threshold=th, **over))
    elif gate in ("len1", "len2"):
        mine, other = (v["len1"], v["len2"]) if gate == "len1" else (v["len2"], v["len1"])
        idx = np.nonzero(ok & (other > 1.01 * mine))[0]  # the other side's length stays clear of the threshold
        for t in _spread(idx, mine):
            for tag, th in _three(mine[t]):
                out.append(_case(f"{gate}-{t}-{tag}", conns[t], tag == "pred", min_length_2d=th, **over))
    elif gate in RANGE_GATES:
        bound, axis, end = gate.split("_")
        k = "xyz".index(axis)
        mine = v["line"][:, k] if end == "start" else v["line"][:, 3 + k]
        other = v["line"][:, 3 + k] if end == "start" else v["line"][:, k]
        # the other endpoint lies well inside the moved bound: this endpoint alone decides
        idx = np.nonzero(ok & ((other > mine + 1e-3) if bound == "lo" else (other < mine - 1e-3)))[0]
        for t in _spread(idx, mine):
            for tag, th in _three(mine[t]):
                lo, hi = np.array(sc.ranges[0], float), np.array(sc.ranges[1], float)
                (lo if bound == "lo" else hi)[k] = th
                keep = tag != "succ" if bound == "lo" else tag != "pred"
                out.append(_case(f"{gate}-{t}-{tag}", conns[t], keep, ranges=(lo, hi), **over))
    else:
        raise ValueError(gate)
    return out


def family_b(ora, gate, by_endpoints=False):
    """Family B, bands: gates that pass through acos.  The threshold is v (1 +- delta) for delta in DELTAS, v the
    target's own value -- the smaller of its two endpoint angles, or the smaller of its two views' sensitivities.  The
    oracle
      * angle (skips `angle < th`): keeps the target at v (1 - delta), drops it at v (1 + delta);
      * sens (drops `sensitivity > th` in both views): drops it at v (1 - delta), keeps it at v (1 + delta).
    The IoU has no acos in it, but its fast decision has a band all the same, so it gets the same thresholds ("iou": kept
    at v (1 - delta), dropped at v (1 + delta)).  gate3 tests delta_iou = num - th den against a margin of at least 1e-7,
    with IoU = num / den and num <= 1: at th = v (1 +- delta) that is |delta_iou| = num delta <= delta, so every
    delta <= BAND_INSIDE lies inside the margin whatever the geometry.
    The targets' values lie below 60 degrees, where a relative delta of the angle is between 0.6 delta and delta in the
    sine the device compares: BAND_INSIDE deltas are inside the 1e-7 band, the others outside.
    Only the target's image is triangulated.  -> list of Case."""
    conns, _, v, _, ok = base_table(ora, by_endpoints)
    over = dict(use_endpoints_triangulation=True) if by_endpoints else {}
    out = []
    if gate == "angle":
        # well inside (1e-3, 89), where make_gen builds the band; IoU well clear of its threshold
        idx = np.nonzero(ok & (v["ang"] > 1.5) & (v["ang"] < 60.0) & (v["iou"] > 0.3))[0]
        key, val = "line_tri_angle_threshold", v["ang"]
    elif gate == "sens":
        idx = np.nonzero(ok & (v["sens"] > 2.0) & (v["sens"] < 60.0))[0]
        key, val = "sensitivity_threshold", v["sens"]
    elif gate == "iou":
        idx = np.nonzero(ok & (v["iou"] > 0.15) & (v["iou"] < 0.9))[0]
        key, val = "IoU_threshold", v["iou"]
    else:
        raise ValueError(gate)
    for t in _spread(idx, val):
        for d in DELTAS:
            for sign in (-1, +1):
                th = float(val[t] * (1.0 + sign * d))
                keep = (sign > 0) if gate == "sens" else (sign < 0)
                out.append(_case(f"{gate}-{t}-{'+' if sign > 0 else '-'}{d:g}", conns[t], keep, **{key: th}, **over))
                out[-1].delta = d
    return out


R_THRESHOLDS = (-1.0, 0.0, 1e-3, float(np.nextafter(1e-3, 1.0)), float(np.nextafter(89.0, 0.0)), 89.0, 90.0, 120.0)
R_SWITCHES = ([("line_tri_angle_threshold", t) for t in R_THRESHOLDS] + [("sensitivity_threshold", t) for t in R_THRESHOLDS] +
              [("min_length_2d", t) for t in (-1.0, 0.0, 5e-324)] + [("IoU_threshold", t) for t in (-1.0, 0.0, 1.0, 2.0)])
R_IMAGES = (1, 2)  # the two images of the base scene that have two neighbours


def family_r(key=None):
    """Family R, regimes: the switches of the band construction (make_gen).  One gate at a time takes a value at which
    the construction changes form -- thresholds outside (1e-3, 89) have no band (the exact expression always decides),
    min_length_2d <= 0 and a denormal one, IoU thresholds outside [0, 1).  The oracle: an angle threshold of 90 or 120
    and an IoU threshold of 2 leave no candidate (no angle reaches 90, the IoU never exceeds 1); an angle or sensitivity
    threshold <= 0, a min_length_2d <= 0 or denormal and an IoU threshold <= 0 reject nothing by that gate; a
    sensitivity threshold >= 90 rejects nothing either.  No target: the whole candidate set is compared.  -> list of Case."""
    sc = base_scene()
    images = tuple(int(sc.img_ids[k]) for k in R_IMAGES)
    return [Case(name=f"{k}={t!r}", scene=sc, cfg=base_cfg(**{k: t}), images=images)
            for k, t in R_SWITCHES if key is None or k == key]


# ---------------------------------------------------------------------------------------------------------------
# family C: one hand-built scene per offset from the degenerate positions
# ---------------------------------------------------------------------------------------------------------------
# what the oracle keeps of each family of family_c: "all", "none", or a function of the offset
C_OUTCOME = dict(plain="all", epipole="none", parallel="none", on_epiline="none", same_pose="none", zero_l1="none",
                 zero_l2="none", far_outside="none", focal_small=lambda o: "all" if o <= 1e-6 else "none", focal_large="all",
                 behind_one="none", behind_both="none", depth_eps=lambda o: "none" if o <= 1e-12 else "some",
                 in_plane="none")
C_FAMILIES = ("plain", "epipole", "parallel", "on_epiline", "same_pose", "zero_l1", "zero_l2", "far_outside", "focal_small",
              "focal_large", "behind_one", "behind_both", "depth_eps", "in_plane")


def _rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def _proj(K4, R, t, X):
    """Homogeneous pinhole projection without any guard: a point behind the camera lands mirrored."""
    x = R @ np.asarray(X, float) + t
    return np.array([K4[0] * x[0] / x[2] + K4[2], K4[1] * x[1] / x[2] + K4[3]])


def family_c(offset):
    """Family C, conditioning: one hand-built scene of six views and 14 segment families, every family placed
    `offset` (px in an image, m in space) from its degenerate position.  Views: 0 at the origin; 1 on view 0's optical
    axis, two metres ahead (the epipoles are the principal points); 2 a generic neighbour; 3 with view 0's pose and its
    centre `offset` metres aside (F = 0 at offset 0); 4 and 5 generic poses with focal lengths 1e-3 and 1e6.  Six views
    and not four: a focal length belongs to a view, so giving one of views 0 - 3 the focal length 1e-3 or 1e6 would
    shrink every segment of that view to 1e-4 px or blow it up to 1e9 px and change the conditioning of every other
    family that uses the view -- each degenerate position is to be the only thing wrong with its rows.
    Each family is written as match rows view -> neighbour (Case.families); what the oracle makes of them (C_OUTCOME,
    asserted by tests/test_gate_cases_host.py at every offset):
      plain         projections of space segments in front of views 0 and 2, both directions: all kept, IoU 1
      epipole       l1's start on view 0's epipole of view 1 (F x~ = 0 up to the rounding of K^-1, so the IoU is an
                    arbitrary finite number, on either side of its threshold): none kept -- the ray through the epipole
                    meets l2's plane behind view 1, or the angle is below its threshold
      parallel      the epipolar line of l1's start parallel to l2 (D -> kEps |a|): the intersection runs off by 1e4 and
                    more segment lengths, |IoU| < 1e-4: none kept
      on_epiline    l2 on the epipolar line of l1's start: the start's ray lies in l2's plane, angle 0 .. 1e-7: none kept
      same_pose     views 0 and 3 coincide (F = 0: normalising the zero epipolar line leaves it zero, the IoU is a finite
                    number; F = O(offset): IoU 1): l1's rays lie in l2's plane, angle <= 0.007: none kept
      zero_l1/l2    a segment of length `offset`: at 0 the length gate `length <= 0` skips it (zero_l2: NaN normal, NaN
                    IoU); longer ones fail the IoU (a point's epipolar overlap with a segment is 0): none kept
      far_outside   segments 1e7 px outside the image: finite arithmetic, IoU -1: none kept
      focal_small   a view with f = 1e-3 (segments of 1e-4 px): all kept while the offset is below the segments' length,
                    none at 1e-3
      focal_large   a view with f = 1e6: all kept
      behind_one / behind_both    the triangulated line behind view 1 / behind both views: stage A passes (IoU 1), the
                    cheirality test of the triangulation rejects: none kept
      depth_eps     l1's start ray meets l2's plane at depth kEps + offset of view 1 (l2 runs to 1e14 px): none kept at
                    offsets 0 and 1e-12 (IoU ~ 1e-3 or 1e-16), some or all from 1e-9 on
      in_plane      l1 inside the back-projected plane of l2 (both rays in the plane, zero determinant): angle 0: none kept
    The scene's ranges are the box [-20, 20]^3.  -> Case (all images triangulated, no target)."""
    o = float(offset)
    f = syn.F_HYPERSIM
    K = np.array([f, f, 400.0, 300.0])
    I3 = np.eye(3)
    views = [  # (K4, R world->cam, centre)
        (K, I3, np.zeros(3)),
        (K, I3, np.array([0.0, 0.0, 2.0])),
        (K, _rot_y(-8.0), np.array([1.0, 0.2, -0.1])),
        (K, I3, np.array([o, 0.0, 0.0])),
        (np.array([1e-3, 1e-3, 400.0, 300.0]), _rot_y(-5.0), np.array([0.8, -0.1, 0.0])),
        (np.array([1e6, 1e6, 400.0, 300.0]), _rot_y(-5.0), np.array([0.8, 0.1, 0.0])),
    ]
    cams = [(k4, R, -R @ c) for k4, R, c in views]
    P = lambda n, X: _proj(*cams[n], X)
    # space segments in front of every view (z in [4, 7])
    rng = np.random.default_rng(12345)
    gts = [(np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1, 1), rng.uniform(4, 7)]),) for _ in range(6)]
    gts = [(a[0], a[0] + np.array([rng.uniform(-1, 1), rng.uniform(-0.8, 0.8), rng.uniform(-0.5, 0.5)])) for a in gts]
    segs = [[] for _ in views]
    rows = {}  # (view, neighbour) -> list of (line, neighbour line)

    def add(n, seg):
        segs[n].append(np.asarray(seg, float).reshape(4))
        return len(segs[n]) - 1

    def row(n, a, m, b):
        rows.setdefault((n, m), []).append((a, b))
        return (n, a, m, b)

    def both(n, m, Xs, Xe, Xs2=None, Xe2=None):
        a = add(n, np.r_[P(n, Xs), P(n, Xe)])
        b = add(m, np.r_[P(m, Xs if Xs2 is None else Xs2), P(m, Xe if Xe2 is None else Xe2)])
        return row(n, a, m, b)

    fam = {}
    # plain: ordinary correspondences 0 -> 2 and 2 -> 0, offset-independent
    fam["plain"] = [both(0, 2, s, e) for s, e in gts] + [both(2, 0, s, e) for s, e in gts[:3]]
    # epipole: l1 in view 0 starts `o` px from the principal point = epipole of view 1; l2 an ordinary segment of view 1
    for s, e in gts[:3]:
        a = add(0, np.r_[400.0 + o, 300.0, P(0, e)])
        b = add(1, np.r_[P(1, s), P(1, e)])
        fam.setdefault("epipole", []).append(row(0, a, 1, b))
    # parallel / on_epiline: 0 -> 2; the epipolar line of l1's start in view 2 is the image of the ray through it
    for s, e in gts[:3]:
        x0, x1 = P(2, s), P(2, 3.0 * s)  # two points of that epipolar line (the images of two points of the ray)
        d = (x1 - x0) / np.linalg.norm(x1 - x0)
        nrm = np.array([-d[1], d[0]])
        a = add(0, np.r_[P(0, s), P(0, e)])
        b = add(2, np.r_[x0 + 50.0 * nrm, x0 + 50.0 * nrm + 80.0 * d + o * nrm])  # parallel to it, 50 px away
        fam.setdefault("parallel", []).append(row(0, a, 2, b))
        b = add(2, np.r_[x0 - 30.0 * d, x0 + 60.0 * d + o * nrm])  # on it
        fam.setdefault("on_epiline", []).append(row(0, a, 2, b))
    # same pose: 0 -> 3 and 3 -> 0
    fam["same_pose"] = [both(0, 3, s, e) for s, e in gts[:3]] + [both(3, 0, s, e) for s, e in gts[3:5]]
    # zero length: an endpoint `o` px from the other
    for s, e in gts[:3]:
        a = add(0, np.r_[P(0, s), P(0, s) + np.array([o, 0.0])])
        b = add(2, np.r_[P(2, s), P(2, e)])
        fam.setdefault("zero_l1", []).append(row(0, a, 2, b))
        a = add(0, np.r_[P(0, s), P(0, e)])
        b = add(2, np.r_[P(2, s), P(2, s) + np.array([0.0, o])])
        fam.setdefault("zero_l2", []).append(row(0, a, 2, b))
    # 1e7 px outside the image
    for s, e in gts[:3]:
        a = add(0, np.r_[1e7 + o, 1e7, 1e7 + 50.0, 1e7 + 30.0])
        b = add(2, np.r_[P(2, s), P(2, e)])
        fam.setdefault("far_outside", []).append(row(0, a, 2, b))
        a = add(0, np.r_[P(0, s), P(0, e)])
        b = add(2, np.r_[-1e7, 1e7 + o, -1e7 + 40.0, 1e7 - 25.0])
        fam["far_outside"].append(row(0, a, 2, b))
    # focal lengths 1e-3 and 1e6 (endpoints `o` px off their projections)
    for name, m in (("focal_small", 4), ("focal_large", 5)):
        fam[name] = []
        for s, e in gts[:3]:
            r = both(0, m, s, e)
            segs[m][r[3]][0] += o
            fam[name].append(r)
            r = both(m, 0, s, e)
            segs[m][r[1]][1] += o
            fam[name].append(r)
    # behind view 1 (space segment between view 0 and view 1, one metre ahead of view 0) and behind both (0 -> 2 with a
    # space segment behind both cameras)
    for s, e in gts[:3]:
        s1, e1 = s / s[2] * (1.0 + o), e / e[2] * 1.2
        fam.setdefault("behind_one", []).append(both(0, 1, s1, e1))
        fam.setdefault("behind_both", []).append(both(0, 2, -s * (1.0 + o), -e))
    # depth in view 1 = kEps + o: the start lies on view 1's principal plane z = 2
    for s, e in gts[:3]:
        s1 = np.array([s[0] / s[2], s[1] / s[2], 1.0]) * (2.0 + 1e-12 + o)
        fam.setdefault("depth_eps", []).append(both(0, 1, s1, e))
    # l1 inside the back-projected plane of l2: the space segment is coplanar with both centres (0 -> 2), its end `o` m
    # out of that plane in view 0 only
    C2 = views[2][2]
    for s, e in gts[:3]:
        e_in = s + 0.7 * C2 + 0.2 * s  # s + alpha (C2 - C0) + beta (s - C0)
        nrm = np.cross(C2, s)
        nrm /= np.linalg.norm(nrm)
        fam.setdefault("in_plane", []).append(both(0, 2, s, e_in + o * nrm, s, e_in))

    # Number the segments of a view block by block: the lines of block (view, neighbour) are contiguous and ascend with
    # the rows (steps of 0 or +1), the segments that only serve as l2 follow -- the regular blocks the line-slot form of
    # stage A takes (an irregular block would send the whole upload to the row-slot form).
    n_views = len(views)
    new_id = []
    for n in range(n_views):
        order = []
        for (v, m) in sorted(rows):
            for a, _ in (rows[(v, m)] if v == n else ()):
                if a not in order:
                    order.append(a)
        order += [a for a in range(len(segs[n])) if a not in order]
        new_id.append({old: k for k, old in enumerate(order)})
        segs[n] = [segs[n][old] for old in order]
    rows = {(n, m): [(new_id[n][a], new_id[m][b]) for a, b in rr] for (n, m), rr in rows.items()}
    fam = {k: [(n, new_id[n][a], m, new_id[m][b]) for n, a, m, b in fv] for k, fv in fam.items()}
    seg_off = np.zeros(n_views + 1, np.int64)
    seg_off[1:] = np.cumsum([len(s) for s in segs])
    scene = syn.Scene(img_ids=np.arange(n_views, dtype=np.int32), kvec=np.array([c[0] for c in cams]),
                      qvec=np.array([syn.rot_to_quat(c[1]) for c in cams]), tvec=np.array([c[2] for c in cams]),
                      seg_off=seg_off, segs=np.concatenate([np.array(s).reshape(-1, 4) for s in segs], 0),
                      gt_ids=-np.ones(int(seg_off[-1]), np.int64), gt_lines=np.zeros((0, 6)),
                      neighbors={n: sorted({m for (a, m) in rows if a == n}) for n in range(n_views)},
                      ranges=(np.full(3, -20.0), np.full(3, 20.0)), seed=0, topk=0)
    matches = {n: {m: np.array(rows[(n, m)], np.int32).reshape(-1, 2) for m in scene.neighbors[n]} for n in range(n_views)}
    assert tuple(fam) == C_FAMILIES
    return Case(name=f"conditioning-{o:g}", scene=scene, cfg=base_cfg(), matches=matches, families=fam)


# ---------------------------------------------------------------------------------------------------------------
# the generation forms the device is run in
# ---------------------------------------------------------------------------------------------------------------
def permuted(case, seed=0):
    """The case with the rows of every block in a random order (the generic grouping of the row pass)."""
    rng = np.random.default_rng(seed)
    ids = [int(i) for i in case.scene.img_ids]
    out = {}
    for i in ids:
        m = case.matches_of(i)
        out[i] = {k: np.ascontiguousarray(np.asarray(r)[rng.permutation(len(r))]) for k, r in m.items()}
    return dataclasses.replace(case, matches=out)
