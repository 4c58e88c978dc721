"""Structured junction scenes for limap_amd.structures, shared by tests/test_bpt_host.py (the grid
prefilter through its host twins, the sparse replay) and tests/test_gpu_bpt_cases.py (the kernels through
lt_bpt_junctions / lt_bpt_associate).  Plain numpy, no GPU, every input from a seeded generator.  A case is
(name, lines (M, 4), keypoints (K, 2), cfg dict); tests/bpt_oracle.py: junctions is the reference for all of them, and
every generator asserts on it the property it exists for, so a case cannot silently stop being the case it claims.

The constants the shapes aim at (limap_amd/csrc/lt_bpt.h): k_bpt_intersect walks row i of the upper triangle in rounds of
256 lanes, j = i + 1 + 256 r + lane; k_bpt_nearest stages 1024 keypoints at a time, k_bpt_assoc 512 lines; the grid of
k_bpt_close_pairs has 2^20 cells per axis of size max(1.25 threshold_merge_junctions, extent / (2^20 - 2))."""
import functools

import numpy as np

import bpt_oracle as bo

BLOCK = 256               # kBptBlock
POINT_TILE = 1024         # kBptPointTile
CELLS = 1 << 20           # 2^kBptCellBits
SLACK = 1.25              # kBptCellSlack
MAX_CANDIDATES = 6000     # per image: what keeps the oracle affordable
MAX_PAIRS = 400000

_REF = {}


def reference(case):
    """bo.junctions of a case, computed once per name and never modified by its users"""
    name, lines, kps, cfg = case
    if name not in _REF:
        o = bo.junctions(lines, kps, cfg)
        assert o["cand_xy"].shape[0] <= MAX_CANDIDATES and o["pairs"].shape[0] <= MAX_PAIRS, name
        _REF[name] = o
    return _REF[name]


def cluster_sizes(o):
    return np.bincount(np.asarray(o["roots"], np.int64)) if len(o["roots"]) else np.zeros(0, np.int64)


def late_round_pairs(o, n_lines):
    """accepted line pairs (i, j) by the round of k_bpt_intersect that finds them: (j - i - 1) // 256"""
    ij = o["cand_lines"][2 * n_lines:]
    return (ij[:, 1] - ij[:, 0] - 1) // BLOCK


def stats(case):
    """what the commit message quotes: candidates, close pairs, largest cluster, pairs found in rounds >= 2 (that is,
    j - i - 1 >= 256)"""
    o = reference(case)
    sz = cluster_sizes(o)
    return dict(candidates=int(o["cand_xy"].shape[0]), pairs=int(o["pairs"].shape[0]),
                largest=int(sz.max()) if sz.size else 0,
                late=int((late_round_pairs(o, np.asarray(case[1]).reshape(-1, 4).shape[0]) >= 1).sum()))


def count_reparents(xy, th, pairs=None):
    """as test_bpt_host.test_chain_fixture_reparents: `parents[j] = i` on a j that already had a parent"""
    parents = [-1] * xy.shape[0]
    moved = 0
    for i, j in (bo.close_pairs(xy, th) if pairs is None else pairs).tolist():
        if bo.find_root(parents, i) != bo.find_root(parents, j):
            moved += parents[j] != -1
            parents[j] = i
    return moved


def extent_branch(lines, th):
    """the grid's cell size comes from the extent, not from the threshold"""
    a = np.asarray(lines, np.float64).reshape(-1, 2)
    ext = float((a.max(0) - a.min(0)).max())
    return ext / (CELLS - 2) > SLACK * th


def _case(name, lines, kps=None, **cfg):
    lines = np.ascontiguousarray(np.asarray(lines, np.float64).reshape(-1, 4))
    kps = np.zeros((0, 2)) if kps is None else np.ascontiguousarray(np.asarray(kps, np.float64).reshape(-1, 2))
    return (name, lines, kps, cfg)


# ---- lattice ----------------------------------------------------------------------------------------------------------
LATTICE_KEPT, LATTICE_DROPPED = (48.0, 40.0), (30.0, 38.0)  # isolated merged junctions, a keypoint 2.0 / 1.0 away


def lattice():
    """axis-aligned segments with integer endpoints of pitch 2.0, all thresholds 2.0: horizontal and vertical
    neighbours are exactly at the threshold and merge, diagonal ones (2 sqrt 2) do not; every endpoint distance is
    exact.  A comb of five rows whose ends are stacked at pitch 2 hangs on a node where three more segments stop 2.0
    short of a fourth one's end: one cluster through `==` alone."""
    L = []
    for k in range(5):                                   # the comb: ends (18, 20 + 2k), starts apart
        L.append([10.0 - 4.0 * k, 20.0 + 2.0 * k, 18.0, 20.0 + 2.0 * k])
    L.append([20.0, 12.0, 20.0, 20.0])                   # ends in the node (20, 20)
    L.append([22.0, 20.0, 30.0, 20.0])                   # starts 2.0 right of it
    L.append([20.0, 32.0, 20.0, 42.0])                   # far above
    for k in range(4):                                   # a collinear chain with gaps of exactly 2.0
        L.append([60.0 + 8.0 * k, 4.0, 66.0 + 8.0 * k, 4.0])
    L.append([40.0, 40.0, 48.0, 40.0])                   # diagonal neighbours (40, 40) and (38, 38): no merge
    L.append([30.0, 38.0, 38.0, 38.0])
    kps = [[50.0, 40.0],                                 # exactly 2.0 from the junction (48, 40): kept
           [30.0, 37.0],                                 # 1.0 from the junction (30, 38): dropped
           [44.0, 42.0], [44.0, np.nextafter(42.0, 43.0)],  # 2.0 / one ulp more from a line's interior
           [80.0, 80.0]]
    c = _case("lattice", L, kps, threshold_keypoints=2.0, threshold_intersection=2.0, threshold_merge_junctions=2.0)
    o = reference(c)
    xy = o["cand_xy"]
    d = np.sqrt(((xy[o["pairs"][:, 0]] - xy[o["pairs"][:, 1]]) ** 2).sum(1))
    assert (d == 2.0).sum() >= 5 and cluster_sizes(o).max() >= 10
    ends = xy[:2 * len(L)].tolist()
    a, b = ends.index([40.0, 40.0]), ends.index([38.0, 38.0])
    assert o["roots"][a] != o["roots"][b]                # 2 sqrt 2 apart
    merged, kept = o["merged_xy"].tolist(), o["xy"].tolist()
    assert list(LATTICE_KEPT) in merged and list(LATTICE_KEPT) in kept
    assert list(LATTICE_DROPPED) in merged and list(LATTICE_DROPPED) not in kept
    return [c]


# ---- star -------------------------------------------------------------------------------------------------------------
def star_lines(n=40, seed=41, hub=(300.0, 200.0)):
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * (np.arange(n) + rng.uniform(-0.2, 0.2, n)) / n
    r = rng.uniform(80, 150, n)[:, None]
    near = np.asarray(hub) + rng.uniform(-0.28, 0.28, (n, 2))  # within 0.4 of the hub
    far = np.asarray(hub) + r * np.stack([np.cos(ang), np.sin(ang)], 1)
    flip = rng.random(n) < 0.5
    return np.where(flip[:, None], np.concatenate([far, near], 1), np.concatenate([near, far], 1))


def star():
    """40 lines with one end within 0.4 of a hub: the 40 ends and all 780 pairwise junctions in one cluster"""
    c = _case("star", star_lines())
    assert cluster_sizes(reference(c)).max() >= 800
    return [c]


# ---- polygons ---------------------------------------------------------------------------------------------------------
def polygon_lines(seed, n_lines=300, frame=(640.0, 480.0), n_chain=8):
    """closed polygons and open polylines; every line end is its vertex + N(0, 0.6); n_chain vertices carry three stub
    lines whose starts are chained at 1.5 spacing (A ~ B, B ~ C, not A ~ C); rows and line directions scrambled"""
    rng = np.random.default_rng(seed)
    W, H = frame
    out, anchors = [], []
    while len(out) < n_lines - 3 * n_chain:
        nv = int(rng.integers(3, 8))
        closed = rng.random() < 0.6
        c = rng.uniform([0.15 * W, 0.15 * H], [0.85 * W, 0.85 * H])
        r = rng.uniform(0.03, 0.1) * W
        ang = np.sort(rng.uniform(0, 2 * np.pi, nv))
        v = c + r * rng.uniform(0.6, 1.0, (nv, 1)) * np.stack([np.cos(ang), np.sin(ang)], 1)
        for k in range(nv if closed else nv - 1):
            out.append(np.concatenate([v[k] + rng.normal(0, 0.6, 2), v[(k + 1) % nv] + rng.normal(0, 0.6, 2)]))
        anchors.append(v[0])
    for k in range(n_chain):
        for s in (1, 2, 3):
            p = anchors[k % len(anchors)] + np.array([1.5 * s, 0.0]) + rng.normal(0, 0.05, 2)
            out.append(np.concatenate([p, p + np.array([10.0 * s, 30.0])]))
    a = np.array(out)[rng.permutation(len(out))]
    flip = rng.random(a.shape[0]) < 0.5
    a[flip] = a[flip][:, [2, 3, 0, 1]]
    return a


def polygons(n_lines=300, name="polygons"):
    c = _case(name, polygon_lines(42, n_lines))
    o = reference(c)
    assert count_reparents(o["cand_xy"], 2.0, o["pairs"]) >= 1
    return [c]


# ---- copies -----------------------------------------------------------------------------------------------------------
COPIES_M = (258, 513, 600, 769)


def copies_lines(M, seed=43):
    """M // 2 random lines, then their copies jittered by less than 1.0 in scrambled order (and one more line where M
    is odd).  The copy of line 0 is the last of the copies, so that row 0 has a hit in its last lane."""
    rng = np.random.default_rng([seed, M])
    h = M // 2
    c = rng.uniform([0, 0], [640.0, 480.0], (h, 2))
    ang = rng.uniform(0, np.pi, h)
    half = 0.5 * rng.uniform(15, 100, h)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    a = np.concatenate([c - half, c + half], 1)
    perm = rng.permutation(np.arange(1, h))
    order = np.concatenate([perm, [0]])
    b = a[order] + rng.uniform(-0.69, 0.69, (h, 4))
    extra = np.array([[5.0, 5.0, 60.0, 9.0]])[:M - 2 * h]
    return np.concatenate([a, b, extra], 0)


def copies(ms=COPIES_M):
    """hits in the second, third and fourth 256-lane round of many rows of k_bpt_intersect.  (With 258 lines only the
    pair (0, 257) can lie in a second round: that one is required there, 50 pairs from 513 lines on.)"""
    out = []
    for M in ms:
        c = _case(f"copies_{M}", copies_lines(M))
        o = reference(c)
        ij = o["cand_lines"][2 * M:]
        gap = ij[:, 1] - ij[:, 0] - 1
        if M >= 2 * BLOCK + 1:
            assert (gap >= BLOCK).sum() >= 50, M
        if M >= 600:
            assert (gap >= 2 * BLOCK).sum() >= 1, M
        if M == 258:
            assert [0, 2 * (M // 2) - 1] in ij.tolist() and gap.max() >= BLOCK
        out.append(c)
    return out


# ---- far --------------------------------------------------------------------------------------------------------------
def far(n_lines=300, suffix=""):
    """large, negative and huge coordinates; the last one takes the cell size from the extent"""
    base = polygon_lines(42, n_lines)
    out = [_case("far_1e6" + suffix, base + np.array([1e6, -3e5, 1e6, -3e5])),
           _case("far_1e9" + suffix, base + 1e9)]
    big = _case("far_extent" + suffix, polygon_lines(44, n_lines, frame=(5.2e6, 3.9e6)))
    assert extent_branch(big[1], 2.0)
    out.append(big)
    for c in out:
        o = reference(c)
        assert cluster_sizes(o).max() >= 3, c[0]  # the jittered vertices still meet
    return out


# ---- tiny_threshold ---------------------------------------------------------------------------------------------------
def tiny_threshold(n_lines=300, name="tiny_threshold"):
    """threshold_merge_junctions = 1e-4 in an ordinary frame (the extent branch); line ends that repeat an earlier
    end exactly, 0.5e-4 beside it and 1.5e-4 beside it"""
    rng = np.random.default_rng(45)
    base = polygon_lines(42, n_lines - 30)
    ends = base.reshape(-1, 2)
    extra = []
    for k, off in enumerate([0.0, 0.5e-4, 1.5e-4] * 10):
        p = ends[(7 * k + 3) % ends.shape[0]] + np.array([off, 0.0])
        extra.append(np.concatenate([p, p + rng.uniform(20, 60, 2)]))
    c = _case(name, np.concatenate([base, extra], 0), threshold_merge_junctions=1e-4)
    assert extent_branch(c[1], 1e-4)
    o = reference(c)
    xy = o["cand_xy"]
    d = np.sqrt(((xy[o["pairs"][:, 0]] - xy[o["pairs"][:, 1]]) ** 2).sum(1))
    assert (d == 0.0).sum() >= 10 and ((d > 0.0) & (d <= 1e-4)).sum() >= 5
    return [c]


# ---- outside_bbox -----------------------------------------------------------------------------------------------------
def outside_bbox():
    """threshold_intersection = 40, threshold_merge_junctions = 0.5: two "Λ" pairs per side of the frame, open towards
    the inside, whose extensions meet beyond the outermost endpoints; the junctions of the two pairs of a side lie
    within 0.5 and merge.  intersect() never returns that apex: where both projection errors are positive the two near
    ends are at most error1 + error2 apart, so an endpoint test has fired and the junction is the midpoint of the near
    ends (no candidate leaves the bounding box, the clamp of a cell coordinate is a guard).  What
    the case pins is therefore candidates *on* the box: cells 0 and the last used cell on both axes."""
    L = []
    for side, (px, py, ux, uy) in enumerate([(320.0, 0.0, 0.0, 1.0), (320.0, 480.0, 0.0, -1.0),
                                             (0.0, 240.0, 1.0, 0.0), (640.0, 240.0, -1.0, 0.0)]):
        for k in range(2):
            ax, ay = px + 0.3 * k * uy, py + 0.3 * k * ux      # the apex, 0.3 along the side for the second pair
            for sgn in (-1.0, 1.0):
                dx, dy = ux + sgn * 0.75 * uy, uy + sgn * 0.75 * ux   # 15 and 90 along the inward normal
                L.append([ax + 15 * dx, ay + 15 * dy, ax + 90 * dx, ay + 90 * dy])
    c = _case("outside_bbox", L, threshold_intersection=40.0, threshold_merge_junctions=0.5)
    o = reference(c)
    a = c[1].reshape(-1, 2)
    lo, hi = a.min(0), a.max(0)
    xy, M = o["cand_xy"], len(L)
    assert (xy.min(0) == lo).all() and (xy.max(0) == hi).all()        # on the box, none beyond
    inter = {tuple(l): k + 2 * M for k, l in enumerate(o["cand_lines"][2 * M:].tolist())}
    for side in range(4):                                             # the two junctions of a side merge
        assert o["roots"][inter[(4 * side, 4 * side + 1)]] == o["roots"][inter[(4 * side + 2, 4 * side + 3)]], side
    return [c]


# ---- thresholds -------------------------------------------------------------------------------------------------------
def thresholds():
    """a 20-line scene at threshold_merge_junctions 0, -1, +inf, 500 and at threshold_intersection +inf, each with and
    without keypoints.  The reference leaves none of them undefined: `dist > th` and `dist < th` are ordinary IEEE
    comparisons (0: only coincident candidates merge; negative: none; +inf and 500: all merge, and with keypoints
    the one junction is dropped)."""
    rng = np.random.default_rng(46)
    lines = rng.uniform(0, 100, (20, 4))
    lines[7, :2] = lines[3, 2:]          # coincident ends, for the threshold 0
    lines[11, 2:] = lines[3, 2:]
    kps = rng.uniform(0, 100, (30, 2))
    out = []
    for tag, cfg in (("m0", dict(threshold_merge_junctions=0.0)), ("mneg", dict(threshold_merge_junctions=-1.0)),
                     ("minf", dict(threshold_merge_junctions=float("inf"))),
                     ("m500", dict(threshold_merge_junctions=500.0)),
                     ("iinf", dict(threshold_intersection=float("inf")))):
        for with_kps in (False, True):
            out.append(_case(f"thresholds_{tag}_{'kps' if with_kps else 'nokps'}", lines, kps if with_kps else None,
                             **cfg))
    by = {c[0]: reference(c) for c in out}
    assert 1 < cluster_sizes(by["thresholds_m0_nokps"]).max() < 10
    assert cluster_sizes(by["thresholds_mneg_nokps"]).max() == 1
    for tag in ("minf", "m500"):
        assert by[f"thresholds_{tag}_nokps"]["xy"].shape[0] == 1 and by[f"thresholds_{tag}_kps"]["xy"].shape[0] == 0
    assert by["thresholds_iinf_nokps"]["cand_xy"].shape[0] == 40 + 190
    return out


# ---- nearest ----------------------------------------------------------------------------------------------------------
NEAREST_K = (1023, 1024, 1025, 2049)


def nearest(ks=NEAREST_K):
    """K keypoints, all at least 3.0 from every merged junction except the last two (and the one at index 1024 where
    there is one), which sit 0.3 from three different junctions: the keypoint that decides is the last of a tile of
    k_bpt_nearest, the first of the next, or the last of all"""
    lines = polygon_lines(47, 80, n_chain=3)
    merged = bo.junctions(lines, np.zeros((0, 2)))["merged_xy"]
    gap = np.sqrt(((merged[:, None, :] - merged[None, :, :]) ** 2).sum(2)) + 1e9 * np.eye(merged.shape[0])
    lonely = np.flatnonzero(gap.min(1) > 3.0)  # a keypoint 0.3 beside one of these is near no other junction
    out = []
    for K in ks:
        rng = np.random.default_rng([48, K])
        p = np.zeros((0, 2))
        while p.shape[0] < K:
            q = rng.uniform([0, 0], [640.0, 480.0], (2 * K, 2))
            d = np.sqrt(((q[:, None, :] - merged[None, :, :]) ** 2).sum(2)).min(1)
            p = np.concatenate([p, q[d >= 3.0]], 0)
        p = p[:K].copy()
        special = [K - 2, K - 1] + ([POINT_TILE] if K > POINT_TILE + 1 else [])
        special = sorted(set(special))
        targets = rng.choice(lonely, len(special), replace=False)
        for k, t in zip(special, targets):
            p[k] = merged[t] + np.array([0.3, 0.0])
        c = _case(f"nearest_{K}", lines, p)
        o = reference(c)
        assert o["xy"].shape[0] == merged.shape[0] - len(special), K  # each of them drops a junction of its own
        for k in special:
            without = bo.nearest_dists(np.delete(p, k, 0), merged)
            assert (without < 2.0).sum() == len(special) - 1, (K, k)
        out.append(c)
    return out


# ---- many_images ------------------------------------------------------------------------------------------------------
def many_images(n=3000, seed=49):
    """n images with 0 to 3 lines and 0 to 2 keypoints in a 30 x 30 frame, the first three and the last three empty:
    (lines list, keypoints list)"""
    rng = np.random.default_rng(seed)
    lines, kps = [], []
    for m in range(n):
        nl, nk = int(rng.integers(0, 4)), int(rng.integers(0, 3))
        if m < 3 or m >= n - 3:
            nl = nk = 0
        a = rng.uniform(0, 30, (nl, 4))
        k = rng.uniform(0, 30, (nk, 2))
        if nk and nl:
            k[0] = a[0, :2] + rng.uniform(-1, 1, 2)  # next to a junction
        lines.append(a)
        kps.append(k)
    assert sum(a.shape[0] == 0 for a in lines) > n // 8 and sum(a.shape[0] == 3 for a in lines) > n // 8
    return lines, kps


def sandwich():
    """copies(769) and star between one-line images: list of cases, all at the default thresholds"""
    one = [_case(f"one_line_{k}", [[3.0 * k, 1.0, 40.0 + k, 9.0]], [[3.0 * k, 1.5]]) for k in range(3)]
    (big,), (st,) = copies((769,)), star()
    return [one[0], big, one[1], st, one[2]]


# ---- all of them ------------------------------------------------------------------------------------------------------
FAMILIES = dict(lattice=lattice, star=star, polygons=polygons, copies=copies, far=far, tiny_threshold=tiny_threshold,
                outside_bbox=outside_bbox, thresholds=thresholds, nearest=nearest)


@functools.lru_cache(maxsize=None)
def family(name):
    return tuple(FAMILIES[name]())


def all_cases():
    out = [c for name in FAMILIES for c in family(name)]
    assert len({c[0] for c in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def reduced_cases():
    """instances of at most 700 candidates for the O(J^2) loop: the small families as they are, the large ones shrunk"""
    rng = np.random.default_rng(50)
    out = [c for name in ("lattice", "outside_bbox", "thresholds") for c in family(name)]
    out.append(_case("star_small", star_lines(18)))
    out += polygons(90, "polygons_small")
    out.append(_case("copies_small", copies_lines(140)))
    out += far(90, "_small")
    out += tiny_threshold(110, "tiny_threshold_small")
    sub = rng.permutation(300)[:60]
    out.append(_case("polygons_rows", polygon_lines(42, 300)[np.sort(sub)]))
    for c in out:
        assert reference(c)["cand_xy"].shape[0] <= 700, c[0]
    return tuple(out)
