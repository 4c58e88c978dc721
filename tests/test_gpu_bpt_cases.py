"""The bipartite kernels (lt_kernels_bpt.hip) on the structured scenes of tests/bpt_cases.py against tests/bpt_oracle.py,
zero tolerance: candidate coordinates bit for bit, line pairs, the union-find's parents, junction coordinates bit for
bit, line-id lists -- and the number of close pairs the device found, which is what turns a pair the grid dropped into a
failure even where another pair keeps the cluster together."""
import numpy as np
import pytest

import bpt_cases as bc
import bpt_oracle as bo
from test_bpt_host import bits

pytestmark = pytest.mark.gpu


def csr_lists(off, flat):
    return [flat[off[k]:off[k + 1]].tolist() for k in range(len(off) - 1)]


def assert_image(res, cand, o, tag):
    assert np.array_equal(bits(cand["xy"]), bits(o["cand_xy"])), tag
    assert np.array_equal(cand["lines"], o["cand_lines"].reshape(-1, 2)), tag
    want_parents = [-1 if r == k else r for k, r in enumerate(o["roots"])]  # after the last root look-ups
    assert cand["parents"].tolist() == want_parents, tag
    assert np.array_equal(bits(res[0]), bits(o["xy"])), tag
    assert csr_lists(res[1], res[2]) == o["line_ids"], tag


def run(st, cases):
    """cases that share a configuration, in one call: (results, candidates, sizes)"""
    cfg = st.PL_Bipartite2dConfig(cases[0][3])
    assert all(st.PL_Bipartite2dConfig(c[3]).as_dict() == cfg.as_dict() for c in cases)
    return st._junctions([c[1] for c in cases], [c[2] for c in cases], cfg, candidates=True, sizes=True)


def same(a, b):
    return all(np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64
                              else y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(bc.FAMILIES))
def test_case_families_equal_oracle(gpu_lib, name):
    from limap_amd import structures as st
    cases = bc.family(name)
    single = []
    for c in cases:
        res, cands, sizes = run(st, [c])
        o = bc.reference(c)
        print(c[0], bc.stats(c), "device pairs", int(sizes[3]))
        assert_image(res[0], cands[0], o, c[0])
        assert sizes.tolist() == [o["xy"].shape[0], sum(len(l) for l in o["line_ids"]), o["cand_xy"].shape[0],
                                  o["pairs"].shape[0]], c[0]
        single.append((res[0], cands[0]))
    # all cases of a configuration in one batched call, in both orders: the single-image results
    groups = {}
    for k, c in enumerate(cases):
        groups.setdefault(tuple(sorted(st.PL_Bipartite2dConfig(c[3]).as_dict().items())), []).append(k)
    for idx in groups.values():
        for order in (idx, idx[::-1]):
            res, cands, sizes = run(st, [cases[k] for k in order])
            assert sizes[3] == sum(bc.reference(cases[k])["pairs"].shape[0] for k in order)
            for n, k in enumerate(order):
                assert same(res[n], single[k][0]), (cases[k][0], order)
                assert same([cands[n][f] for f in ("xy", "lines", "parents")],
                            [single[k][1][f] for f in ("xy", "lines", "parents")]), (cases[k][0], order)


def test_large_images_between_one_line_images(gpu_lib):
    """copies(769) and star between one-line images, forwards and backwards"""
    from limap_amd import structures as st
    cases = bc.sandwich()
    for order in (cases, cases[::-1]):
        res, cands, sizes = run(st, order)
        for n, c in enumerate(order):
            assert_image(res[n], cands[n], bc.reference(c), c[0])
        assert sizes[3] == sum(bc.reference(c)["pairs"].shape[0] for c in order)


def test_many_images_equal_oracle(gpu_lib):
    """3000 images of 0 to 3 lines, empty ones first and last: image_of, the image bits of the keys, pair_img_off"""
    from limap_amd import structures as st
    lines, kps = bc.many_images()
    cfg = st.PL_Bipartite2dConfig()
    res, cands, sizes = st._junctions(lines, kps, cfg, candidates=True, sizes=True)
    n_pairs = n_junc = 0
    for m in range(len(lines)):
        o = bo.junctions(lines[m], kps[m])
        assert_image(res[m], cands[m], o, m)
        n_pairs += o["pairs"].shape[0]
        n_junc += o["xy"].shape[0]
    assert sizes[3] == n_pairs and sizes[0] == n_junc and n_pairs > 500  # (the restatement counts 937: the batch is not vacuous)
    out = st.compute_junctions(dict(enumerate(lines)), dict(enumerate(kps)))
    assert sorted(out) == list(range(len(lines)))
    assert all(np.array_equal(bits(out[m]), bits(res[m][0])) for m in range(len(lines)))


def test_class_surface_on_lattice_and_star(gpu_lib):
    from limap_amd import structures as st
    for c in bc.family("lattice") + bc.family("star"):
        o = bc.reference(c)
        ids = np.arange(c[1].shape[0]) * 2 + 5  # sparse line ids
        b = st.PL_Bipartite2d(c[3])
        b.init_lines(c[1], ids)
        b.compute_intersection_with_points(c[2])
        assert b.get_point_ids() == list(range(o["xy"].shape[0]))
        assert [j.line_ids for j in b.get_all_junctions()] == [ids[l].tolist() for l in o["line_ids"]]
        assert np.array_equal(bits(np.array([p.p for p in b.get_all_points()]).reshape(-1, 2)), bits(o["xy"]))


# ---- association --------------------------------------------------------------------------------------------------------
def assert_association(st, lines, pts, th=2.0):
    res = st._associate(lines, pts, st.PL_Bipartite2dConfig(dict(threshold_keypoints=th)))
    n = 0
    for m in range(len(lines)):
        want = bo.associate(lines[m], pts[m], th)
        assert csr_lists(*res[m]) == [w.tolist() for w in want], m
        n += sum(w.size for w in want)
    return n


def test_association_lattice_exact_threshold_batch(gpu_lib):
    """the lattice keypoints (2.0 from an end, 2.0 and one ulp more from an interior) in every one of 40 images"""
    from limap_amd import structures as st
    (c,) = bc.family("lattice")
    want = bo.associate(c[1], c[2], 2.0)
    assert want[0].tolist() == [12] and want[2].tolist() == [12] and want[3].size == 0
    lines = [c[1][m % 3:] for m in range(40)]  # other line indices per image
    assert assert_association(st, lines, [c[2]] * 40) >= 3 * 40


@pytest.mark.parametrize("n_lines", [511, 512, 513])
def test_association_only_line_at_the_tile_edge(gpu_lib, n_lines):
    """the one line within the threshold of a point is the last of the first tile of 512, the first of the second,
    or the last of all; 255, 256 and 257 points"""
    from limap_amd import structures as st
    rng = np.random.default_rng(n_lines)
    lines, pts, hot = [], [], []
    for n_pts in (255, 256, 257):
        c = rng.uniform([0, 0], [640.0, 480.0], (n_lines, 2))
        ang = rng.uniform(0, np.pi, n_lines)
        h = 0.5 * rng.uniform(15, 100, n_lines)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
        a = np.concatenate([c - h, c + h], 1)
        p = rng.uniform([1000.0, 0], [1600.0, 480.0], (n_pts, 2))  # far from every line
        targets = sorted({k for k in (0, 510, 511, 512, n_lines - 1) if k < n_lines})
        for q, k in enumerate(targets):  # first and last points of the block
            a[k] += np.array([3000.0 * (q + 1), 0, 3000.0 * (q + 1), 0])  # a line of its own, away from the rest
            for row in (q, n_pts - 1 - q):
                p[row] = 0.5 * (a[k, :2] + a[k, 2:]) + np.array([-h[k, 1], h[k, 0]]) / np.linalg.norm(h[k]) * 1.5
        lines.append(a)
        pts.append(p)
        hot.append(targets)
    for a, p, targets in zip(lines, pts, hot):
        want = bo.associate(a, p, 2.0)
        assert [w.tolist() for w in want[:len(targets)]] == [[k] for k in targets]
        assert sum(w.size for w in want) == 2 * len(targets)
    assert_association(st, lines, pts)


def test_association_far_translations(gpu_lib):
    from limap_amd import structures as st
    rng = np.random.default_rng(9)
    lines, pts = [], []
    for c in bc.family("far"):
        a = c[1]
        k = rng.integers(0, a.shape[0], 400)
        t = rng.uniform(-0.05, 1.05, (400, 1))
        lines.append(a)
        pts.append(a[k, :2] + t * (a[k, 2:] - a[k, :2]) + rng.normal(0, 1.4, (400, 2)))
    assert assert_association(st, lines, pts) > 400
