"""MeshEvaluator on the device, bit for bit against the NumPy restatement (tests/mesh_oracle.py), and the hierarchy walk
bit for bit against the brute-force form (LT_TEST_MESH_BRUTE), on meshes that stress the distance and the pruning:
slivers and degenerate faces, shared edges and vertices, far queries, large offsets, a 10^6-face room."""
import numpy as np
import pytest

import eval_oracle as eo
import mesh_oracle as mo

pytestmark = pytest.mark.gpu

TH = np.array([0.001, 0.005, 0.01, 0.05])


@pytest.fixture(scope="module")
def ev():
    from limap_amd import evaluation
    return evaluation


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def grid_mesh(n, lo=0.0, hi=1.0, z=None, rng=None):
    """an n x n grid of squares, two triangles each, coplanar (z None: flat) or with a height field"""
    t = np.linspace(lo, hi, n + 1)
    X, Y = np.meshgrid(t, t, indexing="ij")
    Z = np.zeros_like(X) if z is None else z(X, Y)
    V = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1)
    i = np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]
    i = i.ravel()
    F = np.concatenate([np.stack([i, i + n + 1, i + 1], 1), np.stack([i + 1, i + n + 1, i + n + 2], 1)], 0)
    return V, F


def room(n_side, rng, bump=0.01):
    """the six walls of a 10 m box, each an n_side x n_side grid with a small height perturbation"""
    Vs, Fs, off = [], [], 0
    for axis in range(3):
        for side in (0.0, 10.0):
            V, F = grid_mesh(n_side, 0.0, 10.0)
            h = bump * rng.uniform(-1, 1, V.shape[0])
            W = np.empty_like(V)
            others = [k for k in range(3) if k != axis]
            W[:, others[0]], W[:, others[1]], W[:, axis] = V[:, 0], V[:, 1], side + h
            Vs.append(W)
            Fs.append(F + off)
            off += W.shape[0]
    return np.concatenate(Vs), np.concatenate(Fs)


def meshes():
    rng = np.random.default_rng(5)
    out = {}
    out["single"] = (np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]]))
    V = rng.normal(size=(300, 3))
    out["random"] = (V, rng.integers(0, 300, (2000, 3)))
    # slivers (one corner nudged off a long edge), collinear faces, three equal vertices, duplicated vertices
    a = rng.uniform(-1, 1, (200, 3))
    b = a + rng.normal(size=(200, 3))
    c = 0.5 * (a + b) + rng.normal(size=(200, 3)) * 10.0 ** rng.uniform(-14, -4, (200, 1))
    col = a + 3.0 * (b - a)
    dup = np.concatenate([a, b, c, col, a[:50]], 0)
    n = 200
    F = np.concatenate([np.stack([np.arange(n), n + np.arange(n), 2 * n + np.arange(n)], 1),
                        np.stack([np.arange(n), n + np.arange(n), 3 * n + np.arange(n)], 1),
                        np.stack([np.arange(50)] * 3, 1),
                        np.stack([np.arange(50), 4 * n + np.arange(50), n + np.arange(50)], 1),
                        np.stack([np.arange(50), np.arange(50), 2 * n + np.arange(50)], 1)], 0)
    out["slivers"] = (dup, F)
    out["tiling"] = grid_mesh(12, 0.0, 1.0)
    V, F = room(6, rng)
    out["offset"] = (grid_mesh(20, 0.0, 0.02, z=lambda X, Y: 0.001 * np.sin(300 * X) * np.cos(200 * Y))[0] + 1e5,
                     grid_mesh(20)[1])
    out["room"] = (V, F)
    return out


def queries(name, V, F, rng):
    lo, hi = V.min(0), V.max(0)
    ext = np.maximum(hi - lo, 1e-3)
    q = [rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext, (1500, 3))]
    w = rng.dirichlet([1, 1, 1], 400)
    k = np.arange(400) % len(F)  # near the faces
    q.append((w[:, 0:1] * V[F[k, 0]] + w[:, 1:2] * V[F[k, 1]] + w[:, 2:3] * V[F[k, 2]])
             + rng.normal(size=(400, 3)) * 1e-3 * ext)
    q.append(V[:200])  # exactly on vertices
    if name == "tiling":  # exactly on shared edges: midpoints of the grid edges, and on the face planes
        e = F[:, [0, 1]]
        q.append(0.5 * (V[e[:, 0]] + V[e[:, 1]]))
        q.append(np.stack([rng.uniform(0, 1, 200), rng.uniform(0, 1, 200), np.zeros(200)], 1))
    q.append(rng.normal(size=(100, 3)) * 1e6)  # far
    return np.concatenate(q, 0)


@pytest.fixture(scope="module")
def scenes():
    rng = np.random.default_rng(17)
    return {k: (V, F, queries(k, V, F, rng)) for k, (V, F) in meshes().items()}


@pytest.mark.parametrize("name", ["single", "random", "slivers", "tiling", "offset", "room"])
def test_dist_points_equal_oracle_and_brute_force(ev, scenes, name, monkeypatch):
    V, F, Q = scenes[name]
    E = ev.MeshEvaluator.from_arrays(V, F, 1.0)
    got = E.ComputeDistPoints(Q)
    assert same(got, mo.nearest_dists(V, F, Q)), name
    assert E.ComputeDistPoint(Q[3]) == got[3]
    monkeypatch.setenv("LT_TEST_MESH_BRUTE", "1")
    assert same(E.ComputeDistPoints(Q), got), name


def test_walk_equals_brute_force_on_a_million_faces(ev, monkeypatch):
    rng = np.random.default_rng(23)
    V, F = room(289, rng)  # 6 * 2 * 289^2 = 1 002 252 faces
    assert F.shape[0] > 1_000_000
    E = ev.MeshEvaluator.from_arrays(V, F, 1.0)
    k = rng.integers(0, F.shape[0], 3000)
    w = rng.dirichlet([1, 1, 1], 3000)
    near = (w[:, 0:1] * V[F[k, 0]] + w[:, 1:2] * V[F[k, 1]] + w[:, 2:3] * V[F[k, 2]]) + rng.normal(size=(3000, 3)) * 0.01
    Q = np.concatenate([near, rng.uniform(-2, 12, (2000, 3)), rng.normal(size=(200, 3)) * 1e4], 0)
    walk = E.ComputeDistPoints(Q)
    monkeypatch.setenv("LT_TEST_MESH_BRUTE", "1")
    brute = E.ComputeDistPoints(Q)
    assert same(walk, brute)
    assert (walk[:3000] <= 0.05).mean() > 0.9


@pytest.fixture(scope="module")
def line_scene():
    rng = np.random.default_rng(29)
    V, F = room(5, rng, bump=0.05)
    s = rng.uniform(-0.5, 10.5, (25, 3))
    s[:10, 0] = rng.uniform(-0.01, 0.01, 10)  # lines along a wall: inliers at the thresholds
    d = rng.normal(size=(25, 3))
    d[:10, 0] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    lines = np.concatenate([s, s + d * rng.uniform(0.05, 1.0, (25, 1))], 1)
    return V, F, lines


@pytest.mark.parametrize("chunk", [0, 1, 63, 64, 65])
def test_line_functions_equal_oracle(ev, line_scene, chunk):
    from limap_amd.base import Line3d
    V, F, lines = line_scene
    E = ev.MeshEvaluator.from_arrays(V, F, 1.0, chunk=chunk)
    sub = lines if chunk in (0, 64) else lines[:6]
    l3 = [Line3d(r[:3], r[3:]) for r in sub]
    for n in (1000, 3):
        if chunk in (1, 63, 65) and n == 1000:
            continue
        assert same([E.ComputeDistLine(x, n_samples=n) for x in l3], [mo.dist_line(V, F, r, n) for r in sub])
    for n in (1000, 37):
        if chunk == 1 and n == 1000:
            continue
        assert same(E.ComputeInlierRatios(sub, TH, n_samples=n), mo.inlier_ratios(V, F, sub, TH, n))
        for t in (0.01, 0.05):
            for fn, inl in ((E.ComputeInlierSegs, True), (E.ComputeOutlierSegs, False)):
                got = fn(l3, t, n_samples=n)
                arr = np.array([np.concatenate([x.start, x.end]) for x in got]).reshape(-1, 6)
                assert same(arr, mo.segs(V, F, sub, t, n, inl)), (t, n, inl)
    assert E.ComputeInlierRatio(l3[0], 0.01) == mo.inlier_ratios(V, F, sub[:1], [0.01], 1000)[0, 0]


def test_report_error_to_gt_and_walk_on_lines(ev, line_scene, monkeypatch):
    V, F, lines = line_scene
    E = ev.MeshEvaluator.from_arrays(V, F, 1.0)
    rep = ev.report_error_to_GT(E, lines, TH[:3])
    r = mo.inlier_ratios(V, F, lines, TH[:3], 1000)
    lengths = eo.length(lines)
    assert same(rep["ratios"], r)
    assert same(rep["recall"], np.array([(lengths * r[:, t]).sum() for t in range(3)]))
    assert same(rep["precision"], np.array([100 * (r[:, t] > 0).astype(int).sum() / len(lines) for t in range(3)]))
    monkeypatch.setenv("LT_TEST_MESH_BRUTE", "1")
    assert same(E.ComputeInlierRatios(lines, TH), mo.inlier_ratios(V, F, lines, TH, 1000))


def test_files_round_trip(ev, tmp_path):
    rng = np.random.default_rng(31)
    V, F = grid_mesh(4, 0.0, 1.0, z=lambda X, Y: 0.1 * X * Y)
    V = V + rng.normal(size=V.shape) * 1e-3
    obj, off = tmp_path / "m.obj", tmp_path / "m.off"
    with open(obj, "w") as f:
        f.writelines(f"v {x!r} {y!r} {z!r}\n" for x, y, z in V.tolist())
        f.writelines(f"f {a + 1}/1 {b + 1}/1 {c + 1}/1\n" for a, b, c in F.tolist())
    with open(off, "w") as f:
        f.write(f"OFF\n# a mesh\n{len(V)} {len(F)} 0\n")
        f.writelines(f"{x!r} {y!r} {z!r}\n" for x, y, z in V.tolist())
        f.writelines(f"3 {a} {b} {c}\n" for a, b, c in F.tolist())
    mpau = 0.37
    Q = rng.uniform(-0.2, 0.6, (500, 3))
    want = mo.nearest_dists(mo.scale_vertices(V, mpau), F, Q)
    for fn in (obj, off):
        E = ev.MeshEvaluator(str(fn), mpau)
        assert same(E.ComputeDistPoints(Q), want)


def test_build_timers_and_levels(ev):
    V, F = grid_mesh(40)
    E = ev.MeshEvaluator.from_arrays(V, F)
    E.Build()
    t = E.timers()
    assert t[0] > 0 and t[2] >= 6 and t[3] >= 2
