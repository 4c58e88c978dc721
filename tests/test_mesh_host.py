"""MeshEvaluator without a GPU: the distance restatement (tests/mesh_oracle.py) on known answers in each of the seven
regions and for degenerate faces, limap_amd.io.read_mesh on every face form and error, and the evaluator's input
checks, which all run before any launch."""
import os

import numpy as np
import pytest

import mesh_oracle as mo
from limap_amd import io
from limap_amd.evaluation import MeshEvaluator

A, B, C = np.array([0.0, 0.0, 0.0]), np.array([2.0, 0.0, 0.0]), np.array([0.0, 2.0, 0.0])


@pytest.mark.parametrize("p, reg, d2", [
    ((-1.0, -1.0, 0.0), 1, 2.0),     # behind a
    ((3.0, -1.0, 0.0), 2, 2.0),      # beyond b
    ((1.0, -1.0, 1.0), 3, 2.0),      # below edge ab: q = (1, 0, 0)
    ((-1.0, 3.0, 0.0), 4, 2.0),      # beyond c
    ((-2.0, 1.0, 1.0), 5, 5.0),      # left of edge ac: q = (0, 1, 0)
    ((2.0, 2.0, 0.0), 6, 2.0),       # beyond edge bc: q = (1, 1, 0)
    ((0.5, 0.5, 3.0), 7, 9.0),       # above the interior
    ((0.5, 0.5, 0.0), 7, 0.0),       # on the face
    ((0.0, 0.0, 0.0), 1, 0.0),       # on a vertex
])
def test_regions_known_answers(p, reg, d2):
    p = np.array(p)
    assert mo.region(A, B, C, p) == reg
    got = mo.tri_dist2(A[None], B[None], C[None], p[None])[0]
    assert got == d2
    assert mo.nearest_dists(np.stack([A, B, C]), [[0, 1, 2]], p[None])[0] == np.sqrt(d2)


def test_degenerate_faces():
    # collinear: the interior denominator is 0, the project rule takes the nearest clamped edge point
    a, b, c = np.array([0.0, 0, 0]), np.array([1.0, 0, 0]), np.array([3.0, 0, 0])
    p = np.array([2.0, 1.0, 0.0])
    assert mo.region(a, b, c, p) in (0, 3, 5, 6)
    assert mo.tri_dist2(a[None], b[None], c[None], p[None])[0] == 1.0
    # all three vertices equal: region 1, q = a
    a = np.array([1.0, 2.0, 3.0])
    p = np.array([1.0, 2.0, 5.0])
    assert mo.region(a, a, a, p) == 1
    assert mo.tri_dist2(a[None], a[None], a[None], p[None])[0] == 4.0
    # a == b != c on the side of c: 0/0 in region 3, a NaN that never wins the minimum
    a, c = np.array([0.0, 0, 0]), np.array([0.0, 2.0, 0])
    p = np.array([0.0, 1.0, 1.0])
    assert np.isnan(mo.tri_dist2(a[None], a[None], c[None], p[None])[0])
    V = np.array([[0.0, 0, 0], [0, 2, 0], [5, 5, 5], [6, 5, 5], [5, 6, 5]])
    assert mo.nearest_dists(V, [[0, 0, 1], [2, 3, 4]], p[None])[0] == np.sqrt(mo.tri_dist2(
        V[2][None], V[3][None], V[4][None], p[None])[0])


def test_oracle_min_matches_ordered_fold():
    rng = np.random.default_rng(3)
    V = rng.normal(size=(40, 3))
    F = rng.integers(0, 40, (60, 3))
    Q = rng.normal(size=(50, 3)) * 2
    got = mo.nearest_dists(V, F, Q, block=7, fblock=9)
    for k in range(Q.shape[0]):
        best = np.inf
        for f in F:
            d = mo.region(V[f[0]], V[f[1]], V[f[2]], Q[k])  # (exercises the scalar form on random faces)
            d2 = mo.tri_dist2(V[f[0]][None], V[f[1]][None], V[f[2]][None], Q[k][None])[0]
            best = d2 if d2 < best else best
            assert 0 <= d <= 7
        assert got[k] == np.sqrt(best)


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def test_read_obj_face_forms(tmp_path):
    fn = _write(tmp_path / "m.obj", """# a comment
o thing
v 0 0 0
v 1 0 0 1.0
v 1 1 0
v 0 1 0
vt 0 0
vn 0 0 1
g group
usemtl m
f 1 2 3
f 1/1 3/1 4/1
f 1//1 2//1 3//1
f 1/1/1 2/1/1 4/1/1
f -4 -3 -2
l 1 2
f 1 2 3 4
v 0 0 1
f 1 2 3 4 -1
""")
    V, F = io.read_mesh(fn)
    assert V.dtype == np.float64 and F.dtype == np.int64
    assert V.shape == (5, 3) and V[1].tolist() == [1.0, 0.0, 0.0]
    assert F.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 1, 3], [0, 1, 2],
                          [0, 1, 2], [0, 2, 3],
                          [0, 1, 2], [0, 2, 3], [0, 3, 4]]


def test_read_off(tmp_path):
    fn = _write(tmp_path / "m.off", """OFF
# counts
4 2 0
0 0 0
1 0 0   # a vertex
1 1 0
0 1 0
4 0 1 2 3
3 0 2 3 255 0 0
""")
    V, F = io.read_mesh(fn)
    assert V.shape == (4, 3)
    assert F.tolist() == [[0, 1, 2], [0, 2, 3], [0, 2, 3]]
    fn = _write(tmp_path / "n.off", "OFF 3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n")
    assert io.read_mesh(fn)[1].tolist() == [[0, 1, 2]]


def test_read_mesh_errors(tmp_path):
    with pytest.raises(NotImplementedError):
        io.read_mesh(_write(tmp_path / "m.ply", "ply\n"))
    lines = np.array([[[0.0, 0, 0], [1, 0, 0]], [[0, 1, 0], [1, 1, 0]]])
    io.save_obj(str(tmp_path / "lines.obj"), lines)
    with pytest.raises(ValueError, match="no faces"):
        io.read_mesh(str(tmp_path / "lines.obj"))
    with pytest.raises(ValueError, match="out of range"):
        io.read_mesh(_write(tmp_path / "r.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n"))
    with pytest.raises(ValueError, match="out of range"):
        io.read_mesh(_write(tmp_path / "n.obj", "v 0 0 0\nv 1 0 0\nf -3 1 2\n"))
    with pytest.raises(ValueError, match="index 0"):
        io.read_mesh(_write(tmp_path / "z.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n"))
    with pytest.raises(ValueError, match="non-finite"):
        io.read_mesh(_write(tmp_path / "f.obj", "v 0 0 nan\nv 1 0 0\nv 0 1 0\nf 1 2 3\n"))
    with pytest.raises(ValueError, match="out of range"):
        io.read_mesh(_write(tmp_path / "r.off", "OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 3\n"))
    with pytest.raises(ValueError, match="no faces"):
        io.read_mesh(_write(tmp_path / "e.off", "OFF\n3 0 0\n0 0 0\n1 0 0\n0 1 0\n"))
    with pytest.raises(ValueError, match="corners"):
        io.read_mesh(_write(tmp_path / "c.obj", "v 0 0 0\nv 1 0 0\nf 1 2\n"))


def test_mpau_scaling_before_anything(tmp_path):
    fn = _write(tmp_path / "m.obj", "v 0.1 0.2 0.3\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    E = MeshEvaluator(fn, 0.7)  # no launch: the index is built on first use
    assert E.mpau == 0.7 and E.n_faces == 1
    assert np.array_equal(mo.scale_vertices(E.V, E.mpau)[0], np.array([0.1 * 0.7, 0.2 * 0.7, 0.3 * 0.7]))


@pytest.mark.parametrize("V, F, mpau, msg", [
    (np.zeros((3, 3)), np.zeros((0, 3), np.int64), 1.0, "without faces"),
    (np.zeros((3, 3)), [[0, 1, 3]], 1.0, "out of range"),
    (np.zeros((3, 3)), [[0, -1, 2]], 1.0, "out of range"),
    (np.array([[0, 0, 0], [1, 0, 0], [0, np.inf, 0]]), [[0, 1, 2]], 1.0, "non-finite"),
    (np.array([[0, 0, 0], [1e300, 0, 0], [0, 1, 0]]), [[0, 1, 2]], 1e10, "non-finite"),
    (np.zeros((3, 3)), [[0, 1, 2]], float("nan"), "mpau"),
    (np.zeros((3, 3)), [[0.0, 1.0, 2.0]], 1.0, "integers"),
])
def test_evaluator_rejects_bad_input(V, F, mpau, msg):
    with pytest.raises(ValueError, match=msg):
        MeshEvaluator.from_arrays(V, F, mpau)


def test_evaluator_file_errors(tmp_path):
    with pytest.raises(NotImplementedError):
        MeshEvaluator(_write(tmp_path / "m.stl", "solid\n"), 1.0)
    with pytest.raises(ValueError):
        MeshEvaluator(_write(tmp_path / "m.obj", "v 0 0 0\n"), 1.0)
    assert os.path.exists(tmp_path / "m.obj")
