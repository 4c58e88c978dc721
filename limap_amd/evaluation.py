"""limap.evaluation on the GPU: a drop-in for ``PointCloudEvaluator``, ``RefLineEvaluator`` and ``MeshEvaluator``
(evaluation/bindings.cc of limap; method and argument names, and defaults, follow the bindings), plus batched forms and
the two helpers of scripts/eval_hypersim.py and scripts/eval_tnt.py.

    from limap_amd import evaluation
    ev = evaluation.PointCloudEvaluator(points)       # (N, 3) array, list of (3,) arrays, or a float32/64 GPU tensor
    ev.Build()
    ratios = ev.ComputeInlierRatios(lines, [0.001, 0.005, 0.01])   # (L, T), one distance pass
    mesh = evaluation.MeshEvaluator("scene.obj", MPAU)    # .obj / .off, vertices scaled by mpau
    report = evaluation.report_error_to_GT(mesh, lines, [0.001, 0.005, 0.01])

Every point-cloud and line distance is the reference's expression bit for bit; the few host-side
reductions (ComputeDistLine's sum, the recall length, the segment endpoints) run in the reference's order.  The mesh
distance is Ericson's closest point on a triangle in the FP64 operation order of DESIGN.md section 15, held bit for bit
to a NumPy restatement in the tests; the reference computes it with libigl, against which no agreement is claimed.
"""
import ctypes as C
import hashlib
import math
import struct

import numpy as np

from . import _capi, _native
from .base import Line3d

__all__ = ["PointCloudEvaluator", "RefLineEvaluator", "MeshEvaluator", "report_error_to_GT", "report_pc_recall_for_GT",
           "lines_array", "line_lengths"]

_MAGIC = b"LIMAP_AMD_PCD\x00\x01\x00"  # 16 bytes: name, format version 1
_context = _capi.per_device_contexts()
_p = _capi.ptr


def lines_array(lines):
    """lines: list of Line3d, list of LineTrack (their .line), or an (L, 2, 3) / (L, 6) array -> contiguous (L, 6)"""
    if isinstance(lines, np.ndarray) or (hasattr(lines, "shape") and not isinstance(lines, (list, tuple))):
        a = np.asarray(lines, np.float64)
        if a.ndim == 3 and a.shape[1:] == (2, 3):
            a = a.reshape(-1, 6)
        if a.ndim != 2 or a.shape[1] != 6:
            raise ValueError(f"lines must be (L, 2, 3) or (L, 6), got shape {a.shape}")
    else:
        rows = []
        for x in lines:
            ln = x.line if hasattr(x, "line") and not hasattr(x, "start") else x
            if hasattr(ln, "start") and hasattr(ln, "end"):
                rows.append(np.concatenate([np.asarray(ln.start, np.float64).reshape(3),
                                            np.asarray(ln.end, np.float64).reshape(3)]))
            else:
                rows.append(np.asarray(ln, np.float64).reshape(6))
        a = np.stack(rows, 0) if rows else np.zeros((0, 6))
    a = np.ascontiguousarray(a, np.float64)
    if not np.isfinite(a).all():
        raise ValueError("lines: non-finite coordinate")
    return a


def line_lengths(a):
    """Line3d::length() of the reference, (start - end).norm() = sqrt((x*x + y*y) + z*z), for an (L, 6) array"""
    w = a[:, 0:3] - a[:, 3:6]
    return np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])


def _thresholds(thresholds):
    th = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, np.float64)).reshape(-1))
    if th.size > 64:
        raise ValueError("at most 64 thresholds per call")
    return th


def _check_n(n_samples, lo=1):
    n = int(n_samples)
    if n < lo:
        raise ValueError(f"n_samples must be >= {lo}, got {n}")
    if n >= 2**31:
        raise ValueError("n_samples must be below 2^31")
    return n


def _points3(p):
    q = np.ascontiguousarray(np.asarray(p, np.float64).reshape(-1, 3))
    if not np.isfinite(q).all():
        raise ValueError("query point: non-finite coordinate")
    return q


class _SampledEvaluator:
    """the methods of evaluation/base_evaluator.cc over a device index: nearest distances of free points and of line
    samples generated on the device (distances and per-threshold counts).  A subclass names its two query entry points
    and the free function of the C ABI, and implements _index(), which returns the handle (built on first use) that it
    keeps in _handle."""

    _handle = None

    def _ctx(self):
        return _context(self.device)

    def _free(self):
        if self._handle is not None and self._handle.value:
            getattr(_capi.load_library(), self._free_fn)(self._handle)
        self._handle = None

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass

    def timers(self):
        return self._ctx().module_timers("lt_eval_get_timers", 4)

    def ComputeDistPoints(self, points, chunk=None):
        """ComputeDistPoint for each row of an (M, 3) array"""
        q = _points3(points)
        out = np.zeros(max(q.shape[0], 1))
        ctx = self._ctx()
        index = self._index()
        ctx.chk(getattr(ctx.L, self._nearest_fn)(ctx.h, index, _p(q), q.shape[0], self._chunk(chunk), _p(out)))
        return out[:q.shape[0]]

    def _samples(self, a, mode, n, thresholds=None, want_dists=True, chunk=None):
        ctx = self._ctx()
        index = self._index()
        L = a.shape[0]
        th = _thresholds(thresholds) if thresholds is not None else np.zeros(0)
        dists = np.zeros((max(L, 1), n)) if want_dists else None
        counts = np.zeros((max(L, 1), max(th.size, 1)), np.int32) if th.size else None
        if L:
            ctx.chk(getattr(ctx.L, self._samples_fn)(
                ctx.h, index, _p(a), L, mode, n, _p(th) if th.size else None, th.size, self._chunk(chunk),
                _p(dists) if want_dists else None, _p(counts, C.c_int32) if counts is not None else None))
        return (dists[:L] if want_dists else None), (counts[:L, :th.size] if counts is not None else None)

    def ComputeDistPoint(self, point):
        return float(self.ComputeDistPoints(np.asarray(point, np.float64).reshape(1, 3))[0])

    def _chunk(self, chunk):
        return int(self.chunk if chunk is None else chunk)

    def ComputeDistLine(self, line, n_samples=1000):
        """mean distance of n_samples points start + (i / (n - 1)) (end - start), summed in order"""
        n = int(n_samples)
        if n <= 2:
            raise ValueError("n_samples should be >= 3")
        _check_n(n, 3)
        d, _ = self._samples(lines_array([line]), 1, n)
        s = 0.0
        for v in d[0].tolist():  # std::accumulate: sequential
            s += v
        return s / float(n)

    def ComputeInlierRatios(self, lines, thresholds, n_samples=1000, chunk=None):
        """(L, T) ratios counter / n of samples within (<=) each threshold: one distance pass for all thresholds"""
        n = _check_n(n_samples)
        a = lines_array(lines)
        th = _thresholds(thresholds)
        if a.shape[0] == 0 or th.size == 0:
            return np.zeros((a.shape[0], th.size))
        _, c = self._samples(a, 0, n, th, want_dists=False, chunk=chunk)
        return c.astype(np.float64) / float(n)

    def ComputeInlierRatio(self, line, threshold, n_samples=1000):
        return float(self.ComputeInlierRatios([line], [float(threshold)], n_samples)[0, 0])

    def _segs(self, lines, threshold, n_samples, inlier):
        n = _check_n(n_samples)
        a = lines_array(lines)
        if a.shape[0] == 0:
            return []
        d, _ = self._samples(a, 0, n)
        return _segments(a, d, float(threshold), n, inlier)

    def ComputeInlierSegs(self, lines, threshold, n_samples=1000):
        return self._segs(lines, threshold, n_samples, True)

    def ComputeOutlierSegs(self, lines, threshold, n_samples=1000):
        return self._segs(lines, threshold, n_samples, False)


class PointCloudEvaluator(_SampledEvaluator):
    """evaluation/point_cloud_evaluator.h: nearest-point distances to a GT point cloud, on a device index."""

    _nearest_fn, _samples_fn, _free_fn = "lt_pcd_nearest_dists", "lt_pcd_line_samples", "lt_pcd_free"

    def __init__(self, points=None, device=0, chunk=0):
        self.device = int(device)
        self.chunk = int(chunk)
        self._torch = None
        if points is None:
            raise ValueError("PointCloudEvaluator: an empty point cloud cannot be evaluated against")
        if _native.is_torch(points):
            import torch
            if points.dim() != 2 or points.shape[1] != 3 or points.dtype not in (torch.float32, torch.float64):
                raise ValueError("PointCloudEvaluator: a tensor must be (N, 3) float32 or float64")
            if not points.is_contiguous():
                raise ValueError("PointCloudEvaluator: the tensor must be contiguous")
            if points.shape[0] == 0:
                raise ValueError("PointCloudEvaluator: empty point cloud")
            if not bool(torch.isfinite(points).all()):
                raise ValueError("PointCloudEvaluator: non-finite point coordinate")
            # a GPU tensor is read in place, and the evaluator runs on the tensor's device: no device to refuse
            if _native.check_device(points, host=False, device=None, who="PointCloudEvaluator", what="the tensor"):
                self.device = points.device.index or 0
                self._torch = points
                self.points = None
            else:
                self.points = _native.to_host(points).astype(np.float64).reshape(-1, 3)
        else:
            if isinstance(points, (list, tuple)):
                arr = np.stack([np.asarray(p, np.float64).reshape(3) for p in points], 0) if len(points) else \
                    np.zeros((0, 3))
            else:
                arr = np.asarray(points)
                if arr.dtype != np.float32:
                    arr = arr.astype(np.float64)
                arr = arr.reshape(-1, 3) if arr.size else np.zeros((0, 3))
            if arr.shape[0] == 0:
                raise ValueError("PointCloudEvaluator: empty point cloud")
            if not np.isfinite(arr).all():
                raise ValueError("PointCloudEvaluator: non-finite point coordinate")
            self.points = np.ascontiguousarray(arr.astype(np.float64))
        self.n_points = int(self._torch.shape[0] if self._torch is not None else self.points.shape[0])

    # ---- index -------------------------------------------------------------------------------------------------------
    def _build(self, perm=None):
        ctx = self._ctx()
        self._free()
        out = C.c_void_p()
        pp = None if perm is None else np.ascontiguousarray(perm, np.uint32)
        t = self._torch
        src, is_f64 = (self.points, 1) if t is None else (t, int(str(t.dtype) == "torch.float64"))
        if t is not None:
            _native.wait_for_torch(self.device)
        ctx.chk(ctx.L.lt_pcd_build(ctx.h, C.c_void_p(_native.address(src)), src.shape[0], is_f64, int(t is not None),
                                   None if pp is None else pp.ctypes.data, C.byref(out)))
        self._handle = out

    def _index(self):
        if self._handle is None:
            self._build()
        return self._handle

    def Build(self):
        self._build()

    def _digest(self):
        if self._torch is not None:
            pts = self._torch.detach().to("cpu", dtype=self._torch.dtype).numpy().astype(np.float64)
        else:
            pts = self.points
        return hashlib.sha256(np.ascontiguousarray(pts, "<f8").tobytes()).digest()

    def Save(self, filename):
        """the project's own index file: magic, point count, SHA-256 of the points (float64), the index order"""
        ctx = self._ctx()
        pcd = self._index()
        perm = np.zeros(self.n_points, np.uint32)
        ctx.chk(ctx.L.lt_pcd_get_perm(ctx.h, pcd, perm.ctypes.data))
        with open(filename, "wb") as f:
            f.write(_MAGIC)
            f.write(struct.pack("<q", self.n_points))
            f.write(self._digest())
            f.write(perm.astype("<u4").tobytes())

    def Load(self, filename):
        with open(filename, "rb") as f:
            head = f.read(len(_MAGIC))
            if head != _MAGIC:
                raise ValueError(f"{filename}: not a limap_amd point-cloud index (an index saved by limap's nanoflann "
                                 "KDTree cannot be loaded; call Build() and Save() instead)")
            (n,) = struct.unpack("<q", f.read(8))
            dig = f.read(32)
            perm = np.frombuffer(f.read(4 * max(n, 0)), "<u4")
        if n != self.n_points or perm.size != n:
            raise ValueError(f"{filename}: the index is of {n} points, this evaluator has {self.n_points}")
        if dig != self._digest():
            raise ValueError(f"{filename}: the index was saved for other points than this evaluator's")
        self._build(perm.astype(np.uint32))

    # ---- queries -----------------------------------------------------------------------------------------------------
    def ComputeDistsforEachPoint(self, lines, chunk=None):
        """per cloud point (constructor order): min over the lines of Line3d::point_distance; DBL_MAX without lines"""
        a = lines_array(lines)
        ctx = self._ctx()
        pcd = self._index()
        out = np.zeros(self.n_points)
        ctx.chk(ctx.L.lt_lines_point_dists(ctx.h, pcd, _p(a) if a.shape[0] else None, a.shape[0],
                                           self._chunk(chunk), _p(out)))
        return out

    def ComputeDistsforEachPoint_KDTree(self, lines):
        raise NotImplementedError(
            "ComputeDistsforEachPoint_KDTree is an approximation whose line sampling is wrong in limap "
            "(interval = length / (n - 1) scales an unnormalised direction) and whose ties depend on the kd-tree; "
            "use ComputeDistsforEachPoint, which is exact and runs on the GPU")


def _segments(a, d, threshold, n, inlier):
    """ComputeInlierSegsOneLine / ComputeOutlierSegsOneLine (base_evaluator.cc:47-151) from the sample distances"""
    interval = 1.0 / n
    res = []
    for k in range(a.shape[0]):
        s, e = a[k, 0:3], a[k, 3:6]
        v = e - s
        flags = (d[k] <= threshold) if inlier else ~(d[k] <= threshold)
        idx = np.flatnonzero(np.diff(np.concatenate([[0], flags.astype(np.int8), [0]])))
        for r0, r1 in zip(idx[0::2].tolist(), idx[1::2].tolist()):
            res.append(Line3d(s + (r0 * interval) * v, s + (r1 * interval) * v))
    return res


class RefLineEvaluator:
    """evaluation/refline_evaluator.h: length recall of lines against reference lines and back"""

    def __init__(self, ref_lines=None, device=0, chunk=0):
        self.ref = lines_array([] if ref_lines is None else ref_lines)
        self.device = int(device)
        self.chunk = int(chunk)

    def SumLength(self):
        s = 0.0
        for v in line_lengths(self.ref).tolist():
            s += v
        return s

    def _counts(self, q, lines, thresholds, n, chunk):
        th = _thresholds(thresholds)
        n = _check_n(n)
        c = np.zeros((max(q.shape[0], 1), max(th.size, 1)), np.int32)
        if q.shape[0] and th.size:
            ctx = _context(self.device)
            ctx.chk(ctx.L.lt_refline_counts(ctx.h, _p(q), q.shape[0], _p(lines) if lines.shape[0] else None,
                                            lines.shape[0], n, _p(th), th.size, int(self.chunk if chunk is None else chunk),
                                            _p(c, C.c_int32)))
        return c[:q.shape[0], :th.size], th

    def _recall(self, q, lines, thresholds, n, chunk):
        c, th = self._counts(q, lines, thresholds, n, chunk)
        lens = line_lengths(q).tolist()
        out = np.zeros(th.size)
        for t in range(th.size):  # recall += length * double(counter) / num_samples, reference lines in order
            r = 0.0
            for k, ln in enumerate(lens):
                r += ln * float(c[k, t]) / n
            out[t] = r
        return out

    def ComputeRecallRefs(self, lines, thresholds, num_samples=1000, chunk=None):
        return self._recall(self.ref, lines_array(lines), thresholds, num_samples, chunk)

    def ComputeRecallTesteds(self, lines, thresholds, num_samples=1000, chunk=None):
        return self._recall(lines_array(lines), self.ref, thresholds, num_samples, chunk)

    def ComputeRecallRef(self, lines, threshold, num_samples=1000):
        return float(self.ComputeRecallRefs(lines, [float(threshold)], num_samples)[0])

    def ComputeRecallTested(self, lines, threshold, num_samples=1000):
        return float(self.ComputeRecallTesteds(lines, [float(threshold)], num_samples)[0])


class MeshEvaluator(_SampledEvaluator):
    """evaluation/mesh_evaluator.h: distances to a GT triangle mesh, on a device triangle index.  The point-to-triangle
    distance is Ericson's closest point in a stated FP64 operation order; agreement with
    libigl's point_simplex_squared_distance is not claimed."""

    _nearest_fn, _samples_fn, _free_fn = "lt_mesh_nearest_dists", "lt_mesh_line_samples", "lt_mesh_free"

    def __init__(self, filename, mpau, device=0, chunk=0):
        from .io import read_mesh
        V, F = read_mesh(filename)
        self._init(V, F, mpau, device, chunk)

    @classmethod
    def from_arrays(cls, V, F, mpau=1.0, device=0, chunk=0):
        """a mesh in memory: V (nv, 3) vertices, F (nf, 3) 0-based vertex indices"""
        self = cls.__new__(cls)
        self._init(V, F, mpau, device, chunk)
        return self

    def _init(self, V, F, mpau, device, chunk):
        self.device = int(device)
        self.chunk = int(chunk)
        V = np.ascontiguousarray(np.asarray(V, np.float64).reshape(-1, 3))
        F = np.asarray(F)
        if F.size and not np.issubdtype(F.dtype, np.integer):
            raise ValueError("MeshEvaluator: face indices must be integers")
        F = np.ascontiguousarray(F.astype(np.int64).reshape(-1, 3))
        self.mpau = float(mpau)
        if not math.isfinite(self.mpau):
            raise ValueError("MeshEvaluator: non-finite mpau")
        if F.shape[0] == 0:
            raise ValueError("MeshEvaluator: a mesh without faces")
        if F.min() < 0 or F.max() >= V.shape[0]:
            raise ValueError(f"MeshEvaluator: face index out of range (vertices: {V.shape[0]})")
        with np.errstate(over="ignore", invalid="ignore"):
            if not np.isfinite(V * self.mpau).all():
                raise ValueError("MeshEvaluator: non-finite vertex coordinate (after scaling by mpau)")
        self.V, self.F = V, F
        self.n_vertices, self.n_faces = V.shape[0], F.shape[0]

    def _index(self):
        if self._handle is None:
            ctx = self._ctx()
            out = C.c_void_p()
            ctx.chk(ctx.L.lt_mesh_build(ctx.h, self.V.ctypes.data, self.n_vertices, 1, 0, self.F.ctypes.data,
                                        self.n_faces, self.mpau, C.byref(out)))
            self._handle = out
        return self._handle

    def Build(self):
        """(re)builds the device index; the queries build it on first use"""
        self._free()
        self._index()


# ---- scripts/eval_hypersim.py:47-68, scripts/eval_tnt.py:22-59 ----------------------------------------------------------
def report_error_to_GT(evaluator, lines, thresholds=(0.001, 0.005, 0.01), n_samples=1000):
    """per threshold: length recall (lengths * ratios).sum() and precision 100 * (ratios > 0).sum() / L"""
    a = lines_array(lines)
    th = _thresholds(thresholds)
    lengths = line_lengths(a)
    ratios = evaluator.ComputeInlierRatios(a, th, n_samples)
    recall = np.array([(lengths * ratios[:, t]).sum() for t in range(th.size)])
    L = a.shape[0]
    precision = np.array([100 * (ratios[:, t] > 0).astype(int).sum() / L if L else math.nan for t in range(th.size)])
    return dict(thresholds=th, recall=recall, precision=precision, ratios=ratios, lengths=lengths)


def report_pc_recall_for_GT(evaluator, lines, thresholds=(0.001, 0.005, 0.01, 0.05, 0.1, 0.5, 1.0)):
    """per threshold: inliers (dists < th).sum() and point recall 100 * inliers / P"""
    th = _thresholds(thresholds)
    d = np.asarray(evaluator.ComputeDistsforEachPoint(lines))
    P = d.shape[0]
    inliers = np.array([int((d < t).sum()) for t in th.tolist()])
    return dict(thresholds=th, inliers=inliers, point_recall=100 * inliers / P, dists=d)
