"""limap.pointsfm on the GPU: ``SfmModel`` with its visual neighbours and robust ranges, ``compute_neighbors`` and
``compute_metainfos`` (pointsfm/bindings.cc, sfm_model.{h,cc}, functions.py:20-55 of limap; names and defaults follow
them) -- step [A] of ``runners/line_triangulation.py`` without a limap + COLMAP install:

    from limap_amd import pointsfm
    model = pointsfm.SfmModel.from_arrays(img_ids, R, T, xyz, track_off, track_img)
    neighbors, ranges = pointsfm.compute_metainfos(cfg["sfm"], model, n_neighbors=cfg["n_neighbors"])

Upstream fills one ``std::map`` per image over every pair of images of every point track, serially.  Here every such
pair instance becomes a 64-bit key (image pair | triangulation angle), one device sort groups them, and one wave per
image ranks its partners (which is also the definition: the parts of colmap::mvs::Model upstream
calls are restated there, and ties and the arccosine's domain, which upstream leaves to the standard library, are
fixed).  ``host=True`` on a call computes the same result, bit for bit, by the library's host path.  The ranges are host
work.  ``ReadFromCOLMAP`` and the other file readers are out of scope: a model is built from arrays.
"""
import ctypes as C

import numpy as np

from . import _capi, _native

__all__ = ["SfmImage", "SfmModel", "compute_neighbors", "compute_metainfos", "timers"]

_context = _capi.per_device_contexts()
_p = _capi.ptr
_KINDS = {"overlap": 0, "iou": 1, "dice": 2}


def _f32(a, shape):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32).reshape(shape))


class SfmImage:
    """colmap::mvs::Image as ``CreateSfmImage`` builds it: K, R (row-major) and T narrowed to float32.  ``GetP`` /
    ``GetInvP`` are left out."""

    def __init__(self, name="", width=0, height=0, K=None, R=None, T=None):
        self.name, self.width, self.height = str(name), int(width), int(height)
        self.K = _f32(np.zeros(9) if K is None else K, (3, 3))
        self.R = _f32(np.zeros(9) if R is None else R, (3, 3))
        self.T = _f32(np.zeros(3) if T is None else T, (3,))

    def GetK(self):
        return self.K

    def GetR(self):
        return self.R

    def GetT(self):
        return self.T


class SfmModel:
    """pointsfm/sfm_model.h: images (index = position, plus a registered id each) and points with tracks of image
    *indices*"""

    def __init__(self):
        self.reg_image_ids = []
        self._names = []
        self._R, self._T = [], []           # per image float32 (3, 3), (3,)
        self._xyz, self._tracks = [], []    # per point, as added
        self._flat = None                   # (R, T, xyz, track_off, track_img), rebuilt after a change

    # ---- building ----
    def addImage(self, image, img_id=-1):
        if img_id == -1:
            if self.reg_image_ids and self.reg_image_ids[-1] != len(self.reg_image_ids) - 1:
                raise ValueError("Check failed: reg_image_ids.back() == reg_image_ids.size() - 1")
            img_id = len(self.reg_image_ids)
        self._unpack()
        self.reg_image_ids.append(int(img_id))
        self._names.append(image.name)
        self._R.append(image.R)
        self._T.append(image.T)
        self._flat = None

    def addPoint(self, x, y, z, image_ids):
        self._unpack()
        self._xyz.append((x, y, z))
        self._tracks.append(np.asarray(image_ids, np.int32).reshape(-1))
        self._flat = None

    @classmethod
    def from_arrays(cls, img_ids, R, T, xyz, track_off, track_img, names=None):
        """the whole model at once: registered ids (N,), R (N, 3, 3), T (N, 3), xyz (P, 3), and the tracks as CSR --
        point p is seen in the images track_img[track_off[p]:track_off[p + 1]] (indices into img_ids)"""
        m = cls()
        n = len(img_ids)
        m.reg_image_ids = [int(i) for i in img_ids]
        m._names = [str(s) for s in names] if names is not None else [f"image{i}" for i in m.reg_image_ids]
        R, T = _f32(R, (n, 3, 3)), _f32(T, (n, 3))
        if len(m._names) != n:
            raise ValueError("from_arrays: one name per image")
        xyz = _f32(xyz, (-1, 3))
        track_off = _capi.i64(np.asarray(track_off).reshape(-1))
        track_img = _capi.i32(np.asarray(track_img).reshape(-1))
        if len(track_off) != xyz.shape[0] + 1 or track_off[0] != 0 or (np.diff(track_off) < 0).any() \
                or track_off[-1] != len(track_img):
            raise ValueError("from_arrays: track_off must be the CSR offsets of track_img, one row per point")
        m._R, m._T = list(R), list(T)
        m._flat = (R, T, xyz, track_off, track_img)
        m._xyz = m._tracks = None  # kept flat; addPoint unpacks them first
        return m

    def _unpack(self):
        if self._xyz is None:
            _, _, xyz, off, img = self._flat
            self._xyz = [tuple(p) for p in xyz]
            self._tracks = [img[off[k]:off[k + 1]] for k in range(len(off) - 1)]

    def _arrays(self):
        if self._flat is None:
            self._unpack()
            n = len(self.reg_image_ids)
            off = np.zeros(len(self._tracks) + 1, np.int64)
            if self._tracks:
                off[1:] = np.cumsum([len(t) for t in self._tracks])
            img = _capi.i32(np.concatenate(self._tracks)) if off[-1] else np.zeros(0, np.int32)
            self._flat = (_f32(self._R, (n, 3, 3)) if n else np.zeros((0, 3, 3), np.float32),
                          _f32(self._T, (n, 3)) if n else np.zeros((0, 3), np.float32),
                          _f32(self._xyz, (-1, 3)) if self._xyz else np.zeros((0, 3), np.float32), off, img)
        return self._flat

    def ReadFromCOLMAP(self, path, sparse_path="sparse", images_path="images"):
        raise NotImplementedError("limap_amd.pointsfm reads no COLMAP files: build the model with SfmModel.from_arrays")

    # ---- queries ----
    def GetImageNames(self):
        return list(self._names)

    def ComputeNumPoints(self):
        _, _, _, _, img = self._arrays()
        n = len(self.reg_image_ids)
        if img.size and (img.min() < 0 or img.max() >= n):
            raise IndexError("unknown image index in a point track")
        return np.bincount(img, minlength=n).astype(np.int64).tolist()

    def _call(self, kind, num_images, min_triangulation_angle, host=False, device=0, n_threads=0, pairs=False):
        """-> (nb_off, nb) as image indices; with pairs also (ij (U, 2), shared (U,), angle (U,) float32)"""
        R, T, xyz, off, img = self._arrays()
        n = len(self.reg_image_ids)
        num_images = int(num_images)
        args = (n, _p(R, C.c_float), _p(T, C.c_float), xyz.shape[0], _p(xyz, C.c_float), _p(off, C.c_int64),
                _p(img, C.c_int32), int(kind), num_images, float(min_triangulation_angle))
        n_nb, n_pairs = C.c_int64(0), C.c_int64(0)
        if host:
            L = _capi.load_library()
            if L.lt_fn_sfm_neighbors_host(*args, int(n_threads), C.byref(n_nb), C.byref(n_pairs)) != 0:
                msg = L.lt_fn_sfm_host_error().decode(errors="replace")
                raise IndexError(msg) if msg.startswith("unknown") else ValueError(msg)
        else:
            ctx = _context(device)
            ctx.chk(ctx.L.lt_sfm_neighbors(ctx.h, *args, C.byref(n_nb), C.byref(n_pairs)))
        nb_off = np.zeros(n + 1, np.int64)
        nb = np.zeros(max(n_nb.value, 1), np.int32)
        u = n_pairs.value
        ij, shared, angle = np.zeros((max(u, 1), 2), np.int32), np.zeros(max(u, 1), np.int32), np.zeros(max(u, 1), np.float32)
        if host:
            if pairs:
                L.lt_fn_sfm_host_get(_p(nb_off, C.c_int64), _p(nb, C.c_int32), _p(ij, C.c_int32), _p(shared, C.c_int32),
                                     _p(angle, C.c_float))
            else:
                L.lt_fn_sfm_host_get(_p(nb_off, C.c_int64), _p(nb, C.c_int32), None, None, None)
        else:
            ctx.chk(ctx.L.lt_sfm_get(ctx.h, _p(nb_off, C.c_int64), _p(nb, C.c_int32)))
            if pairs:
                ctx.chk(ctx.L.lt_sfm_get_pairs(ctx.h, _p(ij, C.c_int32), _p(shared, C.c_int32), _p(angle, C.c_float)))
        res = (nb_off, nb[:n_nb.value])
        return res + (ij[:u], shared[:u], angle[:u]) if pairs else res

    def _neighbors(self, kind, num_images, min_triangulation_angle, **kw):
        """neighbors_vec_to_map: indices -> registered ids, a dict in ascending key order"""
        nb_off, nb = self._call(kind, num_images, min_triangulation_angle, **kw)
        ids = self.reg_image_ids
        order = sorted(range(len(ids)), key=lambda k: ids[k])
        out = {ids[k]: [] for k in order}
        for k in range(len(ids)):  # (a registered id given twice collects both lists, as std::map::insert + at do)
            out[ids[k]].extend(ids[j] for j in nb[nb_off[k]:nb_off[k + 1]].tolist())
        return out

    def GetMaxOverlapImages(self, num_images, min_triangulation_angle, host=False, device=0, n_threads=0):
        return self._neighbors(0, num_images, min_triangulation_angle, host=host, device=device, n_threads=n_threads)

    def GetMaxIoUImages(self, num_images, min_triangulation_angle, host=False, device=0, n_threads=0):
        return self._neighbors(1, num_images, min_triangulation_angle, host=host, device=device, n_threads=n_threads)

    def GetMaxDiceCoeffImages(self, num_images, min_triangulation_angle, host=False, device=0, n_threads=0):
        return self._neighbors(2, num_images, min_triangulation_angle, host=host, device=device, n_threads=n_threads)

    def pair_records(self, host=False, device=0, n_threads=0):
        """the image pairs that share a point, ascending: (ij (U, 2) image indices with i < j, shared (U,), the
        percentile triangulation angle (U,) float32 in radians)"""
        return self._call(0, 0, 0.0, host=host, device=device, n_threads=n_threads, pairs=True)[2:]

    def ComputeSharedPoints(self, host=False, device=0, n_threads=0):
        """per image index a dict partner index -> number of shared points"""
        ij, shared, _ = self.pair_records(host=host, device=device, n_threads=n_threads)
        out = [dict() for _ in self.reg_image_ids]
        for (i, j), s in zip(ij.tolist(), shared.tolist()):
            out[i][j] = s
            out[j][i] = s
        return [dict(sorted(d.items())) for d in out]

    def ComputeRanges(self, range_robust, k_stretch):
        """-> (lo, hi), two float64 3-vectors, computed in float32 as ``get_robust_range`` does"""
        xyz = self._arrays()[2]
        lo, hi = np.zeros(3), np.zeros(3)
        L = _capi.load_library()
        x = xyz if xyz.shape[0] else np.zeros((1, 3), np.float32)
        if L.lt_fn_sfm_ranges(xyz.shape[0], _p(x, C.c_float), float(range_robust[0]), float(range_robust[1]),
                              float(k_stretch), _p(lo), _p(hi)) != 0:
            _native.raise_host_error(L, "lt_fn_sfm_host_error")
        return lo, hi


def compute_neighbors(model, n_neighbors, min_triangulation_angle=1.0, neighbor_type="iou", host=False, device=0):
    """pointsfm/functions.py:20-38 -> dict img_id -> list of neighbour img_ids"""
    if neighbor_type not in _KINDS:
        raise NotImplementedError
    return model._neighbors(_KINDS[neighbor_type], n_neighbors, min_triangulation_angle, host=host, device=device)


def compute_metainfos(cfg, model, n_neighbors=20, host=False, device=0):
    """pointsfm/functions.py:41-55 -> (neighbors, ranges) as ``io.save_txt_metainfos``, ``SetRanges`` and
    ``stream.StreamedTriangulation`` take them"""
    neighbors = compute_neighbors(model, n_neighbors, min_triangulation_angle=cfg["min_triangulation_angle"],
                                  neighbor_type=cfg["neighbor_type"], host=host, device=device)
    ranges = model.ComputeRanges(cfg["ranges"]["range_robust"], cfg["ranges"]["k_stretch"])
    return neighbors, ranges


def timers(device=0):
    """lt_sfm_get_timers of the last device call: host ms of setup + upload, the device stage, download; device ms of
    k_sfm_pairs, the key sort, k_sfm_segments, partner lists + selection; launches of k_sfm_segments"""
    return _context(device).module_timers("lt_sfm_get_timers", 8)
