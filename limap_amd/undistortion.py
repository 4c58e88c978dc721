"""limap.undistortion on the GPU: distorted COLMAP cameras, their images and their keypoints brought to pinhole
cameras -- the step ``runners/functions.py:undistort_images`` puts in front of ``line_triangulation``
(undistortion/undistort.{cc,py} of limap over COLMAP's ``UndistortImage``; names follow them):

    from limap_amd import undistortion as und
    cam = und.Camera("OPENCV", [fx, fy, cx, cy, k1, k2, p1, p2], cam_id=1, hw=(h, w))
    cams_u, imgs_u = und.undistort_images({7: cam}, {7: image})          # uint8 arrays or torch GPU tensors
    view = base.CameraView(cams_u[7].kvec(), q, t, hw=(cams_u[7].h(), cams_u[7].w()))

A whole batch of images, which may differ in size, channels and camera, is one launch of ``k_undist_warp``; keypoints
and the border scan of ``UndistortCamera`` run one lane per point through ``k_undist_points`` (which
is also the definition: the parts of COLMAP upstream calls are restated there as recalled).  ``host=True`` on a call
computes the same result, bit for bit, by the library's host path.  Built models: SIMPLE_PINHOLE, PINHOLE,
SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV; the fisheye family and FOV raise ``NotImplementedError``.
"""
import ctypes as C
import os

import numpy as np

from . import _capi, _native

__all__ = ["Camera", "undistort_camera", "undistort_image_camera", "undistort_images", "undistort_points",
           "undistort_points_scene", "timers"]

_context = _capi.per_device_contexts()
_p = _capi.ptr
_EPS = float(np.finfo(np.float64).eps)
MODEL_NAMES = {0: "SIMPLE_PINHOLE", 1: "PINHOLE", 2: "SIMPLE_RADIAL", 3: "RADIAL", 4: "OPENCV", 5: "OPENCV_FISHEYE",
               6: "FULL_OPENCV", 7: "FOV", 8: "SIMPLE_RADIAL_FISHEYE", 9: "RADIAL_FISHEYE", 10: "THIN_PRISM_FISHEYE"}
# built models: id -> (parameter count, focal lengths)
_BUILT = {0: (3, 1), 1: (4, 2), 2: (4, 1), 3: (5, 1), 4: (8, 2), 6: (12, 2)}
_SIZE_MSG = "Error! The height and width of the given camera do not match the input image."
# counters the tests read: border scans made, warp launches (chunks) made
stats = {"border_scans": 0, "warp_calls": 0}


def _model_id(model):
    if isinstance(model, str):
        ids = {v: k for k, v in MODEL_NAMES.items()}
        if model not in ids:
            raise ValueError(f"undistortion: unknown camera model {model!r}")
        return ids[model]
    mid = int(model)
    if mid not in MODEL_NAMES:
        raise ValueError(f"undistortion: unknown camera model id {mid}")
    return mid


class Camera:
    """limap.base.Camera (colmap::Camera) for the models this module builds.  ``params`` in COLMAP's order, or a 3x3 K
    for the two pinhole models as upstream's constructor takes it."""

    def __init__(self, model, params, cam_id=-1, hw=None):
        self.model = _model_id(model)
        if self.model not in _BUILT:
            raise NotImplementedError(f"undistortion: camera model {MODEL_NAMES[self.model]} is not built")
        n, nf = _BUILT[self.model]
        p = np.asarray(params, np.float64)
        if p.shape == (3, 3):
            if self.model == 0:
                p = np.array([p[0, 0], p[0, 2], p[1, 2]])
            elif self.model == 1:
                p = np.array([p[0, 0], p[1, 1], p[0, 2], p[1, 2]])
            else:
                raise ValueError("undistortion: a K matrix gives only the pinhole models")
        p = p.reshape(-1).copy()
        if p.size != n:
            raise ValueError(f"undistortion: {MODEL_NAMES[self.model]} takes {n} parameters, got {p.size}")
        if not np.isfinite(p).all():
            raise ValueError("undistortion: non-finite camera parameter")
        if (p[:nf] == 0).any():
            raise ValueError("undistortion: a focal length is 0")
        self.params = p
        self.camera_id = int(cam_id)
        self._h, self._w = (0, 0) if hw is None else (int(hw[0]), int(hw[1]))
        if hw is not None and (self._h < 1 or self._w < 1):
            raise ValueError("undistortion: image size below 1")

    # ---- queries ----
    def h(self):
        return self._h

    def w(self):
        return self._w

    def _nf(self):
        return _BUILT[self.model][1]

    def kvec(self):
        """(fx, fy, cx, cy) as ``CameraView`` takes it"""
        p, nf = self.params, self._nf()
        return np.array([p[0], p[nf - 1], p[nf], p[nf + 1]])

    def K(self):
        fx, fy, cx, cy = self.kvec()
        return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])

    def IsUndistorted(self):
        return not (np.abs(self.params[self._nf() + 2:]) > _EPS).any()

    def key(self):
        return (self.model, tuple(self.params.tolist()), self._h, self._w)

    def __eq__(self, other):
        return isinstance(other, Camera) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return f"Camera({MODEL_NAMES[self.model]}, {self.params.tolist()}, cam_id={self.camera_id}, hw=({self._h}, {self._w}))"

    def copy(self):
        return Camera(self.model, self.params, self.camera_id, (self._h, self._w) if self._h else None)

    def Rescale(self, new_w, new_h):
        new_w, new_h = int(new_w), int(new_h)
        if self._w < 1 or self._h < 1 or new_w < 1 or new_h < 1:
            raise ValueError("undistortion: image size below 1")
        sx, sy = new_w / self._w, new_h / self._h
        p, nf = self.params, self._nf()
        if nf == 1:
            p[0] *= (sx + sy) / 2
        else:
            p[0] *= sx
            p[1] *= sy
        p[nf] *= sx
        p[nf + 1] *= sy
        self._w, self._h = new_w, new_h
        return self


# ---- the native calls ----
def _cam_table(cams):
    tab = (_capi.LtUndistCamera * max(len(cams), 1))()
    for k, c in enumerate(cams):
        tab[k].model, tab[k].n_params = c.model, c.params.size
        for j, v in enumerate(c.params.tolist()):
            tab[k].params[j] = v
    return tab


def _points_raw(cams, xy, src_idx, dst_idx, host=False, device=0, n_threads=0):
    """-> (out (N, 2), status (N,), iters (N,)): point i through CamFromImg of cams[src_idx[i]] and ImgFromCam of
    cams[dst_idx[i]]"""
    xy = _capi.f64(xy).reshape(-1, 2)
    n = xy.shape[0]
    src_idx, dst_idx = _capi.i32(np.broadcast_to(src_idx, (n,))), _capi.i32(np.broadcast_to(dst_idx, (n,)))
    out = np.zeros((max(n, 1), 2))
    status, iters = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    tab = _cam_table(cams)
    args = (len(cams), tab, n, _p(xy), _p(src_idx, C.c_int32), _p(dst_idx, C.c_int32), _p(out), _p(status, C.c_int32),
            _p(iters, C.c_int32))
    if host:
        L = _capi.load_library()
        if L.lt_fn_undist_points_host(*args, int(n_threads)) != 0:
            _native.raise_host_error(L, "lt_fn_undist_host_error")
    else:
        ctx = _context(device)
        ctx.chk(ctx.L.lt_undist_points(ctx.h, *args))
    return out[:n], status[:n], iters[:n]


def _check_image(img):
    """-> (h, w, channels) of a uint8 image (H, W) or (H, W, C), an array or a tensor"""
    if str(img.dtype).split(".")[-1] != "uint8":
        raise ValueError(f"undistortion: an image must be uint8, got {img.dtype}")
    shape = tuple(img.shape)
    if len(shape) not in (2, 3) or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"undistortion: an image must be (H, W) or (H, W, C) with H, W >= 1, got shape {shape}")
    ch = 1 if len(shape) == 2 else shape[2]
    if ch not in (1, 3, 4):
        raise ValueError(f"undistortion: channel count outside {{1, 3, 4}}: {ch}")
    return shape[0], shape[1], ch


def _rows(img, ch):
    """the Operand of an image whose pixels are ch contiguous bytes and whose rows are a stride apart"""
    st = img.strides
    ok = st[1] == ch and (img.ndim == 2 or st[2] == 1) and st[0] >= img.shape[1] * ch
    return img if ok else img.contiguous()


def _warp_batch(items, host=False, device=0, max_chunk_bytes=1 << 30, n_threads=0):
    """items: (source camera, target camera, image) each -> the list of warped images, (target h, target w[, C]) uint8
    of the image's kind (NumPy array, or torch tensor on its device).  The warp itself, without limap's branches: an
    undistorted source camera is warped like any other.  Images of one kind go through the library in chunks whose
    source and target bytes stay under max_chunk_bytes (at least one image each)."""
    recs, outs, on_gpu = [], [None] * len(items), []
    for k, (cs, ct, img) in enumerate(items):
        h, w, ch = _check_image(img)
        if (cs.h(), cs.w()) != (h, w):
            raise RuntimeError(_SIZE_MSG)
        if ct.h() < 1 or ct.w() < 1:
            raise ValueError("undistortion: image size below 1")
        src = _rows(_native.operand(img, host=host, device=device, who="undistortion", what="the tensor"), ch)
        if src.on_device:
            import torch
            out = torch.empty((ct.h(), ct.w()) + src.shape[2:], dtype=torch.uint8, device=img.device)
            outs[k] = out
            on_gpu.append(k)
        else:
            out = np.zeros((ct.h(), ct.w()) + src.shape[2:], np.uint8)
            outs[k] = (out, img.device if _native.is_torch(img) else None)
        recs.append((k, src, src.strides[0], out, ct.w() * ch, src.on_device, cs, ct, ch))
    for kind in (0, 1):
        group = [r for r in recs if r[5] == kind]
        n = 0
        while n < len(group):
            m, used = n, 0
            while m < len(group):
                _, src, sst, out, ost, _, cs, ct, ch = group[m]
                nbytes = cs.h() * cs.w() * ch + ct.h() * ct.w() * ch
                if m > n and used + nbytes > max_chunk_bytes:
                    break
                used += nbytes
                m += 1
            tab_cams = []
            rows = {}
            arr = (_capi.LtUndistImage * (m - n))()
            for j, (_, src, sst, out, ost, dev, cs, ct, ch) in enumerate(group[n:m]):
                for c in (cs, ct):
                    if c.key() not in rows:
                        rows[c.key()] = len(tab_cams)
                        tab_cams.append(c)
                a = arr[j]
                a.src, a.dst = src.address, _native.address(out)
                a.src_stride, a.dst_stride = sst, ost
                a.src_w, a.src_h, a.dst_w, a.dst_h = cs.w(), cs.h(), ct.w(), ct.h()
                a.channels, a.src_cam, a.dst_cam, a.on_device = ch, rows[cs.key()], rows[ct.key()], dev
            tab = _cam_table(tab_cams)
            if host:
                L = _capi.load_library()
                if L.lt_fn_undist_warp_host(len(tab_cams), tab, m - n, arr, int(n_threads)) != 0:
                    _native.raise_host_error(L, "lt_fn_undist_host_error")
            else:
                if kind:
                    _native.wait_for_torch(device)
                ctx = _context(device)
                ctx.chk(ctx.L.lt_undist_warp(ctx.h, len(tab_cams), tab, m - n, arr))
            stats["warp_calls"] += 1
            n = m
    res = []
    for k, o in enumerate(outs):
        if k in on_gpu:
            res.append(o)
        else:
            out, back = o
            if back is not None:
                import torch
                out = torch.from_numpy(out).to(back)
            res.append(out)
    return res


# ---- COLMAP's UndistortCamera ----
def undistort_camera(camera, host=False, device=0, blank_pixels=0.0, min_scale=0.2, max_scale=2.0):
    """colmap::UndistortCamera with its default options: -> the PINHOLE camera of the undistorted image.  The border of
    a camera that is not a pinhole model goes through the point kernel (2 (w + h) points)."""
    blank_pixels, min_scale, max_scale = float(blank_pixels), float(min_scale), float(max_scale)
    if not 0.0 <= blank_pixels <= 1.0:
        raise ValueError("Check failed: blank_pixels in [0, 1]")
    if not min_scale > 0.0:
        raise ValueError("Check failed: min_scale > 0")
    if not min_scale <= max_scale or not np.isfinite(max_scale):
        raise ValueError("Check failed: min_scale <= max_scale")
    w, h = camera.w(), camera.h()
    if w < 1 or h < 1:
        raise ValueError("undistortion: image size below 1")
    target = Camera("PINHOLE", camera.kvec(), camera.camera_id, (h, w))
    if camera.model in (0, 1):
        return target
    ys, xs = np.arange(h) + 0.5, np.arange(w) + 0.5
    pts = np.concatenate([np.stack([np.full(h, 0.5), ys], 1), np.stack([np.full(h, w - 0.5), ys], 1),
                          np.stack([xs, np.full(w, 0.5)], 1), np.stack([xs, np.full(w, h - 0.5)], 1)])
    out, status, _ = _points_raw([camera, target], pts, 0, 1, host=host, device=device)
    stats["border_scans"] += 1
    if status.any():
        raise ValueError(f"undistortion: camera {camera.camera_id} ({MODEL_NAMES[camera.model]}): a border point has no "
                         f"undistorted position (point {pts[int(np.nonzero(status)[0][0])].tolist()})")
    left, right, top, bottom = out[:h, 0], out[h:2 * h, 0], out[2 * h:2 * h + w, 1], out[2 * h + w:, 1]
    ext = np.array([left.min(), left.max(), right.min(), right.max(), top.min(), top.max(), bottom.min(), bottom.max()])
    res = np.zeros(4)
    L = _capi.load_library()
    fx, fy, cx, cy = target.params
    if L.lt_fn_undist_scale(w, h, cx, cy, _p(ext), blank_pixels, min_scale, max_scale, _p(res)) != 0:
        _native.raise_host_error(L, "lt_fn_undist_host_error", f"undistortion: camera {camera.camera_id}: ")
    return Camera("PINHOLE", [fx, fy, res[2], res[3]], camera.camera_id, (int(res[1]), int(res[0])))


# ---- limap's own part ----
def _as_upstream_returns(camera):
    """undistort.py:20-47 for a camera with IsUndistorted()"""
    if camera.model in (0, 1):
        return camera
    return Camera("SIMPLE_PINHOLE" if camera.model == 2 else "PINHOLE", camera.K(), cam_id=camera.camera_id,
                  hw=(camera.h(), camera.w()))


def _pil():
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("undistortion: reading and writing image files needs PIL (pass arrays or tensors instead)") from e
    return Image


def _read(path):
    img = _pil().open(path)
    if img.mode not in ("L", "RGB", "RGBA"):
        img = img.convert("RGB")
    return np.asarray(img)


def _write(path, img):
    img = _native.to_host(img)
    _pil().fromarray(img[:, :, 0] if img.ndim == 3 and img.shape[2] == 1 else img).save(path)


def _is_path(x):
    return isinstance(x, (str, os.PathLike))


def _plan(camera, img, cache, host, device):
    """-> (source camera, target camera, rotated) of one image of a distorted camera (undistort.cc:18-35); the border
    scan of a camera that compares equal to an earlier one is taken from the cache"""
    h, w, _ = _check_image(img)
    cam, rotated = camera, False
    if (cam.h(), cam.w()) != (h, w):
        if (cam.w(), cam.h()) != (h, w):
            raise RuntimeError(_SIZE_MSG)
        rotated = True
        cam = camera.copy().Rescale(w, h)
    if cam.key() not in cache:
        cache[cam.key()] = undistort_camera(cam, host=host, device=device)
    return cam, cache[cam.key()], rotated


def _finish(camera, target, rotated):
    out = target.copy()
    out.camera_id = camera.camera_id
    if rotated:
        out.Rescale(target.h(), target.w())
    return out


def undistort_images(cameras, images, output_dir=None, host=False, device=0, max_chunk_bytes=1 << 30):
    """dicts img_id -> Camera and img_id -> array | tensor | path: -> (dict img_id -> undistorted Camera, dict img_id ->
    undistorted image).  One border scan per distinct camera, one warp launch per chunk.  With output_dir the images
    are also written as ``image{img_id:08d}.png``."""
    ids = sorted(images)
    loaded = {}
    for i in ids:
        if i not in cameras:
            raise ValueError(f"undistortion: image {i} has no camera")
        loaded[i] = _read(images[i]) if _is_path(images[i]) else images[i]
        _check_image(loaded[i])
        _native.check_device(loaded[i], host=host, device=device, who="undistortion", what="the tensor")
    cache, cams_out, imgs_out, items, item_ids, plans = {}, {}, {}, [], [], {}
    for i in ids:
        cam = cameras[i]
        if cam.IsUndistorted():
            cams_out[i] = _as_upstream_returns(cam)
            imgs_out[i] = loaded[i].clone() if _native.is_torch(loaded[i]) else np.array(loaded[i])
            continue
        src, target, rotated = _plan(cam, loaded[i], cache, host, device)
        plans[i] = (target, rotated)
        items.append((src, target, loaded[i]))
        item_ids.append(i)
    for i, out in zip(item_ids, _warp_batch(items, host=host, device=device, max_chunk_bytes=max_chunk_bytes)):
        imgs_out[i] = out
        cams_out[i] = _finish(cameras[i], *plans[i])
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        for i in ids:
            _write(os.path.join(output_dir, f"image{int(i):08d}.png"), imgs_out[i])
    return cams_out, imgs_out


def undistort_image_camera(camera, image_or_path, out_path=None, host=False, device=0):
    """undistort.py:5-47.  With paths: reads imname_in, writes imname_out, returns the undistorted camera, as upstream
    does (through PIL).  With an array or tensor: -> (undistorted camera, undistorted image)."""
    by_path = _is_path(image_or_path)
    cams, imgs = undistort_images({0: camera}, {0: image_or_path}, host=host, device=device)
    if out_path is not None:
        _write(out_path, imgs[0])
    return cams[0] if by_path else (cams[0], imgs[0])


def undistort_points(points, distorted_camera, undistorted_camera, host=False, device=0, return_status=False):
    """undistort.cc:48-68: -> (N, 2) float64, the keypoints on the undistorted image.  A point without an undistorted
    position (status 1: a singular Jacobian or an overflow of the Newton iteration) comes back as NaN with
    return_status (-> points, status, iterations) and raises ValueError without."""
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    out, status, iters = _points_raw([distorted_camera, undistorted_camera], pts, 0, 1, host=host, device=device)
    if return_status:
        return out, status, iters
    if status.any():
        raise ValueError(f"undistortion: point {int(np.nonzero(status)[0][0])} has no undistorted position")
    return out


def undistort_points_scene(points_by_image, dist_cameras, undist_cameras, host=False, device=0, return_status=False):
    """the keypoints of a whole scene in one call: dicts img_id -> (N, 2) points, img_id -> distorted Camera, img_id ->
    undistorted Camera -> dict img_id -> (N, 2) (with return_status also the dicts of statuses and iterations)"""
    ids = sorted(points_by_image)
    cams, rows = [], {}

    def row(c):
        if c.key() not in rows:
            rows[c.key()] = len(cams)
            cams.append(c)
        return rows[c.key()]

    pts = [np.asarray(points_by_image[i], np.float64).reshape(-1, 2) for i in ids]
    src = [np.full(len(p), row(dist_cameras[i]), np.int32) for i, p in zip(ids, pts)]
    dst = [np.full(len(p), row(undist_cameras[i]), np.int32) for i, p in zip(ids, pts)]
    if not ids:
        return ({}, {}, {}) if return_status else {}
    out, status, iters = _points_raw(cams, np.concatenate(pts), np.concatenate(src), np.concatenate(dst), host=host,
                                     device=device)
    off = np.concatenate([[0], np.cumsum([len(p) for p in pts])])
    if not return_status and status.any():
        k = int(np.nonzero(status)[0][0])
        j = int(np.searchsorted(off, k, side="right")) - 1
        raise ValueError(f"undistortion: image {ids[j]} point {k - int(off[j])} has no undistorted position")
    cut = lambda a: {i: a[off[k]:off[k + 1]].copy() for k, i in enumerate(ids)}  # noqa: E731
    return (cut(out), cut(status), cut(iters)) if return_status else cut(out)


def timers(device=0):
    """lt_undist_get_timers of the last device call: host ms of validation + upload, device ms of the kernel, host ms
    of the download; its work units (runs of 4 target pixels) or points"""
    return _context(device).module_timers("lt_undist_get_timers", 4)
