"""limap.features' line patches on the GPU: for a 2D line, an oriented box around it -- stretched along the line,
``range_perp`` wide across it -- resampled from a dense feature map by bilinear interpolation (features/
line_patch_extractor.cc, featurepatch.h, extract_line_patches.py of limap; names follow them), and the patch side of
``optimize/extract_track_patches_s2dnet.py`` for a whole scene:

    from limap_amd import features
    ext = features.get_line_patch_extractor({"k_stretch": 1.0, "t_stretch": 10, "range_perp": 16}, channels=128)
    patches = ext.ExtractLinePatches(line2ds, feature)                  # feature: (H, W, C) array or torch GPU tensor
    by_pair = features.extract_track_patches(cfg, tracks, imagecols, feature_of_image)   # {(track_id, img_id): PatchInfo}

All patches of one feature map are one launch of ``k_patch_gather``, which reads the map in place -- a NumPy array is
uploaded once, a torch GPU tensor is read where it lies, permuted or not (which is also the
definition).  ``host=True`` on a call computes the same bits by the library's host path; ``dtype=`` chooses the output
(float64 is upstream's ``PatchInfo_f64``; float32 and float16 are what ``write_patch`` stores, rounded once from the
FP64 value); ``device_out=True`` returns torch tensors that view one packed device buffer instead of a download.
The networks that produce the feature maps are not part of this module: ``load_extractor`` raises.
"""
import ctypes as C
import os

import numpy as np

from . import _capi, _native
from . import base as _base

__all__ = ["LinePatchExtractorOptions", "PatchInfo", "PatchInfo_f16", "PatchInfo_f32", "PatchInfo_f64",
           "LinePatchExtractor", "get_line_patch_extractor", "extract_line_patch_one_image", "extract_line_patches",
           "extract_track_patches", "write_patch", "load_patch", "load_extractor", "line2d_ranges", "ranges_from_arrays", "timers"]

_context = _capi.per_device_contexts()
_p = _capi.ptr
_DTYPES = {"float16": _capi.PATCH_F16, "float32": _capi.PATCH_F32, "float64": _capi.PATCH_F64}
TIMER_KEYS = ["host_ms", "kernel_ms", "download_ms", "patches", "chunks", "vector_form", "blocks", "out_bytes"]


class LinePatchExtractorOptions:
    """line_patch_extractor.h:19-31: keys of the dict that are present overwrite the C++ defaults (range_perp is 20
    there; cfgs/refinement/default.yaml passes 16)."""

    def __init__(self, cfg=None):
        self.k_stretch, self.t_stretch, self.range_perp = 1.0, 10, 20
        if isinstance(cfg, LinePatchExtractorOptions):
            cfg = cfg.as_dict()
        cfg = cfg or {}
        if "k_stretch" in cfg:
            self.k_stretch = float(cfg["k_stretch"])
        for key in ("t_stretch", "range_perp"):
            if key in cfg:
                v = cfg[key]
                if int(v) != v:
                    raise ValueError(f"features: {key} must be an integer, got {v!r}")
                setattr(self, key, int(v))

    def as_dict(self):
        return dict(k_stretch=self.k_stretch, t_stretch=self.t_stretch, range_perp=self.range_perp)

    def _struct(self):
        if not -2 ** 31 <= self.t_stretch < 2 ** 31 or not -2 ** 31 <= self.range_perp < 2 ** 31:
            raise ValueError("features: t_stretch or range_perp outside the range of an int")
        return _capi.LtPatchConfig(float(self.k_stretch), int(self.t_stretch), int(self.range_perp))


class PatchInfo:
    """featurepatch.h:18-28: ``array`` (patch_h, patch_w, C), ``R`` = [perp; direc] (2, 2), ``tvec`` the corner (2,),
    ``img_hw`` = (H, W) of the feature map.  local_xy = R (xy - tvec)."""

    def __init__(self, array=None, R=None, tvec=None, img_hw=(0, 0)):
        self.array = array
        self.R = np.zeros((2, 2)) if R is None else np.asarray(R, np.float64).reshape(2, 2)
        self.tvec = np.zeros(2) if tvec is None else np.asarray(tvec, np.float64).reshape(2)
        self.img_hw = (int(img_hw[0]), int(img_hw[1]))


PatchInfo_f16 = PatchInfo_f32 = PatchInfo_f64 = PatchInfo


def _dtype_code(dtype):
    name = "float64" if dtype is None else (dtype if isinstance(dtype, str) else np.dtype(dtype).name)
    if name not in _DTYPES:
        raise ValueError(f"features: the output dtype must be float16, float32 or float64, got {dtype!r}")
    return name, _DTYPES[name]


def _feature_map(feature, host, device):
    """-> (lt_feature_map, (H, W, C), what keeps the memory alive, on_device); any strides are read in place"""
    f = _native.operand(feature, host=host, device=device, who="features", what="the tensor")
    if f.dtype not in _DTYPES:
        raise ValueError("features: a feature map must be float16, float32 or float64, got "
                         f"{getattr(feature, 'dtype', f.dtype)}")
    if f.ndim != 3:
        raise ValueError(f"features: a feature map must be (H, W, C), got shape {f.shape}")
    if min(f.shape) < 1:
        raise ValueError(f"features: a feature map must have H, W, C >= 1, got shape {f.shape}")
    return _capi.LtFeatureMap(f.address, *f.shape, *f.strides, _DTYPES[f.dtype], f.on_device), f.shape, f.keep, f.on_device


def _lines4(line2ds):
    """a list of Line2d or of (x1, y1, x2, y2) rows, or an (n, 4) array -> (n, 4) float64"""
    if isinstance(line2ds, np.ndarray):
        return _capi.f64(line2ds).reshape(-1, 4)
    rows = [np.concatenate([np.asarray(l.start, np.float64).reshape(2), np.asarray(l.end, np.float64).reshape(2)])
            if hasattr(l, "start") else np.asarray(l, np.float64).reshape(4) for l in line2ds]
    return _capi.f64(rows).reshape(-1, 4)


def _extract(options, line2ds, feature, host=False, dtype=None, device_out=False, device=0, max_chunk_bytes=0,
             n_threads=0):
    """-> list of PatchInfo, one per line, from one feature map (one launch per output chunk)"""
    name, code = _dtype_code(dtype)
    cfg = LinePatchExtractorOptions(options)._struct()
    lines = _lines4(line2ds)
    n = len(lines)
    if host and device_out:
        raise ValueError("features: device_out needs the device path (host=False)")
    fm, (H, W, Cc), keep, on_device = _feature_map(feature, host, device)
    L = _capi.load_library()
    R = np.zeros((max(n, 1), 4))
    tv = np.zeros((max(n, 1), 2))
    hs = np.zeros(max(n, 1), np.int32)
    off = np.zeros(n + 1, np.int64)
    lp = _p(lines if n else np.zeros((1, 4)))
    if L.lt_fn_patch_geometry(C.byref(cfg), Cc, n, lp, _p(R), _p(tv), _p(hs, C.c_int32), _p(off, C.c_int64)) != 0:
        _native.raise_host_error(L, "lt_fn_patch_host_error", "features: ")
    total, pw = int(off[n]), cfg.range_perp + 1
    if host:
        flat = np.empty(max(total, 1), np.dtype(name))
        if L.lt_fn_patch_extract_host(C.byref(cfg), C.byref(fm), n, lp, code, flat.ctypes.data, int(n_threads)) != 0:
            _native.raise_host_error(L, "lt_fn_patch_host_error", "features: ")
    else:
        ctx = _context(device)
        if device_out:
            import torch
            flat = torch.empty(max(total, 8), dtype=getattr(torch, name), device=f"cuda:{device}")
        else:
            flat = np.empty(max(total, 1), np.dtype(name))
        if on_device or device_out:
            _native.wait_for_torch(device)
        ctx.chk(ctx.L.lt_patch_extract(ctx.h, C.byref(cfg), C.byref(fm), n, lp, code, _native.address(flat),
                                       1 if device_out else 0, int(max_chunk_bytes)))
    del keep  # (held the map's memory until the call had returned)
    return [PatchInfo(flat[int(off[i]):int(off[i + 1])].reshape(int(hs[i]), pw, Cc), R[i].reshape(2, 2).copy(),
                      tv[i].copy(), (H, W)) for i in range(n)]


def _cam11(view):
    if hasattr(view, "kvec"):
        kvec = np.asarray(view.kvec, np.float64).reshape(4)
    else:
        K = np.asarray(view.K(), np.float64)
        kvec = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    if hasattr(view, "qvec") or hasattr(view, "_qvec_given"):
        q = np.asarray(getattr(view, "_qvec_given", getattr(view, "qvec", None)), np.float64).reshape(4)
        t = np.asarray(view.tvec, np.float64).reshape(3)
    else:
        q = np.asarray(view.pose.qvec, np.float64).reshape(4)
        t = np.asarray(view.pose.tvec, np.float64).reshape(3)
    return np.concatenate([kvec, q, t])


def line2d_ranges(tracks, pairs, views):
    """GetLine2DRange for many (track, image) pairs in one native call: ``tracks`` a list of LineTrack, ``pairs`` a
    list of (track index, image id), ``views`` the CameraView of every pair -> (len(pairs), 4) float64 ranges.  Raises
    ValueError naming the track and the image for a pair without a support, or whose range is not finite or whose 3D
    line is not in front of the camera."""
    T = len(tracks)
    line6 = np.zeros((max(T, 1), 6))
    sup_off = np.zeros(T + 1, np.int64)
    imgs, segs = [], []
    for t, tr in enumerate(tracks):
        line6[t, :3], line6[t, 3:] = np.asarray(tr.line.start, np.float64), np.asarray(tr.line.end, np.float64)
        if len(tr.image_id_list) != len(tr.line2d_list):
            raise ValueError(f"features: track {t}: image_id_list and line2d_list differ in length")
        for img_id, l2 in zip(tr.image_id_list, tr.line2d_list):
            imgs.append(int(img_id))
            segs.append(np.concatenate([np.asarray(l2.start, np.float64), np.asarray(l2.end, np.float64)]))
        sup_off[t + 1] = len(imgs)
    n = len(pairs)
    pt, pi = [p[0] for p in pairs], [p[1] for p in pairs]
    out, status = ranges_from_arrays(line6[:T], sup_off, imgs, segs, pt, pi, [_cam11(v) for v in views])
    bad = np.nonzero(status)[0]
    if len(bad):
        k = int(bad[0])
        why = ("has no supporting line" if status[k] == 1 else
               "projects to a range that is not finite or lies at or behind the camera plane")
        raise ValueError(f"features: track {int(pt[k])} {why} in image {int(pi[k])}")
    return out


def ranges_from_arrays(line6, sup_off, sup_img, sup_seg4, pair_track, pair_img, pair_cam11):
    """lt_fn_patch_ranges on its CSR arrays -> (ranges (n, 4), status (n,)): status 0, 1 without a support, 2 for a range
    that is not finite or a 3D line that is not in front of the camera"""
    T, n = len(sup_off) - 1, len(pair_track)
    line6 = _capi.f64(line6 if T else np.zeros((1, 6))).reshape(-1, 6)
    sup_off = _capi.i64(sup_off)
    sup_img = _capi.i32(sup_img if len(sup_img) else [0])
    sup_seg = _capi.f64(sup_seg4 if len(sup_seg4) else np.zeros((1, 4))).reshape(-1, 4)
    pt = _capi.i32(pair_track if n else [0])
    pi = _capi.i32(pair_img if n else [0])
    cams = _capi.f64(pair_cam11 if n else np.zeros((1, 11))).reshape(-1, 11)
    out = np.zeros((max(n, 1), 4))
    status = np.zeros(max(n, 1), np.int32)
    L = _capi.load_library()
    if L.lt_fn_patch_ranges(T, _p(line6), _p(sup_off, C.c_int64), _p(sup_img, C.c_int32), _p(sup_seg), n,
                            _p(pt, C.c_int32), _p(pi, C.c_int32), _p(cams), _p(out), _p(status, C.c_int32)) != 0:
        _native.raise_host_error(L, "lt_fn_patch_host_error", "features: ")
    return out[:n], status[:n]


class LinePatchExtractor:
    """line_patch_extractor.h:33-61 for any channel count.  Every extraction call takes ``host``, ``dtype``,
    ``device_out`` and ``device``."""

    def __init__(self, options=None, channels=None):
        self.options = LinePatchExtractorOptions(options)
        self.channels = None if channels is None else int(channels)
        if self.channels is not None and self.channels < 1:
            raise ValueError(f"features: channels must be >= 1, got {channels}")

    def _check_channels(self, feature):
        if self.channels is not None and len(feature.shape) == 3 and int(feature.shape[2]) != self.channels:
            raise ValueError(f"features: the extractor was made for {self.channels} channels, the feature map has "
                             f"{int(feature.shape[2])}")

    def ExtractLinePatch(self, line2d, feature, **kw):
        return self.ExtractLinePatches([line2d], feature, **kw)[0]

    def ExtractLinePatches(self, line2ds, feature, **kw):
        self._check_channels(feature)
        return _extract(self.options, line2ds, feature, **kw)

    def GetLine2DRange(self, track, image_id, view):
        r = line2d_ranges([track], [(0, int(image_id))], [view])[0]
        return _base.Line2d(r[0:2], r[2:4])

    def ExtractOneImage(self, track, image_id, view, feature, **kw):
        return self.ExtractLinePatch(self.GetLine2DRange(track, image_id, view), feature, **kw)

    def Extract(self, track, p_views, p_features, **kw):
        n_images = track.count_images()
        if len(p_views) != n_images:
            raise ValueError(f"Check failed: p_views.size() == n_images ({len(p_views)} vs. {n_images})")
        if len(p_features) != n_images:
            raise ValueError(f"Check failed: p_features.size() == n_images ({len(p_features)} vs. {n_images})")
        ids = track.GetSortedImageIds()
        return [self.ExtractOneImage(track, ids[i], p_views[i], p_features[i], **kw) for i in range(n_images)]


def get_line_patch_extractor(cfg, channels):
    """extract_line_patches.py:29-33; any channels >= 1 (upstream instantiates 1, 2, 3, 16, 32, 64 and 128)"""
    return LinePatchExtractor(LinePatchExtractorOptions(cfg), channels)


def extract_line_patch_one_image(cfg, track, img_id, camview, feature, **kw):
    return get_line_patch_extractor(cfg, feature.shape[2]).ExtractOneImage(track, img_id, camview, feature, **kw)


def extract_line_patches(cfg, track, p_camviews, p_features, **kw):
    return get_line_patch_extractor(cfg, p_features[0].shape[2]).Extract(track, p_camviews, p_features, **kw)


def write_patch(fname, patch, dtype="float16"):
    """extract_line_patches.py:5-15: np.savez with the keys array, R, tvec, img_hw"""
    array = _native.to_host(patch.array)
    if dtype == "float16":
        array = array.astype(np.float16)
    elif dtype == "float32":
        array = array.astype(np.float32)
    with open(fname, "wb") as f:
        np.savez(f, array=array, R=patch.R, tvec=patch.tvec, img_hw=np.asarray(patch.img_hw))


def load_patch(fname, dtype="float16"):
    """extract_line_patches.py:18-26 (the file holds plain arrays: no pickle is needed)"""
    with open(fname, "rb") as f:
        data = np.load(f, allow_pickle=False)
        return PatchInfo(data["array"], data["R"], data["tvec"], tuple(int(v) for v in data["img_hw"]))


def load_extractor(*args, **kwargs):
    raise NotImplementedError("limap_amd.features: the feature networks (S2DNet, ...) are not built; pass their output "
                              "maps to extract_track_patches")


def extract_track_patches(cfg, tracks, imagecols, features, output_dir=None, skip_exists=False, host=False, dtype=None,
                          device_out=False, device=0):
    """optimize/extract_track_patches_s2dnet.py:25-72 without the network: ``features`` is a mapping or a callable
    img_id -> (H, W, C) array or tensor.  The ranges of all (track, image) pairs come from one native call, the patches
    of an image from one launch.  cfg: {"patch": options, "channels": C, "dtype": name of the stored type}.  With
    output_dir the patches are written as ``track{t}/track{t}_img{i}.npy`` in cfg["dtype"] (default float16) and nothing
    is returned; without, -> {(track_id, img_id): PatchInfo} of ``dtype`` (default cfg["dtype"], else float64)."""
    ext = get_line_patch_extractor(cfg.get("patch"), cfg.get("channels"))
    get = features if callable(features) else features.__getitem__
    if output_dir is not None:
        if not skip_exists and os.path.isdir(output_dir):
            import shutil
            shutil.rmtree(output_dir)
        os.makedirs(output_dir, exist_ok=True)
    stored = cfg.get("dtype", "float16")  # what write_patch stores; extracting it directly is the same single rounding
    if output_dir is not None:
        dtype = stored
    elif dtype is None:
        dtype = cfg.get("dtype", "float64")
    pairs, views = [], []
    for track_id, track in enumerate(tracks):
        for img_id in track.GetSortedImageIds():
            pairs.append((track_id, int(img_id)))
            views.append(imagecols.camview(img_id))
        if output_dir is not None:
            os.makedirs(os.path.join(output_dir, f"track{track_id}"), exist_ok=True)
    ranges = line2d_ranges(tracks, pairs, views)
    by_image = {int(i): [] for i in imagecols.get_img_ids()}
    for k, (track_id, img_id) in enumerate(pairs):
        if img_id not in by_image:
            raise ValueError(f"features: track {track_id} is supported by image {img_id}, which the collection lacks")
        by_image[img_id].append(k)
    out = {}
    for img_id in imagecols.get_img_ids():
        ks = by_image[int(img_id)]
        if not ks:
            continue
        if output_dir is not None and skip_exists:
            ks = [k for k in ks if not os.path.exists(_patch_name(output_dir, pairs[k][0], img_id))]
            if not ks:
                continue
        patches = ext.ExtractLinePatches(ranges[ks], get(img_id), host=host, dtype=dtype, device_out=device_out,
                                         device=device)
        for k, patch in zip(ks, patches):
            if output_dir is not None:
                write_patch(_patch_name(output_dir, pairs[k][0], img_id), patch, dtype=stored)
            else:
                out[(pairs[k][0], int(img_id))] = patch
    return None if output_dir is not None else out


def _patch_name(output_dir, track_id, img_id):
    return os.path.join(output_dir, f"track{track_id}", f"track{track_id}_img{img_id}.npy")


def timers(device=0):
    """lt_patch_get_timers of the last device call as a dict (TIMER_KEYS)"""
    return dict(zip(TIMER_KEYS, _context(device).module_timers("lt_patch_get_timers", 8).tolist()))
