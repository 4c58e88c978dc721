"""limap.line2d matching on the GPU: the two descriptor matchers that are pure linear algebra -- ``L2D2Matcher``
(line2d/L2D2/matcher.py: top-k and mutual nearest neighbour) and the top-k form of ``NNEndpointsMatcher``
(line2d/endpoints/matcher.py:71-111) -- with the reference's method names, plus one batched entry point for a scene:

    from limap_amd import matching
    matches = matching.match_scene(descinfos, neighbors, kind="l2d2", topk=10)   # img_id -> {ng_img_id: (n, 2) int32}
    for img_id in image_ids:
        triangulator.TriangulateImage(img_id, matches[img_id])

Scores are FP32 fmaf chains computed by the FP32-input MFMA, the top-k of every line is selected on chip
(lt_kernels_match.hip); equal scores rank by ascending neighbour line.  The ``topk == 0`` form
of the endpoints matcher (Sinkhorn), SuperGlue, SOLD2, LBD and GlueStick matchers are out of scope.
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import _capi
from . import io as limapio

__all__ = ["BaseMatcherOptions", "DefaultMatcherOptions", "BaseMatcher", "L2D2Matcher", "NNEndpointsMatcher",
           "match_scene", "match_pair_host", "timers", "MAX_TOPK", "MAX_DIM", "KINDS"]

MAX_TOPK = 64   # LT_MATCH_MAX_TOPK
MAX_DIM = 256   # LT_MATCH_MAX_DIM
KINDS = {"l2d2": 0, "endpoints": 1, "nn_endpoints": 1}
_KEY = {0: "line_descriptors", 1: "endpoints_desc"}

_context = _capi.per_device_contexts()


def _kind(kind):
    if isinstance(kind, str):
        if kind not in KINDS:
            raise ValueError(f"matching: unknown kind {kind!r}")
        return KINDS[kind]
    if int(kind) not in (0, 1):
        raise ValueError(f"matching: unknown kind {kind!r}")
    return int(kind)


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def _rows_of(descinfo, kind):
    """the descriptor rows of one image, (rows, dim) float32: NumPy array, or torch tensor where the input is one.
    Endpoints: limap keeps (dim, 2 M); the native layout is one row per endpoint."""
    d = descinfo[_KEY[kind]] if isinstance(descinfo, dict) else descinfo
    if _is_torch(d):
        import torch
        d = d.to(torch.float32)
        if d.dim() != 2:
            d = d.reshape(0, 0) if d.numel() == 0 else d
        if d.dim() != 2:
            raise ValueError(f"matching: descriptors must be 2-D, got shape {tuple(d.shape)}")
        return (d.t() if kind == 1 else d).contiguous()
    a = np.asarray(d, np.float32)
    if a.ndim != 2:
        if a.size:
            raise ValueError(f"matching: descriptors must be 2-D, got shape {a.shape}")
        a = a.reshape(0, 0)
    return np.ascontiguousarray(a.T if kind == 1 else a)


def _width(parts):
    dims = {int(p.shape[1]) for p in parts if p.shape[0] > 0}
    if len(dims) > 1:
        raise ValueError(f"matching: descriptor widths differ across the call: {sorted(dims)}")
    return dims.pop() if dims else 8


def timers(device=0):
    """lt_match_get_timers of the last native call: host ms of validation + upload, kernels, download, row bookkeeping"""
    out = np.zeros(4)
    ctx = _context(device)
    ctx.chk(ctx.L.lt_match_get_timers(ctx.h, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def _match_flat(parts, pair_off, pair_nb, kind, topk, device=0, want_scores=False):
    """the native call: parts = descriptor rows per image (all NumPy or all torch); returns row_off, rows, scores"""
    ctx = _context(device)
    dim = _width(parts)
    desc_off = np.zeros(len(parts) + 1, np.int64)
    desc_off[1:] = np.cumsum([p.shape[0] for p in parts])
    on_dev = 0
    keep = None
    if parts and all(_is_torch(p) for p in parts):
        import torch
        live = [p for p in parts if p.shape[0] > 0]
        if live and all(p.is_cuda for p in live):
            if any(p.device.index != device for p in live):
                raise ValueError(f"matching: descriptors on another device than cuda:{device}")
            keep = torch.cat(live, 0).contiguous()
            torch.cuda.synchronize(device)  # the context's stream does not wait for torch's streams
            dptr, on_dev = C.c_void_p(keep.data_ptr()), 1
        else:
            parts = [p.cpu().numpy() for p in parts]
    elif any(_is_torch(p) for p in parts):
        parts = [p.cpu().numpy() if _is_torch(p) else p for p in parts]
    if not on_dev:
        live = [p.reshape(-1, dim) for p in parts if p.shape[0] > 0]
        keep = np.ascontiguousarray(np.concatenate(live, 0), np.float32) if live else np.zeros((1, dim), np.float32)
        dptr = C.c_void_p(keep.ctypes.data)
    pair_off, pair_nb = _capi.i64(pair_off), _capi.i32(pair_nb)
    cfg = _capi.LtMatchConfig(int(kind), int(topk), on_dev, 1 if want_scores else 0)
    n_rows = C.c_int64(0)
    ctx.chk(ctx.L.lt_match_scene(ctx.h, len(parts), _capi.ptr(desc_off, C.c_int64), dptr, dim,
                                 _capi.ptr(pair_off, C.c_int64), _capi.ptr(pair_nb if len(pair_nb) else _capi.i32([0]), C.c_int32),
                                 C.byref(cfg), C.byref(n_rows)))
    n = int(n_rows.value)
    row_off = np.zeros(len(pair_nb) + 1, np.int64)
    rows = np.zeros((n, 2), np.int32)
    ctx.chk(ctx.L.lt_match_get(ctx.h, _capi.ptr(row_off, C.c_int64), _capi.ptr(rows, C.c_int32) if n else None))
    scores = None
    if want_scores:
        scores = np.zeros(n, np.float32)
        ctx.chk(ctx.L.lt_match_get_scores(ctx.h, scores.ctypes.data_as(C.POINTER(C.c_float)) if n else None))
    return row_off, rows, scores


def match_scene(descinfos, neighbors, kind="l2d2", topk=10, device=0, return_scores=False):
    """Match every image of `neighbors` (img_id -> list of neighbour ids) against its neighbours in one native call.
    descinfos: img_id -> descinfo dict of the extractor (or the descriptor array itself), NumPy or torch GPU tensors.
    Returns {img_id: {ng_img_id: (n, 2) int32}} -- what ``TriangulateImage(img_id, matches)`` takes; with
    return_scores a second dict of the same shape with the FP32 score of every row."""
    kind = _kind(kind)
    neighbors = {int(i): [int(j) for j in v] for i, v in neighbors.items()}
    ids = sorted(set(neighbors) | {j for v in neighbors.values() for j in v})
    index = {i: k for k, i in enumerate(ids)}
    parts = [_rows_of(descinfos[i], kind) for i in ids]
    pair_off = np.zeros(len(ids) + 1, np.int64)
    pair_nb = []
    for k, i in enumerate(ids):
        pair_nb.extend(index[j] for j in neighbors.get(i, []))
        pair_off[k + 1] = len(pair_nb)
    row_off, rows, scores = _match_flat(parts, pair_off, pair_nb, kind, topk, device, return_scores)
    out, out_s = {}, {}
    for k, i in enumerate(ids):
        if i not in neighbors:
            continue
        out[i], out_s[i] = {}, {}
        for q in range(int(pair_off[k]), int(pair_off[k + 1])):
            j = ids[pair_nb[q]]
            out[i][j] = rows[row_off[q]:row_off[q + 1]]
            if return_scores:
                out_s[i][j] = scores[row_off[q]:row_off[q + 1]]
    return (out, out_s) if return_scores else out


def match_pair_host(desc1, desc2, kind="l2d2", topk=10, return_scores=False):
    """lt_fn_match_pair_host: the same semantics on the host (std::fmaf in a plain loop), for tests; no device"""
    kind = _kind(kind)
    L = _capi.load_library()
    a, b = _rows_of(desc1, kind), _rows_of(desc2, kind)
    if _is_torch(a):
        a = a.cpu().numpy()
    if _is_torch(b):
        b = b.cpu().numpy()
    dim = _width([a, b])
    a = np.ascontiguousarray(a.reshape(-1, dim), np.float32)
    b = np.ascontiguousarray(b.reshape(-1, dim), np.float32)
    per = 2 if kind == 1 else 1
    cap = max(1, (a.shape[0] // per) * max(1, min(max(int(topk), 1), b.shape[0] // per)))
    rows = np.zeros((cap, 2), np.int32)
    scores = np.zeros(cap, np.float32)
    n = C.c_int64(0)
    cfg = _capi.LtMatchConfig(kind, int(topk), 0, 1)
    fp = C.POINTER(C.c_float)
    rc = L.lt_fn_match_pair_host(a.ctypes.data_as(fp), a.shape[0], b.ctypes.data_as(fp), b.shape[0], dim, C.byref(cfg),
                                 _capi.ptr(rows, C.c_int32), scores.ctypes.data_as(fp), C.byref(n))
    if rc != 0:
        raise ValueError(f"lt_fn_match_pair_host: rejected (code {rc})")
    rows, scores = rows[:n.value].copy(), scores[:n.value].copy()
    return (rows, scores) if return_scores else rows


class BaseMatcherOptions(NamedTuple):
    """line2d/base_matcher.py:10-28 (n_jobs and weight_path are accepted and unused: one native call, no weights)"""
    topk: int = 10
    n_neighbors: int = 20
    n_jobs: int = 1
    weight_path: str = None


DefaultMatcherOptions = BaseMatcherOptions()


class BaseMatcher:
    """line2d/base_matcher.py:34-227 over the native matcher.  `extractor` only has to offer
    ``read_descinfo(descinfo_folder, idx)`` (and may be None where descinfos are passed directly)."""

    KIND = None

    def __init__(self, extractor=None, options=DefaultMatcherOptions, device=0):
        self.extractor = extractor
        self.topk = options.topk
        self.n_neighbors = options.n_neighbors
        self.n_jobs = options.n_jobs
        self.weight_path = options.weight_path
        self.device = 0 if device is None else device

    def get_module_name(self):
        raise NotImplementedError

    def match_pair(self, descinfo1, descinfo2):
        if self.topk == 0:
            return self.match_segs_with_descinfo(descinfo1, descinfo2)
        return self.match_segs_with_descinfo_topk(descinfo1, descinfo2, topk=self.topk)

    def _pair(self, descinfo1, descinfo2, topk):
        parts = [_rows_of(descinfo1, self.KIND), _rows_of(descinfo2, self.KIND)]
        _, rows, _ = _match_flat(parts, [0, 1, 1], [1], self.KIND, topk, self.device)
        return rows

    def match_segs_with_descinfo(self, descinfo1, descinfo2):
        raise NotImplementedError

    def match_segs_with_descinfo_topk(self, descinfo1, descinfo2, topk=10):
        if topk <= 0:
            raise ValueError("match_segs_with_descinfo_topk: topk must be positive")
        return self._pair(descinfo1, descinfo2, topk)

    def get_matches_folder(self, output_folder):
        return os.path.join(output_folder, f"{self.get_module_name()}_n{self.n_neighbors}_top{self.topk}")

    def read_descinfo(self, descinfo_folder, idx):
        return self.extractor.read_descinfo(descinfo_folder, idx)

    def get_match_filename(self, matches_folder, idx):
        return os.path.join(matches_folder, f"matches_{idx}.npy")

    def save_match(self, matches_folder, idx, matches):
        limapio.save_matches(matches_folder, idx, matches)

    def read_match(self, matches_folder, idx):
        return limapio.read_matches(matches_folder, idx)

    def match_scene(self, descinfos, neighbors):
        return match_scene(descinfos, neighbors, self.KIND, self.topk, self.device)

    def match_all_neighbors(self, output_folder, image_ids, neighbors, descinfo_folder, skip_exists=False):
        """one native call for all images that still need their file; returns the matches folder"""
        matches_folder = self.get_matches_folder(output_folder)
        if not skip_exists:
            _delete_folder(matches_folder)
        os.makedirs(matches_folder, exist_ok=True)
        todo = {int(i): [int(j) for j in neighbors[i]] for i in image_ids
                if not (skip_exists and os.path.exists(self.get_match_filename(matches_folder, i)))}
        if not todo:
            return matches_folder
        need = sorted(set(todo) | {j for v in todo.values() for j in v})
        descinfos = {i: self.read_descinfo(descinfo_folder, i) for i in need}
        for img_id, m in self.match_scene(descinfos, todo).items():
            self.save_match(matches_folder, img_id, m)
        return matches_folder

    def match_all_exhaustive_pairs(self, output_folder, image_ids, descinfo_folder, skip_exists=False):
        ids = [int(i) for i in image_ids]
        return self.match_all_neighbors(output_folder, ids, {i: [j for j in ids if j != i] for i in ids},
                                        descinfo_folder, skip_exists)


def _delete_folder(folder):
    import shutil
    if os.path.exists(folder):
        shutil.rmtree(folder)


class L2D2Matcher(BaseMatcher):
    """line2d/L2D2/matcher.py: descinfo["line_descriptors"] (M, 128)"""
    KIND = 0

    def get_module_name(self):
        return "l2d2"

    def check_compatibility(self, extractor):
        return extractor.get_module_name() == "l2d2"

    def match_segs_with_descinfo(self, descinfo1, descinfo2):
        return self._pair(descinfo1, descinfo2, 0)


class NNEndpointsMatcher(BaseMatcher):
    """line2d/endpoints/matcher.py:12-111, top-k form: descinfo["endpoints_desc"] (256, 2 M)"""
    KIND = 1

    def get_module_name(self):
        return "nn_endpoints"

    def match_segs_with_descinfo(self, descinfo1, descinfo2):
        raise NotImplementedError("NNEndpointsMatcher with topk == 0 (Sinkhorn through SuperGlue's weights) is out of scope")
