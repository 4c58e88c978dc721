"""SOLD2 line detection from junctions and line heatmaps on the GPU -- the classical step between the SOLD2 network and
what consumes its lines (``LineSegmentDetectionModule`` of line2d/SOLD2/model/line_detection.py; names follow it):

    from limap_amd import line2d
    module = line2d.LineSegmentDetectionModule(**line2d.SHIPPED_CFG)          # config/export_line_features.yaml
    line_map, junctions, heatmap = module.detect(junctions, heatmap)           # one image
    segs = line2d.detect_scene(module, junctions_list, heatmaps)               # a scene: one native call
    descinfo = line2d.compute_descinfo(segs[0], descriptor)                    # what matching.SOLD2Matcher takes

Heatmap refinement, candidate suppression, sampling of all junction pairs, the inlier test and junction refinement run
for every image of a scene in one launch of each kernel (which is also the definition);
``host=True`` computes the same result, bit for bit, by the library's host path.  The tail -- unique refined
endpoints, the line map, the segment list -- is NumPy.  Not built: the network itself (backbone,
``convert_junc_predictions``, ``super_nms``), the saliency column of ``SOLD2LineDetector.detect`` and the multiscale
path; ``compute_descinfo`` builds the ``"regular"`` sampling mode only.
"""
import ctypes as C

import numpy as np

from . import _capi, _native

__all__ = ["LineSegmentDetectionModule", "detect_scene", "line_map_to_segments", "sold2segstosegs", "segstosold2segs",
           "compute_descinfo", "compute_descinfo_scene", "sample_line_points", "kernel_ms", "SHIPPED_CFG"]

_context = _capi.per_device_contexts()
KERNEL_MS_KEYS = ["block_scale", "refine_pixels", "suppress", "score", "compact", "refine_junctions", "kernels", "call"]

# line_detector_cfg of line2d/SOLD2/config/export_line_features.yaml: every option on
SHIPPED_CFG = {
    "detect_thresh": 0.5, "num_samples": 64, "sampling_method": "local_max", "inlier_thresh": 0.99,
    "use_candidate_suppression": True, "nms_dist_tolerance": 3.0, "use_heatmap_refinement": True,
    "heatmap_refine_cfg": {"mode": "local", "ratio": 0.2, "valid_thresh": 0.001, "num_blocks": 20, "overlap_ratio": 0.5},
    "use_junction_refinement": True, "junction_refine_cfg": {"num_perturbs": 9, "perturb_interval": 0.25},
}


def linspace_sampler(n):
    """torch.linspace(0, 1, n) as float32: the sampler of the reference, which no closed form reproduces in FP32"""
    import torch
    return torch.linspace(0, 1, int(n)).numpy().astype(np.float32)


def _perturb_vec(num_perturbs, interval):
    """the reference's torch.arange of the perturbations, float32"""
    import torch
    side = (num_perturbs - 1) // 2
    vec = torch.arange(start=-interval * side, end=interval * (side + 1), step=interval)
    return vec.to(torch.float32).numpy()


class LineSegmentDetectionModule:
    """Module extracting line segments from junctions and line heatmaps (arguments and defaults of the reference)."""

    def __init__(self, detect_thresh, num_samples=64, sampling_method="local_max", inlier_thresh=0.0,
                 heatmap_low_thresh=0.15, heatmap_high_thresh=0.2, max_local_patch_radius=3, lambda_radius=2.0,
                 use_candidate_suppression=False, nms_dist_tolerance=3.0, use_heatmap_refinement=False,
                 heatmap_refine_cfg=None, use_junction_refinement=False, junction_refine_cfg=None, device=0):
        self.detect_thresh = detect_thresh
        self.num_samples = num_samples
        self.sampling_method = sampling_method
        self.inlier_thresh = inlier_thresh
        self.local_patch_radius = max_local_patch_radius
        self.lambda_radius = lambda_radius
        self.low_thresh = heatmap_low_thresh
        self.high_thresh = heatmap_high_thresh
        self.use_candidate_suppression = use_candidate_suppression
        self.nms_dist_tolerance = nms_dist_tolerance
        self.use_heatmap_refinement = use_heatmap_refinement
        self.heatmap_refine_cfg = heatmap_refine_cfg
        if self.use_heatmap_refinement and self.heatmap_refine_cfg is None:
            raise ValueError("[Error] Missing heatmap refinement config.")
        self.use_junction_refinement = use_junction_refinement
        self.junction_refine_cfg = junction_refine_cfg
        if self.use_junction_refinement and self.junction_refine_cfg is None:
            raise ValueError("[Error] Missing junction refinement config.")
        self.device = device
        # largest heatmap window the junction refinement stages in LDS, in floats (None: the library's default)
        self.lds_window_floats = None
        self._validate()
        self.sampler = np.linspace(0, 1, self.num_samples)
        self.torch_sampler = linspace_sampler(self.num_samples)

    def _validate(self):
        n = self.num_samples
        if int(n) != n or n < 2 or n > 64:
            raise ValueError(f"line2d: num_samples outside 2 .. 64: {n}")
        if self.sampling_method not in ("local_max", "bilinear"):
            raise ValueError(f"line2d: sampling_method is unknown: {self.sampling_method!r}")
        r = self.local_patch_radius
        if int(r) != r or r < 0 or r > 4:
            raise ValueError(f"line2d: max_local_patch_radius outside 0 .. 4: {r}")
        if self.use_heatmap_refinement:
            mode = self.heatmap_refine_cfg.get("mode")
            if mode not in ("global", "local"):
                raise ValueError(f"line2d: mode of heatmap_refine_cfg is unknown: {mode!r}")
        if self.use_junction_refinement:
            p = self.junction_refine_cfg["num_perturbs"]
            if int(p) != p or p < 1 or p > 9 or p % 2 == 0:
                raise ValueError(f"line2d: num_perturbs must be odd and at most 9: {p}")

    def _config(self):
        """-> (lt_sold2_config, the arrays it points into)"""
        self._validate()
        c = _capi.LtSold2Config()
        c.detect_thresh, c.inlier_thresh = float(self.detect_thresh), float(self.inlier_thresh)
        c.lambda_radius, c.nms_dist_tolerance = float(self.lambda_radius), float(self.nms_dist_tolerance)
        c.num_samples = int(self.num_samples)
        c.sampling_method = 0 if self.sampling_method == "local_max" else 1
        c.max_local_patch_radius = int(self.local_patch_radius)
        c.use_candidate_suppression = int(bool(self.use_candidate_suppression))
        c.use_heatmap_refinement = int(bool(self.use_heatmap_refinement))
        c.use_junction_refinement = int(bool(self.use_junction_refinement))
        c.lds_window_floats = -1 if self.lds_window_floats is None else int(self.lds_window_floats)
        c.refine_ratio, c.refine_valid_thresh, c.refine_overlap_ratio, c.refine_num_blocks = 0.2, 1e-2, 0.5, 1
        if self.use_heatmap_refinement:
            h = self.heatmap_refine_cfg
            c.refine_mode = 0 if h["mode"] == "global" else 1
            c.refine_ratio, c.refine_valid_thresh = float(h["ratio"]), float(h["valid_thresh"])
            if c.refine_mode == 1:
                c.refine_num_blocks, c.refine_overlap_ratio = int(h["num_blocks"]), float(h["overlap_ratio"])
        sampler = np.ascontiguousarray(linspace_sampler(self.num_samples))
        keep = [sampler]
        c.sampler = sampler.ctypes.data
        c.num_perturbs = 1
        if self.use_junction_refinement:
            j = self.junction_refine_cfg
            vec = np.ascontiguousarray(_perturb_vec(int(j["num_perturbs"]), j["perturb_interval"]))
            if vec.size != int(j["num_perturbs"]):
                raise ValueError(f"line2d: perturb_interval {j['perturb_interval']!r} gives {vec.size} perturbations "
                                 f"for num_perturbs {j['num_perturbs']}")
            c.num_perturbs = int(j["num_perturbs"])
            c.perturb_vec = vec.ctypes.data
            keep.append(vec)
        return c, keep

    def detect(self, junctions, heatmap, device=None, host=False):
        """-> (line_map, junctions, heatmap) as the reference returns them: the line map (int32 without junction
        refinement, float32 with it), the junctions (refined: the unique refined endpoints) and the heatmap the stages
        read (refined where refinement is on).  Torch inputs give torch outputs on the heatmap's device."""
        dev = self.device if device is None else device
        res = detect_scene(self, [junctions], [heatmap], device=dev, host=host, return_stages=True)
        st = res[1][0]
        if self.use_junction_refinement:
            line_map, junc = st["line_map_refined"], st["junctions_refined"]
        else:
            line_map, junc = st["line_map"], np.asarray(_native.to_host(junctions), np.float32).reshape(-1, 2)
        out = (line_map, junc, st["heatmap"])
        if _native.is_torch(heatmap):
            import torch
            out = tuple(torch.from_numpy(np.ascontiguousarray(o)).to(heatmap.device) for o in out)
        return out


def _as_module(module_or_cfg):
    if isinstance(module_or_cfg, LineSegmentDetectionModule):
        return module_or_cfg
    return LineSegmentDetectionModule(**dict(module_or_cfg))


def _prepare_image(junctions, heatmap, host, device):
    """-> the Operands (junctions (n, 2), heatmap) of one image, both FP32, contiguous and in one place: the heatmap's,
    to which the junctions are brought"""
    jshape, hshape = tuple(junctions.shape), tuple(heatmap.shape)
    empty = len(jshape) in (1, 2) and jshape[0] == 0  # np.zeros(0) and np.zeros((0, 2)) both mean "no junction"
    if not empty and (len(jshape) != 2 or jshape[1] != 2):
        raise ValueError(f"line2d: junctions must be (n, 2), got shape {jshape}")
    if len(hshape) != 2:
        raise ValueError(f"line2d: a heatmap must be 2-D (H, W), got shape {hshape}")
    hm = _native.operand(heatmap, host=host, device=device, who="line2d", what="the heatmap")
    hm = hm.astype("float32").contiguous()
    if hm.on_device:
        import torch
        jn = junctions if _native.is_torch(junctions) else torch.as_tensor(np.asarray(junctions))
        jn = jn.to(device=hm.keep.device, dtype=torch.float32).reshape(-1, 2).contiguous()
    else:
        jn = np.ascontiguousarray(_native.to_host(junctions), np.float32).reshape(-1, 2)
    return _native.Operand(jn, hm.on_device), hm


def unique_rows(points):
    """torch.unique(points, dim=0): the distinct rows in lexicographic order"""
    points = np.asarray(points, np.float32).reshape(-1, 2)
    if points.shape[0] == 0:
        return points
    return np.unique(points, axis=0)


def segments_to_line_map(junctions, segments):
    """the reference's segments_to_line_map: float32 (n, n), 1 where a segment joins two junctions"""
    n = junctions.shape[0]
    line_map = np.zeros((n, n), np.float32)
    for seg in segments:
        a = np.nonzero((junctions == seg[0]).sum(axis=1) == 2)[0]
        b = np.nonzero((junctions == seg[1]).sum(axis=1) == 2)[0]
        line_map[np.ix_(a, b)] = 1
        line_map[np.ix_(b, a)] = 1
    return line_map


def line_map_to_segments(junctions, line_map):
    """line_detector.py:line_map_to_segments: (N, 2, 2) float64 segments in the reference's emission order.  A segment
    refined to a single point sits on the diagonal of the line map and is emitted as the reference emits it."""
    junctions = _native.to_host(junctions)
    tmp = np.array(_native.to_host(line_map), copy=True)
    out = []
    for idx in range(junctions.shape[0]):
        if tmp[idx, :].sum() == 0:
            continue
        for idx2 in np.where(tmp[idx, :] == 1)[0]:
            out.append(np.stack([junctions[idx, :], junctions[idx2, :]]))
            tmp[idx, idx2] = 0
            tmp[idx2, idx] = 0
    if not out:
        return np.zeros([0, 2, 2])
    return np.stack(out).astype(np.float64)


def sold2segstosegs(segs_sold2):
    """sold2_wrapper.py: (N, 2, 2) in (h, w) order -> (N, 4) x1, y1, x2, y2"""
    segs_sold2 = np.asarray(segs_sold2)
    return np.flip(segs_sold2, axis=2).reshape(len(segs_sold2), 4)


def segstosold2segs(segs):
    """sold2_wrapper.py: (N, 4) x1, y1, x2, y2 -> (N, 2, 2) in (h, w) order"""
    segs = np.asarray(segs)
    return np.flip(segs.reshape(segs.shape[0], 2, 2), axis=2)


def detect_scene(module_or_cfg, junctions_list, heatmaps, device=0, host=False, return_stages=False, cand_in=None,
                 det_in=None, n_threads=0):
    """Every image of a scene in one native call; junction counts and heatmap sizes may differ between the images.
    -> the list of segments, (N, 2, 2) float64 in SOLD2's (h, w) order, one per image.  With return_stages also a list
    of dicts: ``heatmap`` (the refined heatmap), ``candidates`` (n, n) uint8 after suppression, ``line_map`` (n, n)
    int32 before junction refinement, ``pairs`` (N, 2), ``segments_refined`` (N, 2, 2) float32 and ``perturb`` (N,) the
    index of the chosen perturbation of every detected segment, ``junctions_refined`` / ``line_map_refined`` the
    tail's result.  cand_in / det_in (host form only): per image an (n, n) mask that stands in for the result of the
    suppression / of the detection, or None."""
    module = _as_module(module_or_cfg)
    if len(junctions_list) != len(heatmaps):
        raise ValueError("line2d: one heatmap per junction array")
    n_img = len(heatmaps)
    cfg, keep = module._config()
    # (a list: every heatmap meets the device rule, whatever the others are)
    use_device = n_img > 0 and all([_native.check_device(h, host=host, device=device, who="line2d", what="the heatmap")
                                    for h in heatmaps])
    arr = (_capi.LtSold2Image * max(n_img, 1))()
    recs = []
    for k in range(n_img):
        jn, hm = _prepare_image(junctions_list[k], heatmaps[k], not use_device, device)
        recs.append((jn, hm))
        a = arr[k]
        a.junctions, a.heatmap, a.heat_stride, a.n_junc = jn.address, hm.address, hm.shape[1], jn.shape[0]
        a.H, a.W, a.on_device = *hm.shape, hm.on_device
        for name, masks in (("cand_in", cand_in), ("det_in", det_in)):
            if masks is not None and masks[k] is not None:
                m = np.ascontiguousarray(_native.to_host(masks[k]) != 0, np.uint8)
                if m.shape != (jn.shape[0], jn.shape[0]):
                    raise ValueError(f"line2d: {name} must be (n, n)")
                keep.append(m)
                setattr(a, name, m.ctypes.data)
    if host:
        L, h = _capi.load_library(), None

        def chk(rc):
            if rc != 0:
                _native.raise_host_error(L, "lt_fn_sold2_host_error")
        chk(L.lt_fn_sold2_detect_host(C.byref(cfg), n_img, arr, int(n_threads)))
    else:
        ctx = _context(device)
        L, h, chk = ctx.L, ctx.h, ctx.chk
        if use_device:
            _native.wait_for_torch(device)
        chk(L.lt_sold2_detect_scene(h, C.byref(cfg), n_img, arr))
    counts = np.zeros(max(n_img, 1), np.int64)
    chk(L.lt_sold2_get_counts(h, _capi.ptr(counts, C.c_int64)))
    segments, stages = [], []
    refine = bool(module.use_junction_refinement)
    for k in range(n_img):
        jn, hm = recs[k]
        n, N = jn.shape[0], int(counts[k])
        segs = np.zeros((max(N, 1), 2, 2), np.float32)
        pairs = np.zeros((max(N, 1), 2), np.int32)
        perturb = np.zeros(max(N, 1), np.int32)
        chk(L.lt_sold2_get_segments(h, k, _capi.ptr(segs, C.c_float), _capi.ptr(pairs, C.c_int32),
                                    _capi.ptr(perturb, C.c_int32)))
        segs, pairs, perturb = segs[:N], pairs[:N], perturb[:N]
        if refine:
            junc_new = unique_rows(segs.reshape(-1, 2))
            line_map_new = segments_to_line_map(junc_new, segs)
            out = line_map_to_segments(junc_new, line_map_new)
        else:
            # the line map of the detections emits its segments in candidate order already
            junc_new, line_map_new, out = None, None, segs.astype(np.float64)
        segments.append(out)
        if return_stages:
            heat = np.zeros(hm.shape, np.float32)
            cand, det = np.zeros((max(n, 1), max(n, 1)), np.uint8), np.zeros((max(n, 1), max(n, 1)), np.uint8)
            chk(L.lt_sold2_get_stages(h, k, _capi.ptr(heat, C.c_float), _capi.ptr(cand, C.c_uint8),
                                      _capi.ptr(det, C.c_uint8)))
            cand, det = cand[:n, :n] if n else np.zeros((0, 0), np.uint8), det[:n, :n] if n else np.zeros((0, 0), np.uint8)
            stages.append({"heatmap": heat, "candidates": cand, "line_map": (det | det.T).astype(np.int32),
                           "pairs": pairs, "segments_refined": segs, "perturb": perturb,
                           "junctions_refined": junc_new, "line_map_refined": line_map_new})
    return (segments, stages) if return_stages else segments


def _one_image(module, junctions, heatmap):
    cfg, keep = module._config()
    jn, hm = _prepare_image(junctions, heatmap, True, 0)
    img = _capi.LtSold2Image()
    img.junctions, img.heatmap, img.heat_stride = jn.address, hm.address, hm.shape[1]
    img.n_junc, img.H, img.W = jn.shape[0], hm.shape[0], hm.shape[1]
    return cfg, img, keep + [jn, hm]


def samples_host(module_or_cfg, junctions, heatmap, pairs):
    """the host path's samples of the given junction pairs on the heatmap as it is given: -> (positions (P, S, 2) in
    (h, w), values (P, S)) by the module's sampling method"""
    module = _as_module(module_or_cfg)
    cfg, img, keep = _one_image(module, junctions, heatmap)
    pairs = _capi.i32(pairs).reshape(-1, 2)
    P, S = pairs.shape[0], int(module.num_samples)
    pos, val = np.zeros((max(P, 1), S, 2), np.float32), np.zeros((max(P, 1), S), np.float32)
    L = _capi.load_library()
    if L.lt_fn_sold2_samples_host(C.byref(cfg), C.byref(img), P, _capi.ptr(pairs, C.c_int32), _capi.ptr(pos, C.c_float),
                                  _capi.ptr(val, C.c_float)) != 0:
        _native.raise_host_error(L, "lt_fn_sold2_host_error")
    return pos[:P], val[:P]


def block_scales_host(module_or_cfg, heatmap):
    """the host path's heatmap-refinement blocks: -> (scales (nb, nb), negative where a block is not above
    valid_thresh; bounds (nb, 4): row begin, row end, column begin, column end of block index a)"""
    module = _as_module(module_or_cfg)
    cfg, img, keep = _one_image(module, np.zeros((0, 2), np.float32), heatmap)
    nb = 1 if cfg.refine_mode == 0 else int(cfg.refine_num_blocks)
    nb = max(1, min(nb, 32))
    scales, bounds = np.zeros((nb, nb), np.float32), np.zeros((nb, 4), np.int32)
    L = _capi.load_library()
    if L.lt_fn_sold2_block_scales_host(C.byref(cfg), C.byref(img), _capi.ptr(scales, C.c_float),
                                       _capi.ptr(bounds, C.c_int32)) != 0:
        _native.raise_host_error(L, "lt_fn_sold2_host_error")
    return scales, bounds


def kernel_ms(device=0):
    """lt_sold2_get_kernel_ms of the last device detection: device ms per kernel, all kernels, the whole call"""
    return dict(zip(KERNEL_MS_KEYS, _context(device).module_timers("lt_sold2_get_kernel_ms", 8).tolist()))


# ---- compute_descriptors of WunschLineMatcher ----
def sample_line_points(line_seg, num_samples=5, min_dist_pts=8):
    """line_matching.py:sample_line_points: 2 .. num_samples points at least min_dist_pts apart along every segment,
    padded with zeros -> (points (N, num_samples, 2) float64, valid (N, num_samples) bool)"""
    line_seg = np.asarray(_native.to_host(line_seg), np.float64).reshape(-1, 2, 2)
    num_lines = len(line_seg)
    line_lengths = np.linalg.norm(line_seg[:, 0] - line_seg[:, 1], axis=1)
    num_samples_lst = np.clip(line_lengths // min_dist_pts, 2, num_samples)
    line_points = np.zeros((num_lines, num_samples, 2), dtype=float)
    valid_points = np.zeros((num_lines, num_samples), dtype=bool)
    for n in np.arange(2, num_samples + 1):
        cur_mask = num_samples_lst == n
        cur = line_seg[cur_mask]
        px = np.linspace(cur[:, 0, 0], cur[:, 1, 0], n, axis=-1)
        py = np.linspace(cur[:, 0, 1], cur[:, 1, 1], n, axis=-1)
        pts = np.zeros((len(cur), num_samples, 2))
        pts[:, :n] = np.stack([px, py], axis=-1)
        line_points[cur_mask] = pts
        valid = np.zeros((len(cur), num_samples), bool)
        valid[:, :n] = True
        valid_points[cur_mask] = valid
    return line_points, valid_points


def compute_descinfo_scene(segs_list, descriptors, num_samples=5, min_dist_pts=8, grid_size=4, sampling_mode="regular",
                           device=0, host=False, n_threads=0):
    """compute_descriptors for every image of a scene in one native call: segs (N, 2, 2) in (h, w) order and the
    descriptor map (1, C, H / grid_size, W / grid_size) per image -> [desc (C, num_samples N) float32, valid (N,
    num_samples) bool] per image (NumPy; desc is a torch tensor on the map's device where the map is a GPU tensor).
    An image without segments gives the reference's ``np.empty((0), dtype=int)``."""
    if sampling_mode != "regular":
        raise NotImplementedError(f"line2d: sampling mode {sampling_mode!r} is not built (regular only)")
    if len(segs_list) != len(descriptors):
        raise ValueError("line2d: one descriptor map per segment array")
    if num_samples < 2 or num_samples > 64:
        raise ValueError(f"line2d: num_samples outside 2 .. 64: {num_samples}")
    n_img = len(segs_list)
    arr = (_capi.LtSold2DescImage * max(n_img, 1))()
    keep, outs, valids, rows = [], [], [], []
    for k in range(n_img):
        segs, desc = segs_list[k], descriptors[k]
        if tuple(desc.shape)[:1] != (1,) or len(desc.shape) != 4:
            raise ValueError(f"line2d: a descriptor map must be (1, C, H, W), got shape {tuple(desc.shape)}")
        if len(segs) == 0:
            outs.append(None)
            valids.append(None)
            continue
        pts, valid = sample_line_points(segs, num_samples, min_dist_pts)
        pts = np.ascontiguousarray(pts.reshape(-1, 2), np.float32)
        _, ch, hd, wd = (int(v) for v in desc.shape)
        cl = _native.operand(desc, host=host, device=device, who="line2d", what="the descriptor").astype("float32")
        cl = cl.map(lambda d: d[0].swapaxes(0, 1).swapaxes(1, 2)).contiguous()  # (C, H, W) -> (H, W, C)
        if cl.on_device:
            import torch
            out = torch.empty((ch, pts.shape[0]), dtype=torch.float32, device=desc.device)
        else:
            out = np.zeros((ch, pts.shape[0]), np.float32)
        keep += [pts, cl]
        a = arr[len(rows)]
        a.map, a.points, a.out, a.n_points = cl.address, pts.ctypes.data, _native.address(out), pts.shape[0]
        a.Hd, a.Wd, a.C, a.grid_size, a.on_device = hd, wd, ch, int(grid_size), cl.on_device
        rows.append(k)
        outs.append(out)
        valids.append(valid)
    if host:
        L = _capi.load_library()
        if L.lt_fn_sold2_descinfo_host(len(rows), arr, int(n_threads)) != 0:
            _native.raise_host_error(L, "lt_fn_sold2_host_error")
    else:
        ctx = _context(device)
        if any(arr[j].on_device for j in range(len(rows))):
            _native.wait_for_torch(device)
        ms = C.c_double(0.0)
        ctx.chk(ctx.L.lt_sold2_descinfo_scene(ctx.h, len(rows), arr, C.byref(ms)))
        compute_descinfo_scene.last_ms = ms.value
    return [np.empty((0), dtype=int) if o is None else [o, v] for o, v in zip(outs, valids)]


def compute_descinfo(segs, descriptor, num_samples=5, min_dist_pts=8, grid_size=4, sampling_mode="regular", device=0,
                     host=False):
    """WunschLineMatcher.compute_descriptors for one image -> [desc (C, num_samples N), valid (N, num_samples)]"""
    return compute_descinfo_scene([segs], [descriptor], num_samples, min_dist_pts, grid_size, sampling_mode, device,
                                  host)[0]
