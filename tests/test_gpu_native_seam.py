"""The device rule of limap_amd._native at every entry point that reads a GPU tensor in place: a tensor on cuda:0 handed
to a call for device 1 is refused with the seam's wording, before the module asks for its context -- on a machine with
one GPU a context for device 1 cannot be created (RuntimeError), so the ValueError shows the rule ran first.  No kernel
runs here; the two entry points of `fitting` are in test_gpu_fit_depth.py and test_gpu_fit_scan.py."""
import numpy as np
import pytest
import torch

from limap_amd import features, line2d, matching, undistortion

pytestmark = pytest.mark.gpu


def _refused(who, what):
    return pytest.raises(ValueError, match=f"^{who}: {what} lives on cuda:0, the call runs on cuda:1$")


def _on0(shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda:0")


def test_features_extraction_from_a_tensor_map():
    ext = features.get_line_patch_extractor({"k_stretch": 1.0, "t_stretch": 1, "range_perp": 2}, 3)
    with _refused("features", "the tensor"):
        ext.ExtractLinePatches(np.array([[1.0, 1.0, 5.0, 5.0]]), _on0((8, 8, 3)), device=1)


def test_undistortion_warp():
    cam = undistortion.Camera("SIMPLE_RADIAL", [6.0, 4.0, 4.0, 0.05], cam_id=0, hw=(8, 8))
    target = undistortion.Camera("PINHOLE", [6.0, 6.0, 4.0, 4.0], cam_id=0, hw=(8, 8))
    img = _on0((8, 8, 3), torch.uint8)
    with _refused("undistortion", "the tensor"):
        undistortion._warp_batch([(cam, target, img)], device=1)
    with _refused("undistortion", "the tensor"):  # before the border scan of the camera asks for the context
        undistortion.undistort_images({0: cam}, {0: img}, device=1)


def test_line2d_detect_scene_and_descriptor_info():
    junctions = np.array([[1.0, 1.0], [6.0, 6.0]], np.float32)
    with _refused("line2d", "the heatmap"):
        line2d.detect_scene(line2d.SHIPPED_CFG, [junctions], [_on0((8, 8))], device=1)
    segs = np.array([[[1.0, 1.0], [6.0, 6.0]], [[1.0, 6.0], [6.0, 1.0]]])
    with _refused("line2d", "the descriptor"):
        line2d.compute_descinfo_scene([segs], [_on0((1, 4, 2, 2))], device=1)


def test_matching_with_descriptor_tensors_and_with_dense_warps():
    desc = {0: _on0((3, 8)), 1: _on0((3, 8))}
    with _refused("matching", "a descriptor array"):
        matching.match_scene(desc, {0: [1]}, kind="l2d2", topk=1, device=1)
    sold2 = {i: [_on0((8, 3)), np.ones((3, 1), bool)] for i in (0, 1)}
    with _refused("matching", "a descriptor array"):
        matching.match_scene(sold2, {0: [1]}, kind="sold2", topk=1, device=1, num_samples=1)
    lines = np.array([[[1.0, 1.0], [6.0, 6.0]], [[1.0, 6.0], [6.0, 1.0]]])
    dense = {i: {"lines": lines, "image_shape": (8, 8)} for i in (0, 1)}
    warps = (_on0((8, 8, 2)), _on0((8, 8)), _on0((8, 8, 2)), _on0((8, 8)))
    with _refused("matching", "a warp"):
        matching.match_scene_dense(dense, {0: [1]}, lambda i, j: warps, sample_thresh=0.5, device=1)
