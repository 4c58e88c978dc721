"""limap_amd.features on one GPU: a record of what the patch extraction costs, nothing asserts a
time.  A warm process, one untimed pass first, then the median of ten passes with their minimum and maximum:

  kernel      k_patch_gather by HIP events, one launch per image, over N device-resident H x W x C binary16 feature maps
              and the line ranges of the supports of tests/refine_scenes.make_tracks' tracks (binary16 output left on
              the device); per image
  bytes       written: the patches, once.  requested: the four neighbour texels of every output value, as the lanes
              ask for them -- neighbouring samples share texels, so most of these are served by the caches and the rate
              is what the load path delivers, not an HBM rate.  Beside it a 16-bytes-per-lane device copy kernel over
              the same byte count (half read, half written), timed in the same process: the yardstick.  And the same
              copy over the floor: the map read once plus the patches written once
  host path   the library's host path on --threads threads, a few images, its bytes checked equal to the device's

usage: python tools/time_patch.py [--images 100] [--tracks 3000] [--height 480] [--width 640] [--channels 128]
                                  [--range-perp 16] [--threads 16] [--out profiles/patch_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(vals):
    return dict(median=float(np.median(vals)), min=float(np.min(vals)), max=float(np.max(vals)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--tracks", type=int, default=3000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--range-perp", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-images", type=int, default=3)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import refine_scenes
    from limap_amd import features
    H, W, Cc, n_img = a.height, a.width, a.channels, a.images
    opts = dict(k_stretch=1.0, t_stretch=10, range_perp=a.range_perp)

    # ---- the scene's (track, image) pairs and their ranges: one native call ----
    s = refine_scenes.make_tracks(n_tracks=a.tracks, n_views=n_img, seed=0)
    row = {int(i): k for k, i in enumerate(s["img_ids"])}
    pair_track, pair_img = [], []
    for t in range(a.tracks):
        for i in sorted(set(int(x) for x in s["img"][s["off"][t]:s["off"][t + 1]])):
            pair_track.append(t)
            pair_img.append(i)
    rows = [row[i] for i in pair_img]
    cam11 = np.concatenate([s["k"][rows], s["q"][rows], s["t"][rows]], 1)
    t0 = time.perf_counter()
    ranges, status = features.ranges_from_arrays(s["line6"], s["off"], s["img"], s["l2d"], pair_track, pair_img, cam11)
    ranges_ms = 1e3 * (time.perf_counter() - t0)
    keep = status == 0
    # the scene's cameras see 2 cx x 2 cy pixels (800 x 600); the ranges are brought to the map's size
    scale = W / (2.0 * float(s["k"][0][2]))
    ranges = ranges * scale
    by_image = {int(i): ranges[keep & (np.array(pair_img) == int(i))] for i in s["img_ids"]}

    # ---- the kernel on device-resident maps ----
    gen = torch.Generator(device="cuda").manual_seed(0)
    maps = {i: torch.randn((H, W, Cc), generator=gen, device="cuda", dtype=torch.float32).to(torch.float16) for i in by_image}
    ext = features.get_line_patch_extractor(opts, Cc)
    info = {}

    def one_pass():
        ms, written, rows_total, forms = [], 0, 0, set()
        for i, lines in by_image.items():
            out = ext.ExtractLinePatches(lines, maps[i], dtype="float16", device_out=True)
            t = features.timers()
            ms.append(t["kernel_ms"])
            written += int(t["out_bytes"])
            rows_total += sum(int(p.array.shape[0]) for p in out)
            forms.add(t["vector_form"])
        info.update(written=written, rows=rows_total, forms=sorted(forms))
        return float(np.mean(ms))

    one_pass()  # untimed
    per_image = [one_pass() for _ in range(a.passes)]
    n_patches = int(keep.sum())
    written = info["written"] / n_img        # bytes per image
    requested = 4 * written                  # input and output are both binary16: four neighbours per output value
    moved = written + requested
    ctx = features._context(0)

    def copy_ms(nbytes=moved):
        ms = C.c_double(0.0)
        ctx.chk(ctx.L.lt_patch_copy_yardstick(ctx.h, int(nbytes) // 2, C.byref(ms)))  # reads half, writes half
        return ms.value

    copy_ms()
    copy = [copy_ms() for _ in range(a.passes)]
    # the floor: what has to cross the memory interface at least once -- the map read once, the patches written once
    floor_bytes = written + H * W * Cc * 2
    copy_ms(floor_bytes)
    floor = [copy_ms(floor_bytes) for _ in range(a.passes)]

    # ---- the host path, a few images ----
    host = []
    for i in list(by_image)[:a.host_images]:
        f = maps[i].cpu().numpy()
        t0 = time.perf_counter()
        ref = ext.ExtractLinePatches(by_image[i], f, host=True, dtype="float16", n_threads=a.threads)
        host.append(1e3 * (time.perf_counter() - t0))
        dev = ext.ExtractLinePatches(by_image[i], maps[i], dtype="float16")
        assert all(np.array_equal(x.array.view(np.uint16), y.array.view(np.uint16)) for x, y in zip(ref, dev)), \
            "host and device disagree"

    k_med = float(np.median(per_image))
    out = dict(images=n_img, tracks=a.tracks, map=[H, W, Cc], map_dtype="float16", out_dtype="float16", options=opts,
               ranges_scaled_by=scale, pairs=len(pair_track), pairs_refused=int((~keep).sum()), patches=n_patches,
               patches_per_image=n_patches / n_img, mean_patch_rows=info["rows"] / max(n_patches, 1),
               vector_form=info["forms"], ranges_native_call_ms=ranges_ms,
               per_image=dict(k_patch_gather_ms=stats(per_image), bytes_written=written, bytes_requested=requested,
                              map_bytes=H * W * Cc * 2, gb_per_s=moved / k_med / 1e6,
                              copy16_ms=stats(copy), copy16_gb_per_s=moved / float(np.median(copy)) / 1e6,
                              fraction_of_copy=float(np.median(copy)) / k_med,
                              floor_bytes=floor_bytes, floor_copy16_ms=stats(floor),
                              floor_gb_per_s=floor_bytes / k_med / 1e6),
               host_path=dict(threads=a.threads, images=len(host), per_image_ms=stats(host) if host else None),
               not_measured=["the map's upload from host memory", "the download of the patches", "file writing",
                             "float32 and float64 maps", "the scalar form", "HBM traffic (no counters were read)"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(out, fo, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
