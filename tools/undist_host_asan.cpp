// undist_host_asan.cpp -- the host path of limap_amd.undistortion (lt_fn_undist_warp_host, lt_fn_undist_points_host,
// lt_fn_undist_scale of lt_undist_host.cpp) under AddressSanitizer and UBSan, as a program of its own:
// lt_undist_host.cpp, the host-only unit, is compiled into it with the sanitizers; nothing is loaded into Python and no
// device is touched.  `make -C limap_amd/csrc undist_asan` builds and runs it (tests/test_undist_host.py does that).
// The cases are the degenerate ones of the tests: 1x1 and one-pixel-wide images, every channel count, a row stride
// larger than a row, the exact-coordinate case whose last row and column are black, coefficients that overflow to
// infinity and NaN, a target larger and one smaller than its source, no points, the singular Jacobian, the 100
// iterations, and every refusal.  Buffers are exactly as large as the sizes say: an overrun of one byte is the
// sanitizer's to find.
#include "host_asan.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

lt_undist_camera cam(int model, std::vector<double> p) {
  lt_undist_camera c;
  std::memset(&c, 0, sizeof(c));
  c.model = model;
  c.n_params = (int32_t)p.size();
  for (size_t k = 0; k < p.size() && k < 12; ++k) c.params[k] = p[k];
  return c;
}

struct Warp {
  int rc;
  std::vector<unsigned char> out;
};

// warps a sw x sh image of `ch` channels whose rows lie `pad` bytes further apart than they are long
Warp warp(const lt_undist_camera &src, const lt_undist_camera &dst, int sw, int sh, int tw, int th, int ch, int pad,
          int threads, unsigned char fill = 0) {
  const lt_undist_camera cams[2] = {src, dst};
  std::vector<unsigned char> in((size_t)sh * (size_t)(sw * ch + pad) - (size_t)pad);
  for (size_t k = 0; k < in.size(); ++k) in[k] = fill ? fill : (unsigned char)(37 * k + 11);
  Warp w;
  w.out.assign((size_t)th * (size_t)(tw * ch + pad) - (size_t)pad, 0xab);
  lt_undist_image im;
  std::memset(&im, 0, sizeof(im));
  im.src = in.data();
  im.dst = w.out.data();
  im.src_stride = sw * ch + pad;
  im.dst_stride = tw * ch + pad;
  im.src_w = sw; im.src_h = sh; im.dst_w = tw; im.dst_h = th;
  im.channels = ch;
  im.src_cam = 0;
  im.dst_cam = 1;
  w.rc = lt_fn_undist_warp_host(2, cams, 1, &im, threads);
  return w;
}

struct Pts {
  int rc;
  std::vector<double> out;
  std::vector<int32_t> status, iters;
};

Pts points(const lt_undist_camera &src, const lt_undist_camera &dst, const std::vector<double> &xy, int threads) {
  const lt_undist_camera cams[2] = {src, dst};
  const int64_t n = (int64_t)xy.size() / 2;
  std::vector<int32_t> a((size_t)n, 0), b((size_t)n, 1);
  Pts p;
  p.out.resize((size_t)(2 * n));
  p.status.resize((size_t)n);
  p.iters.resize((size_t)n);
  p.rc = lt_fn_undist_points_host(2, cams, n, xy.data(), a.data(), b.data(), p.out.data(), p.status.data(),
                                  p.iters.data(), threads);
  return p;
}

bool has(const char *what) { return host_asan::has(lt_fn_undist_host_error, what); }

}  // namespace

int main() {
  const lt_undist_camera pin = cam(1, {64.0, 64.0, 4.5, 3.25});
  const lt_undist_camera quirk = cam(2, {64.0, 4.5, 3.25, 0.0});
  for (int threads : {1, 4}) {
    // the exact-coordinate case: the source, its last row and column black
    for (int ch : {1, 3, 4})
      for (int pad : {0, 5}) {
        const int w = 9, h = 6;
        Warp r = warp(quirk, pin, w, h, w, h, ch, pad, threads);
        EXPECT(r.rc == 0);
        bool ok = true;
        for (int y = 0; y < h && r.rc == 0; ++y)
          for (int x = 0; x < w; ++x)
            for (int c = 0; c < ch; ++c) {
              const size_t k = (size_t)y * (size_t)(w * ch + pad) + (size_t)(x * ch + c);
              const unsigned char want = (x == w - 1 || y == h - 1) ? 0 : (unsigned char)(37 * k + 11);
              ok = ok && r.out[k] == want;
            }
        EXPECT(ok);
      }
    // one pixel, one column, one row: no pixel has four neighbours, everything is black
    for (int wh : {0, 1, 2}) {
      const int w = wh == 1 ? 1 : (wh == 2 ? 7 : 1), h = wh == 1 ? 7 : 1;
      Warp r = warp(quirk, pin, w, h, w, h, 3, 0, threads, 255);
      EXPECT(r.rc == 0);
      bool black = true;
      for (unsigned char b : r.out) black = black && b == 0;
      EXPECT(black);
    }
    // a target larger and a target smaller than its source
    EXPECT(warp(cam(2, {20.0, 4.5, 3.25, -0.3}), pin, 9, 6, 18, 12, 3, 0, threads).rc == 0);
    EXPECT(warp(cam(2, {20.0, 4.5, 3.25, 0.3}), pin, 9, 6, 2, 1, 4, 3, threads).rc == 0);
    // overflow: infinite and NaN source coordinates are black
    {
      Warp r = warp(cam(3, {64.0, 4.5, 3.25, 1e308, 1e308}), pin, 9, 6, 9, 6, 3, 0, threads, 255);
      EXPECT(r.rc == 0);
      bool black = true;
      for (unsigned char b : r.out) black = black && b == 0;
      EXPECT(black);
    }
    // points: none, the principal point, the singular Jacobian, the 100 iterations, a pinhole source
    const lt_undist_camera fold = cam(2, {64.0, 32.0, 16.0, -1.0}), flat = cam(1, {64.0, 64.0, 32.0, 16.0});
    EXPECT(points(fold, flat, {}, threads).rc == 0);
    Pts p = points(fold, flat, {32.0, 16.0, 96.0, 16.0, 57.5, 16.0, 40.0, 20.0}, threads);
    EXPECT(p.rc == 0);
    if (p.rc == 0) {
      EXPECT(p.status[0] == 0 && p.out[0] == 32.0 && p.out[1] == 16.0 && p.iters[0] == 1);
      EXPECT(p.status[1] == 1 && std::isnan(p.out[2]) && std::isnan(p.out[3]));
      EXPECT(p.status[2] == 0 && p.iters[2] == 100 && std::isfinite(p.out[4]));
      EXPECT(p.status[3] == 0 && p.iters[3] < 100);
    }
    p = points(flat, flat, {1.0, 2.0}, threads);
    EXPECT(p.rc == 0 && p.status[0] == 0 && p.iters[0] == 0 && p.out[0] == 1.0 && p.out[1] == 2.0);
  }
  // ---- refusals ----
  EXPECT(warp(cam(2, {NAN, 4.5, 3.25, 0.0}), pin, 9, 6, 9, 6, 3, 0, 1).rc != 0 && has("non-finite"));
  EXPECT(warp(cam(2, {0.0, 4.5, 3.25, 0.0}), pin, 9, 6, 9, 6, 3, 0, 1).rc != 0 && has("focal length is 0"));
  EXPECT(warp(cam(5, {1.0, 1.0, 1.0, 1.0, 0, 0, 0, 0}), pin, 9, 6, 9, 6, 3, 0, 1).rc != 0 && has("not built"));
  EXPECT(warp(cam(2, {64.0, 4.5, 3.25}), pin, 9, 6, 9, 6, 3, 0, 1).rc != 0 && has("parameters"));
  EXPECT(warp(quirk, pin, 9, 6, 9, 6, 2, 0, 1).rc != 0 && has("channel count"));
  EXPECT(warp(quirk, quirk, 9, 6, 9, 6, 3, 0, 1).rc != 0 && has("pinhole"));
  {
    const lt_undist_camera cams[2] = {quirk, pin};
    unsigned char px[4] = {0, 0, 0, 0};
    lt_undist_image im;
    std::memset(&im, 0, sizeof(im));
    im.src = px; im.dst = px;
    im.src_stride = im.dst_stride = 1;
    im.src_w = 0; im.src_h = 1; im.dst_w = 1; im.dst_h = 1;
    im.channels = 1;
    im.dst_cam = 1;
    EXPECT(lt_fn_undist_warp_host(2, cams, 1, &im, 1) != 0 && has("size below 1"));
    im.src_w = 2;
    EXPECT(lt_fn_undist_warp_host(2, cams, 1, &im, 1) != 0 && has("stride"));
    im.src_stride = 2;
    im.dst_cam = 2;
    EXPECT(lt_fn_undist_warp_host(2, cams, 1, &im, 1) != 0 && has("camera index"));
    EXPECT(lt_fn_undist_warp_host(2, cams, 0, nullptr, 1) == 0);
    const double xy[2] = {1.0, 1.0};
    const int32_t bad = 7, good = 0;
    double out[2];
    int32_t st, it;
    EXPECT(lt_fn_undist_points_host(2, cams, 1, xy, &bad, &good, out, &st, &it, 1) != 0 && has("camera index"));
  }
  // ---- the scale rule ----
  {
    const double ext[8] = {-1.0, -0.5, 41.0, 42.0, -2.0, -1.0, 31.0, 33.0};
    double out[4];
    EXPECT(lt_fn_undist_scale(40, 30, 20.0, 15.0, ext, 0.0, 0.2, 2.0, out) == 0 && out[0] >= 1.0 && out[1] >= 1.0);
    EXPECT(lt_fn_undist_scale(40, 30, 20.0, 15.0, ext, 1.0, 0.2, 2.0, out) == 0);
    EXPECT(lt_fn_undist_scale(40, 30, 20.0, 15.0, ext, 1.5, 0.2, 2.0, out) != 0 && has("blank_pixels"));
    EXPECT(lt_fn_undist_scale(40, 30, 20.0, 15.0, ext, 0.0, 0.0, 2.0, out) != 0 && has("min_scale"));
    EXPECT(lt_fn_undist_scale(40, 30, 20.0, 15.0, ext, 0.0, 3.0, 2.0, out) != 0 && has("max_scale"));
    const double on_centre[8] = {20.0, 20.0, 20.0, 20.0, 15.0, 15.0, 15.0, 15.0};  // every quotient divides by zero
    EXPECT(lt_fn_undist_scale(40, 30, 20.0, 15.0, on_centre, 0.0, 0.2, 2.0, out) != 0 && has("no scale"));
    const double far[8] = {-1e9, -1e9, 1e9, 1e9, -1e9, -1e9, 1e9, 1e9};  // clamped at max_scale
    EXPECT(lt_fn_undist_scale(40, 30, 20.0, 15.0, far, 0.0, 0.2, 2.0, out) == 0 && out[0] == 80.0 && out[1] == 60.0);
    const double nan_ext[8] = {NAN, 0, 0, 0, 0, 0, 0, 0};
    EXPECT(lt_fn_undist_scale(40, 30, 20.0, 15.0, nan_ext, 0.0, 0.2, 2.0, out) != 0 && has("non-finite"));
  }
  return finish("undist_host_asan");
}
