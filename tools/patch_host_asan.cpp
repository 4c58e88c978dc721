// patch_host_asan.cpp -- the host path of limap_amd.features (lt_fn_patch_extract_host, lt_fn_patch_geometry,
// lt_fn_patch_ranges of lt_patch.cpp) under AddressSanitizer and UBSan, as a program of its own: lt_patch.cpp is
// compiled into it with LT_HOST_ONLY and the sanitizers; nothing is loaded into Python and no device is touched.
// `make -C limap_amd/csrc patch_asan` builds and runs it (tests/test_patch_host.py does that).
// The cases are the degenerate ones of the tests: a 1x1 map, one row, one column, every input and output type, channel
// counts 1, 3 and 8, a (C, H, W) map read through its strides, patches that hang over every edge or lie outside the
// image, a zero-length line, range_perp 0, no lines, the narrowing's edge values, tracks without supports, and every
// refusal.  Buffers are exactly as large as the sizes say: an overrun of one element is the sanitizer's to find.
#include "host_asan.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

int esize(int dtype) { return dtype == LT_PATCH_F16 ? 2 : (dtype == LT_PATCH_F32 ? 4 : 8); }

bool has(const char *what) { return host_asan::has(lt_fn_patch_host_error, what); }

const std::vector<double> kLines = {
    2.0, 3.0, 6.0, 3.0,      // horizontal
    4.0, -5.0, 4.0, 12.0,    // over the top and the bottom
    -7.0, 2.0, 15.0, 4.5,    // over the left and the right
    -50.0, -60.0, -40.0, -70.0,  // outside
    3.25, 2.5, 3.25, 2.5,    // zero length
};

// extracts kLines from an h x w x c map of in_dtype whose bytes are a pattern; layout 0: (h, w, c), 1: (c, h, w)
// through strides.  Returns the call's code; on success checks the size the geometry announces.
int run(int h, int w, int c, int in_dtype, int out_dtype, int layout, lt_patch_config cfg, int threads, int64_t n = -1) {
  const int64_t n_lines = n < 0 ? (int64_t)kLines.size() / 4 : n;
  std::vector<unsigned char> map((size_t)h * w * c * esize(in_dtype));
  for (size_t k = 0; k < map.size(); ++k) map[k] = (unsigned char)(k % 2 == 1 && in_dtype == LT_PATCH_F16 ? 0x3c : 37 * k + 11);
  if (in_dtype != LT_PATCH_F16)  // keep the values finite: clear the top exponent bit of every element
    for (size_t k = (size_t)esize(in_dtype) - 1; k < map.size(); k += (size_t)esize(in_dtype)) map[k] &= 0x3f;
  lt_feature_map fm;
  std::memset(&fm, 0, sizeof(fm));
  fm.ptr = map.data();
  fm.h = h; fm.w = w; fm.c = c;
  if (layout == 0) { fm.row_stride = (int64_t)w * c; fm.pix_stride = c; fm.chan_stride = 1; }
  else { fm.row_stride = w; fm.pix_stride = 1; fm.chan_stride = (int64_t)h * w; }
  fm.dtype = in_dtype;
  std::vector<int32_t> hs((size_t)n_lines + 1);
  std::vector<int64_t> off((size_t)n_lines + 1);
  std::vector<double> R((size_t)(4 * n_lines) + 1), tv((size_t)(2 * n_lines) + 1);
  int rc = lt_fn_patch_geometry(&cfg, c, n_lines, kLines.data(), R.data(), tv.data(), hs.data(), off.data());
  if (rc != 0) return rc;
  std::vector<unsigned char> out((size_t)off[(size_t)n_lines] * esize(out_dtype));
  rc = lt_fn_patch_extract_host(&cfg, &fm, n_lines, kLines.data(), out_dtype, out.empty() ? nullptr : out.data(), threads);
  if (rc == 0 && n_lines > 0) EXPECT(off[1] == (int64_t)hs[0] * (cfg.range_perp + 1) * c);
  return rc;
}

}  // namespace

int main() {
  lt_patch_config def;
  lt_patch_config_default(&def);
  EXPECT(def.k_stretch == 1.0 && def.t_stretch == 10 && def.range_perp == 20);
  const int types[3] = {LT_PATCH_F16, LT_PATCH_F32, LT_PATCH_F64};
  for (int threads : {1, 4})
    for (int in : types)
      for (int out : types)
        for (int c : {1, 3, 8})
          for (int layout : {0, 1}) {
            EXPECT(run(7, 9, c, in, out, layout, def, threads) == 0);
            EXPECT(run(1, 1, c, in, out, layout, def, threads) == 0);
          }
  EXPECT(run(1, 9, 2, LT_PATCH_F32, LT_PATCH_F16, 0, def, 2) == 0);
  EXPECT(run(7, 1, 2, LT_PATCH_F32, LT_PATCH_F16, 1, def, 2) == 0);
  EXPECT(run(7, 9, 2, LT_PATCH_F64, LT_PATCH_F16, 0, lt_patch_config{1.0, 0, 0}, 2) == 0);
  EXPECT(run(7, 9, 2, LT_PATCH_F64, LT_PATCH_F32, 0, lt_patch_config{1.5, 0, 15}, 2) == 0);
  EXPECT(run(7, 9, 2, LT_PATCH_F64, LT_PATCH_F64, 0, def, 2, 0) == 0);  // no lines

  // ---- a known answer and the single rounding: node-exact samples of a constant map ----
  {
    const double tie = 1.0 + std::ldexp(1.0, -11) + std::ldexp(1.0, -30);
    std::vector<double> map(40 * 48, tie);
    lt_feature_map fm;
    std::memset(&fm, 0, sizeof(fm));
    fm.ptr = map.data();
    fm.h = 40; fm.w = 48; fm.c = 1; fm.row_stride = 48; fm.pix_stride = 1; fm.chan_stride = 1;
    fm.dtype = LT_PATCH_F64;
    const double line[4] = {10.0, 20.0, 30.0, 20.0};
    lt_patch_config cfg{1.0, 10, 16};
    double R[4], tv[2];
    int32_t h;
    int64_t off[2];
    EXPECT(lt_fn_patch_geometry(&cfg, 1, 1, line, R, tv, &h, off) == 0);
    EXPECT(h == 31 && off[1] == 31 * 17 && R[0] == 0.0 && R[1] == -1.0 && R[2] == 1.0 && R[3] == 0.0 && tv[0] == 5.0 && tv[1] == 28.0);
    std::vector<uint16_t> out((size_t)off[1]);
    EXPECT(lt_fn_patch_extract_host(&cfg, &fm, 1, line, LT_PATCH_F16, out.data(), 1) == 0);
    bool ok = true;
    for (uint16_t v : out) ok = ok && v == 0x3c01;  // 1 + 2^-10; through float it would be 0x3c00
    EXPECT(ok);
    // edge values of the narrowing: the largest half, the overflow threshold, the subnormal range, a tie to even
    const double vals[8] = {65504.0, 65520.0, std::ldexp(1.0, -24), std::ldexp(1.0, -25), std::ldexp(3.0, -25), 1e9, -1e-30, 1e-320};
    const uint16_t want[8] = {0x7bff, 0x7c00, 0x0001, 0x0000, 0x0002, 0x7c00, 0x8000, 0x0000};
    for (int k = 0; k < 8; ++k) {
      for (double &v : map) v = vals[k];
      EXPECT(lt_fn_patch_extract_host(&cfg, &fm, 1, line, LT_PATCH_F16, out.data(), 1) == 0);
      EXPECT(out[0] == want[k] && out.back() == want[k]);
    }
  }

  // ---- ranges ----
  {
    const double line6[12] = {-0.2, -0.15, 6.0, 0.25, 0.2, 7.0, -0.2, -0.15, 6.0, 0.25, 0.2, -1.0};
    const int64_t sup_off[3] = {0, 2, 2};  // the second track has no support at all
    const int32_t sup_img[2] = {7, 3};
    const double seg4[8] = {10.0, 8.0, 30.0, 22.0, 0.0, 0.0, 100.0, 100.0};
    const int32_t pair_track[4] = {0, 0, 1, 1}, pair_img[4] = {7, 9, 7, 3};
    double cam[44];
    const double one[11] = {500.0, 480.0, 24.0, 20.0, 0.98, 0.05, -0.12, 0.03, 0.2, -0.1, 0.4};
    for (int k = 0; k < 44; ++k) cam[k] = one[k % 11];
    double range4[16];
    int32_t status[4];
    EXPECT(lt_fn_patch_ranges(2, line6, sup_off, sup_img, seg4, 4, pair_track, pair_img, cam, range4, status) == 0);
    EXPECT(status[0] == 0 && status[1] == 1 && status[2] == 1 && status[3] == 1);
    EXPECT(std::isfinite(range4[0]) && std::isfinite(range4[3]));
    const int64_t sup_off2[3] = {0, 1, 2};
    EXPECT(lt_fn_patch_ranges(2, line6, sup_off2, sup_img, seg4, 4, pair_track, pair_img, cam, range4, status) == 0);
    EXPECT(status[0] == 0 && status[3] == 2);  // the second track ends behind the camera
    EXPECT(lt_fn_patch_ranges(0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    const int32_t bad_track[1] = {2};
    EXPECT(lt_fn_patch_ranges(2, line6, sup_off2, sup_img, seg4, 1, bad_track, pair_img, cam, range4, status) != 0 && has("track index"));
    const int64_t bad_off[3] = {0, 2, 1};
    EXPECT(lt_fn_patch_ranges(2, line6, bad_off, sup_img, seg4, 1, pair_track, pair_img, cam, range4, status) != 0 && has("decrease"));
    double nan_line[12];
    std::memcpy(nan_line, line6, sizeof(line6));
    nan_line[4] = NAN;
    EXPECT(lt_fn_patch_ranges(2, nan_line, sup_off2, sup_img, seg4, 1, pair_track, pair_img, cam, range4, status) != 0 && has("non-finite 3D line"));
  }

  // ---- refusals ----
  EXPECT(run(7, 9, 2, LT_PATCH_F64, LT_PATCH_F64, 0, lt_patch_config{1.0, 10, -1}, 1) != 0 && has("range_perp below 0"));
  EXPECT(run(7, 9, 2, LT_PATCH_F64, LT_PATCH_F64, 0, lt_patch_config{1.0, -1, 4}, 1) != 0 && has("t_stretch below 0"));
  EXPECT(run(7, 9, 2, LT_PATCH_F64, LT_PATCH_F64, 0, lt_patch_config{NAN, 10, 4}, 1) != 0 && has("k_stretch"));
  EXPECT(run(7, 9, 2, LT_PATCH_F64, LT_PATCH_F64, 0, lt_patch_config{1e300, 10, 4}, 1) != 0 && has("rows"));
  EXPECT(run(7, 9, 2, LT_PATCH_F64, LT_PATCH_F64, 0, lt_patch_config{1.0, 10, 5000}, 1) != 0 && has("range_perp above"));
  {
    double px = 0.0, out[11 * 21];
    lt_feature_map fm;
    std::memset(&fm, 0, sizeof(fm));
    fm.ptr = &px;
    fm.h = 1; fm.w = 1; fm.c = 1; fm.row_stride = 1; fm.pix_stride = 1; fm.chan_stride = 1;
    fm.dtype = LT_PATCH_F64;
    const double line[4] = {0.0, 0.0, 0.0, 0.0}, bad[4] = {0.0, INFINITY, 0.0, 0.0};
    EXPECT(lt_fn_patch_extract_host(&def, &fm, 1, line, LT_PATCH_F64, out, 1) == 0);
    EXPECT(lt_fn_patch_extract_host(&def, &fm, 1, bad, LT_PATCH_F64, out, 1) != 0 && has("non-finite coordinate"));
    EXPECT(lt_fn_patch_extract_host(&def, &fm, 1, line, 9, out, 1) != 0 && has("unknown output dtype"));
    EXPECT(lt_fn_patch_extract_host(&def, nullptr, 1, line, LT_PATCH_F64, out, 1) != 0 && has("null feature map"));
    EXPECT(lt_fn_patch_extract_host(nullptr, &fm, 1, line, LT_PATCH_F64, out, 1) != 0 && has("null configuration"));
    EXPECT(lt_fn_patch_extract_host(&def, &fm, 1, line, LT_PATCH_F64, nullptr, 1) != 0 && has("null output"));
    fm.dtype = 4;
    EXPECT(lt_fn_patch_extract_host(&def, &fm, 1, line, LT_PATCH_F64, out, 1) != 0 && has("unknown feature map dtype"));
    fm.dtype = LT_PATCH_F64;
    fm.c = 0;
    EXPECT(lt_fn_patch_extract_host(&def, &fm, 1, line, LT_PATCH_F64, out, 1) != 0 && has("below 1"));
    fm.c = 1;
    fm.on_device = 1;
    EXPECT(lt_fn_patch_extract_host(&def, &fm, 1, line, LT_PATCH_F64, out, 1) != 0 && has("device feature map"));
    fm.on_device = 0;
    EXPECT(lt_fn_patch_extract_host(&def, &fm, 1, line, LT_PATCH_F64, out, 1) == 0 && has(""));
  }
  return finish("patch_host_asan");
}
