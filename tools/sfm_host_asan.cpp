// sfm_host_asan.cpp -- the host path of limap_amd.pointsfm (lt_fn_sfm_neighbors_host, lt_fn_sfm_ranges of lt_sfm_host.cpp)
// under AddressSanitizer and UBSan, as a program of its own: lt_sfm_host.cpp, the host-only unit, is compiled into it
// with the sanitizers; nothing is loaded into Python and no device is touched.  `make -C limap_amd/csrc sfm_asan` builds
// and runs it (tests/test_sfm_host.py does that).
// The cases are the degenerate ones: no images, no points, tracks of length 0 and 1, repeated images, skipped slots
// only, one image, a bad index, non-finite input, every undefined range.
#include "host_asan.h"

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include <cstdio>
#include <cstdlib>
#include <limits>

namespace {

struct Out {
  int rc;
  std::vector<int64_t> off;
  std::vector<int32_t> nb, ij, shared;
  std::vector<float> angle;
};

Out run(int n_img, const std::vector<float> &R, const std::vector<float> &T, const std::vector<float> &xyz,
        const std::vector<int64_t> &off, const std::vector<int32_t> &img, int kind, int64_t k, int threads) {
  Out o;
  int64_t n_nb = -1, n_pairs = -1;
  o.rc = lt_fn_sfm_neighbors_host(n_img, R.data(), T.data(), (int64_t)off.size() - 1, xyz.data(), off.data(), img.data(),
                                  kind, k, 1.0, threads, &n_nb, &n_pairs);
  if (o.rc != 0) return o;
  // exactly as large as the counts say: an overrun of one element is the sanitizer's to find
  o.off.resize((size_t)n_img + 1);
  o.nb.resize((size_t)n_nb);
  o.ij.resize(2 * (size_t)n_pairs);
  o.shared.resize((size_t)n_pairs);
  o.angle.resize((size_t)n_pairs);
  lt_fn_sfm_host_get(o.off.data(), o.nb.data(), o.ij.data(), o.shared.data(), o.angle.data());
  return o;
}

std::vector<float> poses_R(int n) {
  std::vector<float> R(9 * (size_t)n, 0.f);
  for (int i = 0; i < n; ++i) R[9 * i] = R[9 * i + 4] = R[9 * i + 8] = 1.f;
  return R;
}
std::vector<float> poses_T(int n) {
  std::vector<float> T(3 * (size_t)n, 0.f);
  for (int i = 0; i < n; ++i) T[3 * i] = -(float)i;  // centres at x = 0, 1, 2, ...
  return T;
}

}  // namespace

int main() {
  for (int threads : {1, 4}) {
    for (int kind = 0; kind < 3; ++kind) {
      // no images, no points
      Out o = run(0, {}, {}, {}, {0}, {}, kind, 5, threads);
      EXPECT(o.rc == 0 && o.off.size() == 1 && o.nb.empty() && o.shared.empty());
      // images without points
      o = run(3, poses_R(3), poses_T(3), {}, {0}, {}, kind, 5, threads);
      EXPECT(o.rc == 0 && o.off == std::vector<int64_t>(4, 0));
      // tracks of length 0 and 1, image 4 in no track, repeats, one real pair next to a repeat
      const std::vector<int32_t> img = {0, 2, 2, 1, 1, 1, 0, 1, 0, 0, 3, 3, 1, 2};
      const std::vector<int64_t> off = {0, 0, 1, 3, 6, 9, 11, 14, 14};
      std::vector<float> xyz(3 * 8, 0.f);
      for (int p = 0; p < 8; ++p) { xyz[3 * p] = 0.3f * p; xyz[3 * p + 2] = 5.f; }
      o = run(5, poses_R(5), poses_T(5), xyz, off, img, kind, 5, threads);
      EXPECT(o.rc == 0 && o.shared.size() == 5 && o.shared[0] == 2 && o.off[5] == o.off[4]);
      EXPECT(o.ij == (std::vector<int32_t>{0, 1, 0, 3, 1, 2, 1, 3, 2, 3}));
      o = run(5, poses_R(5), poses_T(5), xyz, off, img, kind, 0, threads);
      EXPECT(o.rc == 0 && o.nb.empty() && o.shared.size() == 5);
      // skipped slots only; one image
      o = run(3, poses_R(3), poses_T(3), {0, 0, 5, 1, 0, 5, 2, 0, 5}, {0, 2, 5, 7}, {1, 1, 2, 2, 2, 0, 0}, kind, 5, threads);
      EXPECT(o.rc == 0 && o.nb.empty() && o.shared.empty());
      o = run(1, poses_R(1), poses_T(1), {0, 0, 5, 1, 0, 5}, {0, 1, 3}, {0, 0, 0}, kind, 5, threads);
      EXPECT(o.rc == 0 && o.off == (std::vector<int64_t>{0, 0}) && o.shared.empty());
      // a track that names its images more than once: shared = 6 > n_0 + n_1 = 5, the IoU is negative (or +inf)
      o = run(3, poses_R(3), poses_T(3), {0.5f, 0, 5}, {0, 6}, {0, 0, 0, 1, 1, 2}, kind, 5, threads);
      EXPECT(o.rc == 0 && o.shared == (std::vector<int32_t>{6, 3, 2}) && o.nb.size() == 6);
      EXPECT(o.nb[0] == (kind == 1 ? 2 : 1));  // image 0: overlap 6 > 3, Dice 12/5 > 6/4, but IoU 6/(5 - 6) < 3/(4 - 3)
      o = run(3, poses_R(3), poses_T(3), {0.5f, 0, 5}, {0, 5}, {0, 0, 1, 1, 2}, kind, 5, threads);
      EXPECT(o.rc == 0 && o.shared == (std::vector<int32_t>{4, 2, 2}) && o.nb.size() == 6 && o.nb[0] == 1);
      // a point on a projection centre (den == 0) and two cameras in one place
      o = run(2, poses_R(2), {0, 0, 0, 0, 0, 0}, {0, 0, 0, 1, 1, 1}, {0, 2, 4}, {0, 1, 1, 0}, kind, 5, threads);
      EXPECT(o.rc == 0 && o.shared.size() == 1 && o.shared[0] == 2 && o.angle[0] == 0.f && o.nb.empty());
    }
  }
  // refused input
  EXPECT(run(2, poses_R(2), poses_T(2), {0, 0, 5}, {0, 2}, {0, 2}, 1, 5, 1).rc == LT_ERR_ARGUMENT);
  EXPECT(std::string(lt_fn_sfm_host_error()).rfind("unknown image index 2", 0) == 0);
  EXPECT(run(2, poses_R(2), poses_T(2), {0, 0, 5}, {0, 2}, {0, -1}, 1, 5, 1).rc == LT_ERR_ARGUMENT);
  EXPECT(run(2, poses_R(2), poses_T(2), {0, 0, 5}, {1, 2}, {0, 1}, 1, 5, 1).rc == LT_ERR_ARGUMENT);
  EXPECT(run(2, poses_R(2), poses_T(2), {0, 0, 5}, {0, 2}, {0, 1}, 3, 5, 1).rc == LT_ERR_ARGUMENT);
  EXPECT(run(2, poses_R(2), poses_T(2), {0, 0, 5}, {0, 2}, {0, 1}, 1, -1, 1).rc == LT_ERR_ARGUMENT);
  EXPECT(run(2, poses_R(2), poses_T(2), {0, std::numeric_limits<float>::infinity(), 5}, {0, 2}, {0, 1}, 1, 5, 1).rc ==
         LT_ERR_ARGUMENT);
  // ranges
  double lo[3], hi[3];
  std::vector<float> pts(3 * 20);
  for (int p = 0; p < 20; ++p) { pts[3 * p] = (float)((7 * p) % 20); pts[3 * p + 1] = 2.f * pts[3 * p]; pts[3 * p + 2] = -pts[3 * p]; }
  EXPECT(lt_fn_sfm_ranges(20, pts.data(), 0.05, 0.95, 1.25, lo, hi) == 0);
  EXPECT(lo[0] == -21.5 && hi[0] == 41.5 && lo[1] == -43.0 && hi[1] == 83.0 && lo[2] == -40.5 && hi[2] == 22.5);
  EXPECT(lt_fn_sfm_ranges(1, pts.data(), 0.0, 0.5, 1.25, lo, hi) == 0 && lo[0] == 0.0 && hi[0] == 0.0);
  EXPECT(lt_fn_sfm_ranges(0, pts.data(), 0.05, 0.95, 1.25, lo, hi) == LT_ERR_ARGUMENT);
  EXPECT(lt_fn_sfm_ranges(0, nullptr, 0.05, 0.95, 1.25, lo, hi) == LT_ERR_ARGUMENT);
  EXPECT(lt_fn_sfm_ranges(20, pts.data(), 0.05, 1.0, 1.25, lo, hi) == LT_ERR_ARGUMENT);
  EXPECT(lt_fn_sfm_ranges(20, pts.data(), -0.1, 0.9, 1.25, lo, hi) == LT_ERR_ARGUMENT);
  EXPECT(lt_fn_sfm_ranges(20, pts.data(), std::nan(""), 0.9, 1.25, lo, hi) == LT_ERR_ARGUMENT);
  EXPECT(lt_fn_sfm_ranges(20, pts.data(), 0.05, 1e30, 1.25, lo, hi) == LT_ERR_ARGUMENT);
  pts[7] = std::nanf("");
  EXPECT(lt_fn_sfm_ranges(20, pts.data(), 0.05, 0.95, 1.25, lo, hi) == LT_ERR_ARGUMENT);
  return finish("sfm_host_asan");
}
