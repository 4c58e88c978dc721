// lt_ingest.h -- what lt_refine, lt_ba and lt_assoc do with the cameras and tracks a caller passes in before they build
// their own tables: the camera arrays into an id-to-row map, one camera row into kvec / pose, one line track's supports
// in upstream's residual order, one point track into residual blocks.  The order of a line track's supports
// -- sorted image ids, then list order -- is the order every reduction of the three solvers runs in, so it exists once.
// Every function returns 0, or 1 with the message of the refusal; `what` is the caller's word for a track in its
// messages ("track", "line track").  Header-only: the stand-alone host programs compile one .cpp alone.
#pragma once

#include "lt_hostutil.h"
#include "lt_ba.h"

#include <algorithm>
#include <numeric>
#include <unordered_map>

namespace lt_impl {

typedef std::unordered_map<int, int> IdRows;

inline int ingest_cams(int n_img, const int32_t *ids, const double *k, const double *q, const double *t, IdRows &id2row,
                       std::string &msg) {
  if (n_img < 0 || (n_img > 0 && (!ids || !k || !q || !t))) { msg = "bad camera arrays"; return 1; }
  if (!all_finite(k, 4 * (long long)n_img) || !all_finite(q, 4 * (long long)n_img) || !all_finite(t, 3 * (long long)n_img)) {
    msg = "non-finite camera";
    return 1;
  }
  for (int n = 0; n < n_img; ++n)
    if (!id2row.emplace(ids[n], n).second) { msg = "image id " + std::to_string(ids[n]) + " appears twice"; return 1; }
  return 0;
}

// row r of the camera arrays into kvec[4] and pose[7] = (q normalised as CameraPose's constructor does, t); with
// `check`, a focal length of 0 and a zero quaternion are refused first
inline int ingest_cam_row(const int32_t *ids, const double *k, const double *q, const double *t, int r, bool check,
                          double kvec[4], double pose[7], std::string &msg) {
  k += 4 * r;
  q += 4 * r;
  if (check) {
    if (k[0] == 0.0 || k[1] == 0.0) { msg = "image " + std::to_string(ids[r]) + ": a focal length is 0"; return 1; }
    if (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0) { msg = "image " + std::to_string(ids[r]) + ": zero quaternion"; return 1; }
  }
  for (int x = 0; x < 4; ++x) kvec[x] = k[x];
  lt::lm_normalise_q(q, pose);
  for (int x = 0; x < 3; ++x) pose[4 + x] = t[3 * r + x];
  return 0;
}

// CHECK_GT(line.length(), 0.0) (infinite_line.cc:68)
inline int ingest_line_length(const char *what, long long n, const double l[6], std::string &msg) {
  const double dx = l[0] - l[3], dy = l[1] - l[4], dz = l[2] - l[5];
  if (std::sqrt((dx * dx + dy * dy) + dz * dz) > 0.0) return 0;
  msg = std::string(what) + " " + std::to_string(n) + ": the line has zero length";
  return 1;
}

// values[num_outliers] and values[2 K - 1 - num_outliers] of the K supports' end points (infinite_line.cc:284-285)
inline int ingest_outliers(const char *what, long long n, int num_outliers, int K, std::string &msg) {
  if (num_outliers >= 0 && num_outliers <= 2 * K - 1) return 0;
  msg = "num_outliers " + std::to_string(num_outliers) + " leaves the " + std::to_string(2 * K) + " values of " + what + " " +
        std::to_string(n);
  return 1;
}

// The K supports of line track n with the image ids img[0 .. K) in residual order (AddLineGeometricResiduals: sorted
// image ids, then list order -- a stable sort): each(k, x, row) takes the k-th of them, which is the caller's support x
// in the camera row `row` (imagecols_.camview(img_id): std::map::at refuses an unknown id).  *n_images: count_images()
struct SupportOrder {
  std::vector<int> order, ids;
};
template <class Each>
int ingest_supports(const char *what, long long n, const int32_t *img, int K, const IdRows &id2row, SupportOrder &w,
                    int *n_images, std::string &msg, Each each) {
  w.order.resize((size_t)K);
  std::iota(w.order.begin(), w.order.end(), 0);
  std::stable_sort(w.order.begin(), w.order.end(), [&](int x, int y) { return img[x] < img[y]; });
  w.ids.assign(img, img + K);
  std::sort(w.ids.begin(), w.ids.end());
  *n_images = (int)(std::unique(w.ids.begin(), w.ids.end()) - w.ids.begin());
  for (int k = 0; k < K; ++k) {
    const int x = w.order[(size_t)k];
    auto it = id2row.find(img[x]);
    if (it == id2row.end()) {
      msg = std::string(what) + " " + std::to_string(n) + ": image id " + std::to_string(img[x]) + " is not in the collection";
      return 1;
    }
    each(k, x, it->second);
  }
  return 0;
}

// the residual block of a 2D support g = (x1 y1 x2 y2) of line structure s: ScaledLoss weight length / 30
// (ComputeLineWeights)
inline lt::BaBlk line_blk(const double g[4], int row, int s) {
  const double ex = g[2] - g[0], ey = g[3] - g[1];
  return lt::BaBlk{{g[0], g[1], g[2], g[3]}, std::sqrt(ex * ex + ey * ey) / 30.0, row, s, 0, 1};
}

// the residual blocks of point track n = structure s, observations [off[n], off[n + 1]) in list order with the
// ScaledLoss weight w, appended to blk
inline int ingest_point_track(long long n, int s, const int64_t *off, const int32_t *img, const double *xy, double w,
                              const IdRows &id2row, std::vector<lt::BaBlk> &blk, std::string &msg) {
  for (long long i = off[n]; i < off[n + 1]; ++i) {
    auto it = id2row.find(img[i]);
    if (it == id2row.end()) {  // imagecols_.camview(img_id): std::map::at
      msg = "point track " + std::to_string(n) + ": image id " + std::to_string(img[i]) + " is not in the collection";
      return 1;
    }
    blk.push_back(lt::BaBlk{{xy[2 * i], xy[2 * i + 1], 0.0, 0.0}, w, it->second, s, 0, 0});
  }
  return 0;
}

}  // namespace lt_impl
