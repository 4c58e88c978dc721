// lt_sfm_host.h -- what the device entry point (lt_sfm.cpp) and the host-only entry points (lt_sfm_host.cpp) of the
// visual neighbours share on the host: the validated model and the gate.  lt_sfm_host.cpp links without the device
// side (tools/sfm_host_asan.cpp builds it into a sanitizer program of its own).
#pragma once

#include "lt_sfm.h"

#include <cstdint>
#include <string>
#include <vector>

namespace lt_impl {

struct SfmPrep {
  int n_img = 0;
  long long n_pts = 0, n_slots = 0;
  std::vector<double> centres;      // 3 per image
  std::vector<int> n_points;        // ComputeNumPoints
  std::vector<long long> pair_off;  // n_pts + 1
};

// validates the arrays of a model and derives what both paths start from; 0, or 1 with msg set.  A message that starts
// with "unknown" is an index error (upstream's std::out_of_range of .at()), any other a value error
int sfm_prepare(int n_img, const float *R9, const float *T3, int64_t n_pts, const float *xyz, const int64_t *track_off,
                const int32_t *track_img, int kind, int64_t num_images, double min_angle_deg, SfmPrep &m,
                std::string &msg);

// colmap::DegToRad in double, narrowed where upstream assigns it to `const float min_triangulation_angle_rad`
inline float sfm_gate_of(double min_angle_deg) {
  return (float)(min_angle_deg * 0.0174532925199432954743716805978692718781530857086181640625);
}

// pair records into the arrays of lt_sfm_get_pairs (any pointer may be null)
void sfm_copy_pairs(const std::vector<lt::SfmPair> &pairs, int32_t *ij, int32_t *shared, float *angle);

}  // namespace lt_impl
