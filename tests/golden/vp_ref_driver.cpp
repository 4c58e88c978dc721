// vp_ref_driver.cpp -- C entry points over the reference's own vplib::JLinkage::JLinkage, for make_vp_golden.py.
//
// The generator compiles this file together with the reference's vplib/base_vp_detector.cc and
// vplib/JLinkage/JLinkage.cc where they lie, against the stand-in headers of oracle/ref_shim and the objects
// `make -C oracle ref` builds (oracle/_ref/obj/**/*.o: base/linebase.o, base/infinite_line.o, base/graph.o).  The two
// headers of the J-Linkage third party are not on disk: the generator writes stand-ins into its temporary directory
// whose run() functions record what they are given and return the Labels / LabelCount injected through vp_inject below.  Everything around the two calls is the reference's code.
#include "limap/vplib/JLinkage/JLinkage.h"

#include <cstdint>
#include <vector>

namespace vp_inject {
std::vector<unsigned int> labels, counts;
std::vector<float> seen_pts;
float seen_threshold = 0.f;
int sample_calls = 0, cluster_calls = 0;
}  // namespace vp_inject

using namespace limap;

extern "C" {

void vp_set_injection(const unsigned int *labels, int64_t n, const unsigned int *counts, int64_t n_counts) {
  vp_inject::labels.assign(labels, labels + n);
  vp_inject::counts.assign(counts, counts + n_counts);
  vp_inject::seen_pts.clear();
  vp_inject::sample_calls = vp_inject::cluster_calls = 0;
}

// AssociateVPs under the given configuration; labels_out[n], vps_out[3 * vps_cap]; returns the number of vps
int64_t vp_associate(double min_length, double inlier_threshold, int min_num_supports, double th_perp_supports,
                     const double *l4, int64_t n, int *labels_out, double *vps_out, int64_t vps_cap) {
  vplib::JLinkage::JLinkageConfig cfg;
  cfg.min_length = min_length;
  cfg.inlier_threshold = inlier_threshold;
  cfg.min_num_supports = min_num_supports;
  cfg.th_perp_supports = th_perp_supports;
  vplib::JLinkage::JLinkage det(cfg);
  std::vector<Line2d> lines;
  lines.reserve((size_t)n);
  for (int64_t k = 0; k < n; ++k) lines.emplace_back(V2D(l4[4 * k], l4[4 * k + 1]), V2D(l4[4 * k + 2], l4[4 * k + 3]));
  const vplib::VPResult res = det.AssociateVPs(lines);
  for (size_t k = 0; k < res.labels.size(); ++k) labels_out[k] = res.labels[k];
  const int64_t nv = (int64_t)res.vps.size();
  for (int64_t v = 0; v < nv && v < vps_cap; ++v)
    for (int c = 0; c < 3; ++c) vps_out[3 * v + c] = res.vps[(size_t)v][c];
  return nv;
}

int vp_sample_calls() { return vp_inject::sample_calls; }
int vp_cluster_calls() { return vp_inject::cluster_calls; }
float vp_seen_threshold() { return vp_inject::seen_threshold; }
int64_t vp_seen_points(float *out) {  // 4 floats per line the clustering call received
  if (out)
    for (size_t k = 0; k < vp_inject::seen_pts.size(); ++k) out[k] = vp_inject::seen_pts[k];
  return (int64_t)vp_inject::seen_pts.size() / 4;
}

}  // extern "C"
