// bpt_ref_driver.cpp -- C entry points over the reference's own structures::PL_Bipartite2d, for make_bpt_golden.py.
//
// Linked against the objects `make -C oracle ref` builds from the reference's sources (oracle/_ref/obj/**/*.o:
// structures/pl_bipartite{,_base}.o, base/linebase.o, base/graph.o, util/kd_tree.o) and built with the stand-in
// headers of oracle/ref_shim.  Lines are 4 doubles (start, end), points 2.
#include "limap/base/linebase.h"
#include "limap/structures/pl_bipartite.h"
#include "limap/util/kd_tree.h"

#include <chrono>
#include <cstdint>
#include <vector>

using namespace limap;
using limap::structures::PL_Bipartite2d;
using limap::structures::PL_Bipartite2dConfig;

namespace {
std::vector<V2D> to_points(const double *a, int64_t n) {
  std::vector<V2D> out;
  out.reserve((size_t)n);
  for (int64_t k = 0; k < n; ++k) out.emplace_back(a[2 * k], a[2 * k + 1]);
  return out;
}
double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

extern "C" {

void *bpt_create(double th_keypoints, double th_intersection, double th_merge_junctions) {
  PL_Bipartite2dConfig cfg;
  cfg.threshold_keypoints = th_keypoints;
  cfg.threshold_intersection = th_intersection;
  cfg.threshold_merge_junctions = th_merge_junctions;
  return new PL_Bipartite2d(cfg);
}
void bpt_free(void *h) { delete static_cast<PL_Bipartite2d *>(h); }

// init_lines with the default ids 0 .. M - 1
void bpt_init_lines(void *h, const double *l4, int64_t M) {
  std::vector<Line2d> lines;
  lines.reserve((size_t)M);
  for (int64_t k = 0; k < M; ++k)
    lines.emplace_back(V2D(l4[4 * k], l4[4 * k + 1]), V2D(l4[4 * k + 2], l4[4 * k + 3]));
  static_cast<PL_Bipartite2d *>(h)->init_lines(lines);
}

// add_keypoints_with_point3D_ids; ids may be NULL (default ids); returns its wall ms
double bpt_add_keypoints(void *h, const double *xy, const int *point3D_ids, const int *ids, int64_t P) {
  const auto pts = to_points(xy, P);
  std::vector<int> p3d(point3D_ids, point3D_ids + P), id;
  if (ids) id.assign(ids, ids + P);
  const auto t0 = std::chrono::steady_clock::now();
  static_cast<PL_Bipartite2d *>(h)->add_keypoints_with_point3D_ids(pts, p3d, id);
  return ms_since(t0);
}

// compute_intersection_with_points; returns its wall ms
double bpt_intersection_with_points(void *h, const double *kps, int64_t K) {
  const auto pts = to_points(kps, K);
  const auto t0 = std::chrono::steady_clock::now();
  static_cast<PL_Bipartite2d *>(h)->compute_intersection_with_points(pts);
  return ms_since(t0);
}

int64_t bpt_count_points(void *h) { return (int64_t) static_cast<PL_Bipartite2d *>(h)->count_points(); }
int64_t bpt_count_edges(void *h) { return (int64_t) static_cast<PL_Bipartite2d *>(h)->count_edges(); }

// get_all_junctions: point ids, coordinates, point3D ids, and the CSR (off: count_points() + 1, ids: count_edges())
// of their line ids
void bpt_get_junctions(void *h, int *point_ids, double *xy, int *point3D_ids, int64_t *off, int *line_ids) {
  auto *b = static_cast<PL_Bipartite2d *>(h);
  const auto pids = b->get_point_ids();
  const auto juncs = b->get_all_junctions();
  int64_t n = 0;
  off[0] = 0;
  for (size_t k = 0; k < juncs.size(); ++k) {
    point_ids[k] = pids[k];
    xy[2 * k] = juncs[k].p.p[0];
    xy[2 * k + 1] = juncs[k].p.p[1];
    point3D_ids[k] = juncs[k].p.point3D_id;
    for (int l : juncs[k].line_ids) line_ids[n++] = l;
    off[k + 1] = n;
  }
}

// KDTree::point_distance of q against the tree of kps (z = 0), as compute_intersection_with_points builds it
void bpt_kdtree_dists(const double *kps, int64_t K, const double *q, int64_t n, double *out) {
  std::vector<V3D> pts;
  for (int64_t k = 0; k < K; ++k) pts.push_back(V3D(kps[2 * k], kps[2 * k + 1], 0.0));
  KDTree tree(pts);
  for (int64_t k = 0; k < n; ++k) out[k] = tree.point_distance(V3D(q[2 * k], q[2 * k + 1], 0.0));
}

}  // extern "C"
