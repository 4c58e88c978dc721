// eval_ref_driver.cpp -- C entry points over the reference's own evaluation code, for make_eval_golden.py.
//
// Compiled together with the reference's evaluation/base_evaluator.cc, point_cloud_evaluator.cc and
// refline_evaluator.cc (read where they lie), linked against the objects `make -C oracle ref` builds from the
// reference's sources (oracle/_ref/obj/**/*.o: kd_tree.o, linebase.o) and built with the stand-in headers of
// oracle/ref_shim.  Lines are 6 doubles (start, end).
#include "limap/base/linebase.h"
#include "limap/evaluation/point_cloud_evaluator.h"
#include "limap/evaluation/refline_evaluator.h"

#include <omp.h>

#include <chrono>
#include <cstdint>
#include <vector>

using namespace limap;
using limap::evaluation::PointCloudEvaluator;
using limap::evaluation::RefLineEvaluator;

namespace {
std::vector<Line3d> to_lines(const double *a, int64_t n) {
  std::vector<Line3d> out;
  out.reserve((size_t)n);
  for (int64_t k = 0; k < n; ++k)
    out.emplace_back(V3D(a[6 * k], a[6 * k + 1], a[6 * k + 2]), V3D(a[6 * k + 3], a[6 * k + 4], a[6 * k + 5]));
  return out;
}
}  // namespace

extern "C" {

void *ev_pcd_create(const double *pts, int64_t n) {
  std::vector<V3D> v((size_t)n);
  for (int64_t k = 0; k < n; ++k) v[(size_t)k] = V3D(pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]);
  auto *e = new PointCloudEvaluator(v);
  e->Build();
  return e;
}
void ev_pcd_free(void *h) { delete static_cast<PointCloudEvaluator *>(h); }

void ev_dist_points(void *h, const double *q, int64_t m, double *out) {
  auto *e = static_cast<PointCloudEvaluator *>(h);
  for (int64_t k = 0; k < m; ++k) out[k] = e->ComputeDistPoint(V3D(q[3 * k], q[3 * k + 1], q[3 * k + 2]));
}

double ev_dist_line(void *h, const double *line, int n) {
  return static_cast<PointCloudEvaluator *>(h)->ComputeDistLine(to_lines(line, 1)[0], n);
}

double ev_inlier_ratio(void *h, const double *line, double th, int n) {
  return static_cast<PointCloudEvaluator *>(h)->ComputeInlierRatio(to_lines(line, 1)[0], th, n);
}

// inlier (1) or outlier (0) segments of all lines: returns the count, writes up to cap of them
int64_t ev_segs(void *h, const double *lines, int64_t L, double th, int n, int inlier, double *out, int64_t cap) {
  auto *e = static_cast<PointCloudEvaluator *>(h);
  const auto ls = to_lines(lines, L);
  const auto r = inlier ? e->ComputeInlierSegs(ls, th, n) : e->ComputeOutlierSegs(ls, th, n);
  for (size_t k = 0; k < r.size() && (int64_t)k < cap; ++k)
    for (int c = 0; c < 3; ++c) {
      out[6 * k + c] = r[k].start[c];
      out[6 * k + 3 + c] = r[k].end[c];
    }
  return (int64_t)r.size();
}

// ComputeDistsforEachPoint; returns its wall ms
double ev_dists_each(void *h, const double *lines, int64_t L, double *out) {
  auto *e = static_cast<PointCloudEvaluator *>(h);
  const auto ls = to_lines(lines, L);
  const auto t0 = std::chrono::steady_clock::now();
  const auto r = e->ComputeDistsforEachPoint(ls);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (size_t k = 0; k < r.size(); ++k) out[k] = r[k];
  return ms;
}

// which 0: ComputeRecallRef, 1: ComputeRecallTested, 2: SumLength of the reference lines
double ev_refline(const double *ref, int64_t R, const double *lines, int64_t L, double th, int n, int which) {
  RefLineEvaluator e(to_lines(ref, R));
  const auto ls = to_lines(lines, L);
  if (which == 2) return e.SumLength();
  return which == 0 ? e.ComputeRecallRef(ls, th, n) : e.ComputeRecallTested(ls, th, n);
}

int ev_threads() { return omp_get_max_threads(); }
void ev_set_threads(int n) { omp_set_num_threads(n); }

// wall ms of the reference's calls on one scene: [0] constructor + Build, [1] ComputeInlierRatio for every line at
// each threshold (the scripts' loop), [2] ComputeDistsforEachPoint
void ev_time_scene(const double *pts, int64_t n, const double *lines, int64_t L, const double *th, int n_th,
                   double ms[3]) {
  using clk = std::chrono::steady_clock;
  auto t0 = clk::now();
  void *h = ev_pcd_create(pts, n);
  auto t1 = clk::now();
  auto *e = static_cast<PointCloudEvaluator *>(h);
  const auto ls = to_lines(lines, L);
  volatile double sink = 0.0;
  for (int t = 0; t < n_th; ++t)
    for (const auto &l : ls) sink = sink + e->ComputeInlierRatio(l, th[t], 1000);
  auto t2 = clk::now();
  const auto r = e->ComputeDistsforEachPoint(ls);
  auto t3 = clk::now();
  sink = sink + r[0];
  ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
  ms[1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
  ms[2] = std::chrono::duration<double, std::milli>(t3 - t2).count();
  ev_pcd_free(h);
}

}  // extern "C"
