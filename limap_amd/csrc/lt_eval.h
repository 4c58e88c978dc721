// lt_eval.h -- records shared by the host side (lt_eval.cpp) and the device side (lt_kernels_eval.hip) of
// the line-map evaluation (limap.evaluation: PointCloudEvaluator, RefLineEvaluator, MeshEvaluator).  DESIGN §14, §15.
#pragma once

#include <hip/hip_runtime.h>

namespace lt {

constexpr int kEvalBucket = 32;     // cloud points per leaf bucket (consecutive in Morton order)
constexpr int kEvalFanout = 8;      // children per node of the implicit AABB hierarchy
constexpr int kEvalMaxLevels = 16;  // 32 * 8^15 points: far beyond any cloud that fits a device
constexpr int kEvalMaxTh = 64;      // thresholds per call
constexpr double kEvalEps = 1e-12;  // util/types.h EPS (RefLineEvaluator::DistPointLines' early exit)

// one line, prepared on the host once: direction and length as Line3d::direction() / length() compute them, and the
// sample spacing of RefLineEvaluator (length / (n - 1))
struct EvalLine {
  double s[3], e[3], d[3];
  double len, rint, pad_;
};

// the level table of an index: leaf buckets over n members in Morton order and an implicit fanout-8 hierarchy of AABBs
// over them, levels bottom (0: the buckets) to top (one root)
struct EvalLevels {
  long long n;
  long long total;  // nodes of all levels
  long long lvl_off[kEvalMaxLevels], lvl_n[kEvalMaxLevels];
  int top;
};

// the levels of n members in buckets of `bucket`, then fanout 8 up to one root
inline EvalLevels eval_levels(long long n, int bucket) {
  EvalLevels L{};
  L.n = n;
  long long cnt = (n + bucket - 1) / bucket;
  int l = 0;
  for (;; ++l) {
    L.lvl_off[l] = L.total;
    L.lvl_n[l] = cnt;
    L.total += cnt;
    if (cnt == 1) break;
    cnt = (cnt + kEvalFanout - 1) / kEvalFanout;
  }
  L.top = l;
  return L;
}

// the point index: the cloud in Morton order (SoA), leaf buckets of kEvalBucket points.  box: 6 doubles per node (lo, hi).
struct EvalTree {
  const double *x, *y, *z;
  const double *box;
  EvalLevels L;
  // what the hierarchy walk asks of an index (lt_kernels_eval.hip): a lower bound of the computed squared distance of p
  // to everything below a node, and the scan of leaf bucket b, which returns the new best
  __device__ double bound2(long long node, const double p[3]) const;
  __device__ double scan(long long b, const double p[3], double best) const;
};

enum EvalQueryMode { EV_Q_POINTS = 0, EV_Q_CENTER = 1, EV_Q_ENDS = 2, EV_Q_REFLINE = 3 };

// where the query points come from: free points (x, y, z with a stride) or the samples of lines, generated in the
// kernel from (line, i) -- query q is sample q % n of line q / n
struct EvalQuery {
  const double *x, *y, *z;
  long long stride;
  const EvalLine *lines;
  double interval;  // 1 / n (EV_Q_CENTER), 1 / (n - 1) (EV_Q_ENDS)
  int mode, n;
};

constexpr int kMeshBucket = 4;      // faces per leaf bucket (consecutive in the Morton order of the centroids), DESIGN §15
constexpr int kMeshMaxBucket = 64;  // LT_TEST_MESH_BUCKET: the bucket sizes a measurement may try

// the triangle index: the faces in the Morton order of their centroids, as nine SoA vertex arrays (a, b, c: x, y, z),
// leaf buckets of `bucket` faces.  box: 6 doubles per node, the leaf boxes widened by a few ulps of their coordinates
// (DESIGN §15); eta: per node the largest region-7 slack factor of the faces below it (+inf: a near-degenerate face,
// the node is never pruned).
struct MeshTree {
  const double *v[9];
  const double *box, *eta;
  EvalLevels L;
  int bucket;
  __device__ double bound2(long long node, const double p[3]) const;  // as EvalTree's
  __device__ double scan(long long b, const double p[3], double best) const;
};

void launch_eval_bbox(hipStream_t st, const void *xyz, int dtype, long long n, unsigned long long *keys6);
void launch_eval_morton(hipStream_t st, const void *xyz, int dtype, long long n, const double lo[3],
                        const double scale[3], unsigned long long *keys, unsigned *idx);
size_t eval_sort_temp_bytes(long long n);
int launch_eval_sort(hipStream_t st, void *temp, size_t temp_bytes, long long n, const unsigned long long *keys_in,
                     unsigned long long *keys_out, const unsigned *idx_in, unsigned *idx_out);
void launch_eval_gather(hipStream_t st, const void *xyz, int dtype, long long n, const unsigned *perm, double *x,
                        double *y, double *z);
void launch_eval_boxes(hipStream_t st, const EvalTree &T, double *box);
void launch_eval_nearest(hipStream_t st, const EvalTree &T, const EvalQuery &Q, long long nq, double *dist);
// form 0: Line3d::point_distance, minimum DBL_MAX; form 1: RefLineEvaluator::DistPointLine with the EPS rule.
// scatter (may be null): out[scatter[q]] instead of out[q]
void launch_eval_lines_min(hipStream_t st, int form, const EvalQuery &Q, long long nq, const EvalLine *lines,
                           long long n_lines, double *out, const unsigned *scatter);
// counts[l * n_th + t] = #{i < n : dist[l * n + i] <= th[t]} (le) or < th[t] (!le), one block per line
void launch_eval_count(hipStream_t st, const double *dist, long long n_lines, int n, const double *th, int n_th, int le,
                       int *counts);

// the mesh index: centroids (nf x 3) of faces F (int64, validated) over vertices V (nv x 3, scaled)
void launch_mesh_centroids(hipStream_t st, const double *V, const long long *F, long long nf, double *cen);
// faces in the order perm into the nine SoA arrays of T
void launch_mesh_gather(hipStream_t st, const double *V, const long long *F, long long nf, const unsigned *perm,
                        double *const out[9]);
// leaf boxes and slack factors, then the levels above (k_eval_level_boxes and the maximum of eta)
void launch_mesh_boxes(hipStream_t st, const MeshTree &T, double *box, double *eta);
// squared-distance minimum over the faces, sqrt at the end: the hierarchy walk, or (brute) every face, staged in LDS
void launch_mesh_nearest(hipStream_t st, const MeshTree &T, const EvalQuery &Q, long long nq, int brute, double *dist);

}  // namespace lt
