// lt_kernels_eval.hip -- device side of limap.evaluation (evaluation/point_cloud_evaluator.cc, base_evaluator.cc,
// refline_evaluator.cc of the reference): the point index (Morton order, buckets, an implicit AABB hierarchy), exact
// nearest-point queries on it, and the brute-force minima of point-to-segment distances.  DESIGN §14.  The same
// machinery over triangle faces for MeshEvaluator (mesh_evaluator.cc): DESIGN §15.
//
// Exactness: every distance is the reference's expression in its operation order (-ffp-contract=off); the minimum is
// kept over SQUARED distances and the one correctly rounded sqrt taken at the end, which gives the same double because
// sqrt is monotone.  The hierarchy only prunes a node whose lower bound is strictly greater than the best squared
// distance so far, and that bound never exceeds the computed squared distance of a point inside the box.

#include "lt_eval.h"

#include <cfloat>
#include <cmath>

#include <rocprim/device/device_radix_sort.hpp>

namespace lt {

namespace {

constexpr int kBlock = 256;
constexpr int kPerLane = 2;     // brute force: queries a lane keeps in registers
constexpr int kLineTile = 256;  // brute force: lines staged in LDS per pass (96 B each)

inline unsigned nblk(long long n, int b) { return (unsigned)((n + b - 1) / b); }

__device__ inline double load_coord(const void *xyz, int dtype, long long i) {
  return dtype ? reinterpret_cast<const double *>(xyz)[i] : (double)reinterpret_cast<const float *>(xyz)[i];
}

// the order-preserving map of a double to an unsigned key (for atomicMin / atomicMax)
__device__ inline unsigned long long ord_key(double v) {
  unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ inline unsigned long long spread21(unsigned long long v) {  // 21 bits -> every third of 63
  v &= 0x1fffffull;
  v = (v | v << 32) & 0x1f00000000ffffull;
  v = (v | v << 16) & 0x1f0000ff0000ffull;
  v = (v | v << 8) & 0x100f00f00f00f00full;
  v = (v | v << 4) & 0x10c30c30c30c30c3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}

__device__ inline unsigned quant21(double v, double lo, double scale) {
  double q = (v - lo) * scale;
  q = q >= 0.0 ? q : 0.0;  // (also a NaN of an overflowed extent: the order only steers the pruning)
  q = q > 2097151.0 ? 2097151.0 : q;
  return (unsigned)q;
}

__global__ __launch_bounds__(kBlock) void k_eval_bbox(const void *xyz, int dtype, long long n,
                                                      unsigned long long *keys6) {
  unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0};
  for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
    for (int k = 0; k < 3; ++k) {
      const unsigned long long v = ord_key(load_coord(xyz, dtype, 3 * i + k));
      lo[k] = v < lo[k] ? v : lo[k];
      hi[k] = v > hi[k] ? v : hi[k];
    }
  for (int off = 32; off > 0; off >>= 1)
    for (int k = 0; k < 3; ++k) {
      const unsigned long long a = __shfl_xor(lo[k], off), b = __shfl_xor(hi[k], off);
      lo[k] = a < lo[k] ? a : lo[k];
      hi[k] = b > hi[k] ? b : hi[k];
    }
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 3; ++k) {
      atomicMin(keys6 + k, lo[k]);
      atomicMax(keys6 + 3 + k, hi[k]);
    }
}

struct Vec3Arg {
  double v[3];
};

__global__ __launch_bounds__(kBlock) void k_eval_morton(const void *xyz, int dtype, long long n, Vec3Arg lo,
                                                        Vec3Arg scale, unsigned long long *keys, unsigned *idx) {
  const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (i >= n) return;
  unsigned long long key = 0;
  for (int k = 0; k < 3; ++k) key |= spread21(quant21(load_coord(xyz, dtype, 3 * i + k), lo.v[k], scale.v[k])) << k;
  keys[i] = key;
  idx[i] = (unsigned)i;
}

__global__ __launch_bounds__(kBlock) void k_eval_gather(const void *xyz, int dtype, long long n, const unsigned *perm,
                                                        double *x, double *y, double *z) {
  const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (i >= n) return;
  const long long j = perm[i];
  x[i] = load_coord(xyz, dtype, 3 * j);
  y[i] = load_coord(xyz, dtype, 3 * j + 1);
  z[i] = load_coord(xyz, dtype, 3 * j + 2);
}

__global__ __launch_bounds__(kBlock) void k_eval_leaf_boxes(EvalTree T, double *box) {
  const long long b = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (b >= T.L.lvl_n[0]) return;
  const long long p0 = b * kEvalBucket;
  const long long p1 = p0 + kEvalBucket < T.L.n ? p0 + kEvalBucket : T.L.n;
  double lo[3] = {T.x[p0], T.y[p0], T.z[p0]}, hi[3] = {lo[0], lo[1], lo[2]};
  for (long long p = p0 + 1; p < p1; ++p) {
    const double v[3] = {T.x[p], T.y[p], T.z[p]};
    for (int k = 0; k < 3; ++k) {
      lo[k] = v[k] < lo[k] ? v[k] : lo[k];
      hi[k] = v[k] > hi[k] ? v[k] : hi[k];
    }
  }
  double *o = box + 6 * (T.L.lvl_off[0] + b);
  for (int k = 0; k < 3; ++k) {
    o[k] = lo[k];
    o[3 + k] = hi[k];
  }
}

__global__ __launch_bounds__(kBlock) void k_eval_level_boxes(EvalLevels L, int l, double *box) {
  const long long j = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (j >= L.lvl_n[l]) return;
  const long long c0 = j * kEvalFanout;
  const long long c1 = c0 + kEvalFanout < L.lvl_n[l - 1] ? c0 + kEvalFanout : L.lvl_n[l - 1];
  const double *c = box + 6 * (L.lvl_off[l - 1] + c0);
  double b[6] = {c[0], c[1], c[2], c[3], c[4], c[5]};
  for (long long i = 1; i < c1 - c0; ++i)
    for (int k = 0; k < 3; ++k) {
      b[k] = c[6 * i + k] < b[k] ? c[6 * i + k] : b[k];
      b[3 + k] = c[6 * i + 3 + k] > b[3 + k] ? c[6 * i + 3 + k] : b[3 + k];
    }
  double *o = box + 6 * (L.lvl_off[l] + j);
  for (int k = 0; k < 6; ++k) o[k] = b[k];
}

// query q's point, in the reference's grouping: start + (c * (end - start)) per component with c = (i + 0.5) * interval
// (ComputeInlierRatio, the seg functions) or i * interval (ComputeDistLine); start + ((length / (n - 1)) * i) *
// direction() (ComputeRecallLength)
__device__ inline void query_point(const EvalQuery &Q, long long q, double p[3]) {
  if (Q.mode == EV_Q_POINTS) {
    p[0] = Q.x[q * Q.stride];
    p[1] = Q.y[q * Q.stride];
    p[2] = Q.z[q * Q.stride];
    return;
  }
  const long long l = q / Q.n;
  const int i = (int)(q - l * Q.n);
  const EvalLine &L = Q.lines[l];
  if (Q.mode == EV_Q_REFLINE) {
    const double c = L.rint * (double)i;
    for (int k = 0; k < 3; ++k) p[k] = L.s[k] + c * L.d[k];
  } else {
    const double c = (Q.mode == EV_Q_CENTER ? (double)i + 0.5 : (double)i) * Q.interval;
    for (int k = 0; k < 3; ++k) p[k] = L.s[k] + c * (L.e[k] - L.s[k]);
  }
}

// sum of squared per-axis gaps, in the operation order of the point distance ((x + y) + z)
__device__ inline double box_bound2(const double *b, const double p[3]) {
  double g[3];
  for (int k = 0; k < 3; ++k) {
    const double a = b[k] - p[k], c = p[k] - b[3 + k];
    g[k] = a > 0.0 ? a : (c > 0.0 ? c : 0.0);
  }
  return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

__device__ inline double scan_bucket(const EvalTree &T, long long b, const double p[3], double best) {
  const long long p0 = b * kEvalBucket;
  const long long p1 = p0 + kEvalBucket < T.L.n ? p0 + kEvalBucket : T.L.n;
  for (long long j = p0; j < p1; ++j) {
    const double dx = p[0] - T.x[j], dy = p[1] - T.y[j], dz = p[2] - T.z[j];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    best = d2 < best ? d2 : best;
  }
  return best;
}

// Line3d::point_distance (base/linebase.cc:67-80), squared: the projection onto the segment, clamped at its ends
__device__ inline double seg_dist2(const EvalLine &L, const double p[3]) {
  const double ax = p[0] - L.s[0], ay = p[1] - L.s[1], az = p[2] - L.s[2];
  const double proj = (ax * L.d[0] + ay * L.d[1]) + az * L.d[2];
  double c[3];
  for (int k = 0; k < 3; ++k) c[k] = proj < 0.0 ? L.s[k] : (proj > L.len ? L.e[k] : L.s[k] + proj * L.d[k]);
  const double vx = p[0] - c[0], vy = p[1] - c[1], vz = p[2] - c[2];
  return (vx * vx + vy * vy) + vz * vz;
}

// RefLineEvaluator::DistPointLine (refline_evaluator.cc:58-66), squared: min(perp to the infinite line, both ends)
__device__ inline double refline_dist2(const EvalLine &L, const double p[3]) {
  const double ax = p[0] - L.s[0], ay = p[1] - L.s[1], az = p[2] - L.s[2];
  const double bx = p[0] - L.e[0], by = p[1] - L.e[1], bz = p[2] - L.e[2];
  const double ds2 = (ax * ax + ay * ay) + az * az;
  const double de2 = (bx * bx + by * by) + bz * bz;
  const double t = (ax * L.d[0] + ay * L.d[1]) + az * L.d[2];
  double perp = ds2 - t * t;
  perp = perp < 0.0 ? 0.0 : perp;            // std::max(perp, 0.0)
  const double ends = de2 < ds2 ? de2 : ds2;  // std::min(dist_start, dist_end)
  return ends < perp ? ends : perp;           // std::min(dist_perp, ...)
}

template <int FORM>
__global__ __launch_bounds__(kBlock) void k_eval_lines_min(EvalQuery Q, long long nq, const EvalLine *lines,
                                                           long long n_lines, double *out, const unsigned *scatter) {
  __shared__ EvalLine tile[kLineTile];
  const long long base = blockIdx.x * (long long)(kBlock * kPerLane) + threadIdx.x;
  double p[kPerLane][3], m2[kPerLane];
  for (int r = 0; r < kPerLane; ++r) {
    const long long q = base + r * kBlock;
    if (q < nq) query_point(Q, q, p[r]);
    else p[r][0] = p[r][1] = p[r][2] = 0.0;
    m2[r] = INFINITY;
  }
  for (long long t0 = 0; t0 < n_lines; t0 += kLineTile) {
    const int cnt = (int)(n_lines - t0 < kLineTile ? n_lines - t0 : kLineTile);
    __syncthreads();
    const double *src = reinterpret_cast<const double *>(lines + t0);
    double *dst = reinterpret_cast<double *>(tile);
    for (int k = threadIdx.x; k < cnt * 12; k += kBlock) dst[k] = src[k];
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const EvalLine &L = tile[j];
      for (int r = 0; r < kPerLane; ++r) {
        const double d2 = FORM == 0 ? seg_dist2(L, p[r]) : refline_dist2(L, p[r]);
        m2[r] = d2 < m2[r] ? d2 : m2[r];
      }
    }
  }
  for (int r = 0; r < kPerLane; ++r) {
    const long long q = base + r * kBlock;
    if (q >= nq) continue;
    // dist < min_dist from DBL_MAX: a minimum that stayed infinite leaves DBL_MAX (also for an empty line list)
    double d = m2[r] < INFINITY ? sqrt(m2[r]) : DBL_MAX;
    if (FORM == 1) d = d < kEvalEps ? 0.0 : d;  // DistPointLines returns 0 once the minimum drops below EPS
    out[scatter ? (long long)scatter[q] : q] = d;
  }
}

__global__ __launch_bounds__(kBlock) void k_eval_count(const double *dist, int n, const double *th, int n_th, int le,
                                                       int *counts) {
  __shared__ int c[kEvalMaxTh];
  for (int t = threadIdx.x; t < n_th; t += kBlock) c[t] = 0;
  __syncthreads();
  const double *d = dist + (long long)blockIdx.x * n;
  for (int i0 = 0; i0 < n; i0 += kBlock) {  // whole waves take part in every ballot
    const int i = i0 + threadIdx.x;
    const double v = i < n ? d[i] : 0.0;
    for (int t = 0; t < n_th; ++t) {
      const bool f = i < n && (le ? v <= th[t] : v < th[t]);
      const unsigned long long m = __ballot(f);
      if ((threadIdx.x & 63) == 0 && m) atomicAdd(&c[t], __popcll(m));
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < n_th; t += kBlock) counts[(long long)blockIdx.x * n_th + t] = c[t];
}

// ---- MeshEvaluator: point-to-triangle distances ----------------------------------------------------------

constexpr int kFaceTile = 256;  // brute force: faces staged in LDS per pass (72 B each)

__device__ inline double dot3(const double u[3], const double v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

__device__ inline double sqn_diff(const double p[3], const double q[3]) {
  const double r[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
  return dot3(r, r);
}

// the project rule of a face whose region-7 denominator is not > 0: the closest of the clamped projections onto
// AB, BC, CA, in that order, kept with <
__device__ inline double degenerate_dist2(const double a[3], const double b[3], const double c[3], const double p[3]) {
  const double *U[3] = {a, b, c}, *W[3] = {b, c, a};
  double m = INFINITY;
  for (int k = 0; k < 3; ++k) {
    double e[3], up[3], q[3];
    for (int i = 0; i < 3; ++i) {
      e[i] = W[k][i] - U[k][i];
      up[i] = p[i] - U[k][i];
    }
    const double ee = dot3(e, e);
    double t = ee > 0.0 ? dot3(up, e) / ee : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    for (int i = 0; i < 3; ++i) q[i] = U[k][i] + t * e[i];
    const double d = sqn_diff(p, q);
    m = d < m ? d : m;
  }
  return m;
}

// Ericson's ClosestPtPointTriangle (Real-Time Collision Detection §5.1.5), squared distance, in the operation order of
// the first region that matches decides q
__device__ inline double tri_dist2(const double a[3], const double b[3], const double c[3], const double p[3]) {
  double ab[3], ac[3], ap[3], bp[3], cp[3], q[3];
  for (int i = 0; i < 3; ++i) {
    ab[i] = b[i] - a[i];
    ac[i] = c[i] - a[i];
    ap[i] = p[i] - a[i];
  }
  const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
  if (d1 <= 0.0 && d2 <= 0.0) return sqn_diff(p, a);  // 1: vertex a
  for (int i = 0; i < 3; ++i) bp[i] = p[i] - b[i];
  const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
  if (d3 >= 0.0 && d4 <= d3) return sqn_diff(p, b);  // 2: vertex b
  const double vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {  // 3: edge ab
    const double v = d1 / (d1 - d3);
    for (int i = 0; i < 3; ++i) q[i] = a[i] + v * ab[i];
    return sqn_diff(p, q);
  }
  for (int i = 0; i < 3; ++i) cp[i] = p[i] - c[i];
  const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  if (d6 >= 0.0 && d5 <= d6) return sqn_diff(p, c);  // 4: vertex c
  const double vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {  // 5: edge ac
    const double w = d2 / (d2 - d6);
    for (int i = 0; i < 3; ++i) q[i] = a[i] + w * ac[i];
    return sqn_diff(p, q);
  }
  const double va = d3 * d6 - d5 * d4;
  const double e43 = d4 - d3, e56 = d5 - d6;
  if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {  // 6: edge bc
    const double w = e43 / (e43 + e56);
    for (int i = 0; i < 3; ++i) q[i] = b[i] + w * (c[i] - b[i]);
    return sqn_diff(p, q);
  }
  const double s = (va + vb) + vc;
  if (!(s > 0.0)) return degenerate_dist2(a, b, c, p);
  const double denom = 1.0 / s;  // 7: the interior
  const double v = vb * denom, w = vc * denom;
  for (int i = 0; i < 3; ++i) q[i] = (a[i] + ab[i] * v) + ac[i] * w;
  return sqn_diff(p, q);
}

__device__ inline void load_face(const MeshTree &T, long long f, double a[3], double b[3], double c[3]) {
  for (int i = 0; i < 3; ++i) {
    a[i] = T.v[i][f];
    b[i] = T.v[3 + i][f];
    c[i] = T.v[6 + i][f];
  }
}

__global__ __launch_bounds__(kBlock) void k_mesh_centroids(const double *V, const long long *F, long long nf,
                                                           double *cen) {
  const long long f = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (f >= nf) return;
  const long long i0 = F[3 * f], i1 = F[3 * f + 1], i2 = F[3 * f + 2];
  for (int k = 0; k < 3; ++k) cen[3 * f + k] = ((V[3 * i0 + k] + V[3 * i1 + k]) + V[3 * i2 + k]) / 3.0;
}

struct FaceOut {
  double *p[9];
};

__global__ __launch_bounds__(kBlock) void k_mesh_gather(const double *V, const long long *F, long long nf,
                                                        const unsigned *perm, FaceOut out) {
  const long long f = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (f >= nf) return;
  const long long g = perm[f];
  for (int j = 0; j < 3; ++j) {
    const long long vi = F[3 * g + j];
    for (int k = 0; k < 3; ++k) out.p[3 * j + k][f] = V[3 * vi + k];
  }
}

// a bucket's box over all its vertices, widened per axis by 2 * 2^-48 * max(|lo|, |hi|) (+ a subnormal floor): the few
// roundings of regions 1-6 and of the degenerate rule keep q inside it.  eta: the largest region-7 factor of its faces,
// 2^-40 E^3 / S (E^2 the longest squared edge, S = |ab|^2 |ac|^2 - (ab.ac)^2), +inf when S <= 2^-30 E^4
__global__ __launch_bounds__(kBlock) void k_mesh_leaf_boxes(MeshTree T, double *box, double *eta) {
  const long long b = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (b >= T.L.lvl_n[0]) return;
  const long long f0 = b * T.bucket;
  const long long f1 = f0 + T.bucket < T.L.n ? f0 + T.bucket : T.L.n;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, et = 0.0;
  for (long long f = f0; f < f1; ++f) {
    double v[3][3];
    load_face(T, f, v[0], v[1], v[2]);
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k) {
        lo[k] = v[j][k] < lo[k] ? v[j][k] : lo[k];
        hi[k] = v[j][k] > hi[k] ? v[j][k] : hi[k];
      }
    double ab[3], ac[3], bc[3];
    for (int k = 0; k < 3; ++k) {
      ab[k] = v[1][k] - v[0][k];
      ac[k] = v[2][k] - v[0][k];
      bc[k] = v[2][k] - v[1][k];
    }
    const double l1 = dot3(ab, ab), l2 = dot3(ac, ac), l3 = dot3(bc, bc), x = dot3(ab, ac);
    double e2 = l1 > l2 ? l1 : l2;
    e2 = l3 > e2 ? l3 : e2;
    if (e2 > 0.0) {  // (three equal vertices: region 1 always, q = a)
      const double S = l1 * l2 - x * x;
      const double h = S > 0x1p-30 * (e2 * e2) ? 0x1p-40 * (e2 * sqrt(e2)) / S : INFINITY;
      et = h > et ? h : et;
    }
  }
  double *o = box + 6 * (T.L.lvl_off[0] + b);
  for (int k = 0; k < 3; ++k) {
    const double m = 0x1p-48 * fmax(fabs(lo[k]), fabs(hi[k])) + 0x1p-1060;
    o[k] = lo[k] - 2.0 * m;
    o[3 + k] = hi[k] + 2.0 * m;
  }
  eta[T.L.lvl_off[0] + b] = et;
}

__global__ __launch_bounds__(kBlock) void k_mesh_level_eta(MeshTree T, int l, double *eta) {
  const long long j = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (j >= T.L.lvl_n[l]) return;
  const long long c0 = j * kEvalFanout;
  const long long c1 = c0 + kEvalFanout < T.L.lvl_n[l - 1] ? c0 + kEvalFanout : T.L.lvl_n[l - 1];
  double m = 0.0;
  for (long long c = c0; c < c1; ++c) {
    const double e = eta[T.L.lvl_off[l - 1] + c];
    m = e > m ? e : m;
  }
  eta[T.L.lvl_off[l] + j] = m;
}

// a lower bound of the computed squared distance of p to every face below a node: the per-axis gap to the (widened)
// box, reduced by the region-7 slack X = eta * Rfar^2 (Rfar: the farthest point of the box) and by 2^-50 of itself,
// squared and summed in the distance's order.  A NaN slack (inf * 0) leaves no gap.
__device__ inline double mesh_bound2(const double *b, double eta, const double p[3]) {
  double g[3], r[3];
  for (int k = 0; k < 3; ++k) {
    const double lo = b[k] - p[k], hi = p[k] - b[3 + k];
    g[k] = lo > 0.0 ? lo : (hi > 0.0 ? hi : 0.0);
    const double al = fabs(lo), ah = fabs(hi);
    r[k] = al > ah ? al : ah;
  }
  const double X = (eta * ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])) * (1.0 + 0x1p-40);
  for (int k = 0; k < 3; ++k) {
    const double h = g[k] - (X + g[k] * 0x1p-50);
    g[k] = h > 0.0 ? h : 0.0;
  }
  return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

__device__ inline double scan_faces(const MeshTree &T, long long b, const double p[3], double best) {
  const long long f0 = b * T.bucket;
  const long long f1 = f0 + T.bucket < T.L.n ? f0 + T.bucket : T.L.n;
  for (long long f = f0; f < f1; ++f) {
    double a[3], bb[3], c[3];
    load_face(T, f, a, bb, c);
    const double d2 = tri_dist2(a, bb, c, p);
    best = d2 < best ? d2 : best;
  }
  return best;
}

}  // namespace

// what the walk asks of the two indexes (lt_eval.h)
__device__ inline double EvalTree::bound2(long long node, const double p[3]) const {
  return box_bound2(box + 6 * node, p);
}
__device__ inline double EvalTree::scan(long long b, const double p[3], double best) const {
  return scan_bucket(*this, b, p, best);
}
__device__ inline double MeshTree::bound2(long long node, const double p[3]) const {
  return mesh_bound2(box + 6 * node, eta[node], p);
}
__device__ inline double MeshTree::scan(long long b, const double p[3], double best) const {
  return scan_faces(*this, b, p, best);
}

namespace {

// exact minimum squared distance of p to the members of an index: a greedy descent to one bucket for a first bound,
// then a depth-first walk of the implicit hierarchy (no stack: the next node follows from (level, index) alone) that
// skips subtrees whose bound exceeds the best.  Each node is visited at most once: the walk is bounded by L.total.
template <class Index>
__device__ inline double nearest2(const Index &T, const double p[3]) {
  const EvalLevels &L = T.L;
  long long j = 0;
  for (int l = L.top; l > 0; --l) {
    const long long c0 = j * kEvalFanout;
    const long long c1 = c0 + kEvalFanout < L.lvl_n[l - 1] ? c0 + kEvalFanout : L.lvl_n[l - 1];
    long long bj = c0;
    double bb = INFINITY;
    for (long long c = c0; c < c1; ++c) {
      const double v = T.bound2(L.lvl_off[l - 1] + c, p);
      if (v < bb) { bb = v; bj = c; }
    }
    j = bj;
  }
  const long long first = j;
  double best = T.scan(first, p, INFINITY);
  int l = L.top;
  j = 0;
  for (long long it = 0; it < L.total; ++it) {
    const double lb = T.bound2(L.lvl_off[l] + j, p);
    if (!(lb > best)) {
      if (l > 0) {  // descend to the first child
        --l;
        j *= kEvalFanout;
        continue;
      }
      if (j != first) best = T.scan(j, p, best);
    }
    // next: the following sibling, else up to the parent's following sibling
    bool done = true;
    for (int u = 0; u < kEvalMaxLevels && l < L.top; ++u) {
      if ((j + 1) % kEvalFanout != 0 && j + 1 < L.lvl_n[l]) {
        ++j;
        done = false;
        break;
      }
      ++l;
      j /= kEvalFanout;
    }
    if (done) break;
  }
  return best;
}

__global__ __launch_bounds__(kBlock) void k_eval_nearest(EvalTree T, EvalQuery Q, long long nq, double *dist) {
  const long long q = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (q >= nq) return;
  double p[3];
  query_point(Q, q, p);
  dist[q] = sqrt(nearest2(T, p));
}

__global__ __launch_bounds__(kBlock) void k_mesh_nearest(MeshTree T, EvalQuery Q, long long nq, double *dist) {
  const long long q = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (q >= nq) return;
  double p[3];
  query_point(Q, q, p);
  dist[q] = sqrt(nearest2(T, p));
}

// the walk's yardstick: every face, tiles of kFaceTile faces staged in LDS (SoA), kPerLane queries per lane
__global__ __launch_bounds__(kBlock) void k_mesh_brute(MeshTree T, EvalQuery Q, long long nq, double *dist) {
  __shared__ double tile[9][kFaceTile];
  const long long base = blockIdx.x * (long long)(kBlock * kPerLane) + threadIdx.x;
  double p[kPerLane][3], m2[kPerLane];
  for (int r = 0; r < kPerLane; ++r) {
    const long long q = base + r * kBlock;
    if (q < nq) query_point(Q, q, p[r]);
    else p[r][0] = p[r][1] = p[r][2] = 0.0;
    m2[r] = INFINITY;
  }
  for (long long t0 = 0; t0 < T.L.n; t0 += kFaceTile) {
    const int cnt = (int)(T.L.n - t0 < kFaceTile ? T.L.n - t0 : kFaceTile);
    __syncthreads();
    for (int k = threadIdx.x; k < 9 * kFaceTile; k += kBlock) {
      const int a = k / kFaceTile, f = k - a * kFaceTile;
      if (f < cnt) tile[a][f] = T.v[a][t0 + f];
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const double a[3] = {tile[0][j], tile[1][j], tile[2][j]};
      const double b[3] = {tile[3][j], tile[4][j], tile[5][j]};
      const double c[3] = {tile[6][j], tile[7][j], tile[8][j]};
      for (int r = 0; r < kPerLane; ++r) {
        const double d2 = tri_dist2(a, b, c, p[r]);
        m2[r] = d2 < m2[r] ? d2 : m2[r];
      }
    }
  }
  for (int r = 0; r < kPerLane; ++r) {
    const long long q = base + r * kBlock;
    if (q < nq) dist[q] = sqrt(m2[r]);
  }
}

}  // namespace

void launch_eval_bbox(hipStream_t st, const void *xyz, int dtype, long long n, unsigned long long *keys6) {
  const unsigned g = nblk(n, kBlock) < 1024u ? nblk(n, kBlock) : 1024u;
  hipLaunchKernelGGL(k_eval_bbox, dim3(g ? g : 1), dim3(kBlock), 0, st, xyz, dtype, n, keys6);
}

void launch_eval_morton(hipStream_t st, const void *xyz, int dtype, long long n, const double lo[3],
                        const double scale[3], unsigned long long *keys, unsigned *idx) {
  Vec3Arg a{{lo[0], lo[1], lo[2]}}, b{{scale[0], scale[1], scale[2]}};
  hipLaunchKernelGGL(k_eval_morton, dim3(nblk(n, kBlock)), dim3(kBlock), 0, st, xyz, dtype, n, a, b, keys, idx);
}

size_t eval_sort_temp_bytes(long long n) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                  (unsigned *)nullptr, (unsigned *)nullptr, (size_t)n, 0, 63, (hipStream_t)0);
  return bytes;
}

int launch_eval_sort(hipStream_t st, void *temp, size_t temp_bytes, long long n, const unsigned long long *keys_in,
                     unsigned long long *keys_out, const unsigned *idx_in, unsigned *idx_out) {
  if (n <= 0) return 0;
  return (int)rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, idx_in, idx_out, (size_t)n, 0, 63, st);
}

void launch_eval_gather(hipStream_t st, const void *xyz, int dtype, long long n, const unsigned *perm, double *x,
                        double *y, double *z) {
  hipLaunchKernelGGL(k_eval_gather, dim3(nblk(n, kBlock)), dim3(kBlock), 0, st, xyz, dtype, n, perm, x, y, z);
}

void launch_eval_boxes(hipStream_t st, const EvalTree &T, double *box) {
  hipLaunchKernelGGL(k_eval_leaf_boxes, dim3(nblk(T.L.lvl_n[0], kBlock)), dim3(kBlock), 0, st, T, box);
  for (int l = 1; l <= T.L.top; ++l)
    hipLaunchKernelGGL(k_eval_level_boxes, dim3(nblk(T.L.lvl_n[l], kBlock)), dim3(kBlock), 0, st, T.L, l, box);
}

void launch_eval_nearest(hipStream_t st, const EvalTree &T, const EvalQuery &Q, long long nq, double *dist) {
  if (nq <= 0) return;
  hipLaunchKernelGGL(k_eval_nearest, dim3(nblk(nq, kBlock)), dim3(kBlock), 0, st, T, Q, nq, dist);
}

void launch_eval_lines_min(hipStream_t st, int form, const EvalQuery &Q, long long nq, const EvalLine *lines,
                           long long n_lines, double *out, const unsigned *scatter) {
  if (nq <= 0) return;
  const dim3 g(nblk(nq, kBlock * kPerLane));
  if (form == 0)
    hipLaunchKernelGGL(k_eval_lines_min<0>, g, dim3(kBlock), 0, st, Q, nq, lines, n_lines, out, scatter);
  else
    hipLaunchKernelGGL(k_eval_lines_min<1>, g, dim3(kBlock), 0, st, Q, nq, lines, n_lines, out, scatter);
}

void launch_eval_count(hipStream_t st, const double *dist, long long n_lines, int n, const double *th, int n_th, int le,
                       int *counts) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_eval_count, dim3((unsigned)n_lines), dim3(kBlock), 0, st, dist, n, th, n_th, le, counts);
}

void launch_mesh_centroids(hipStream_t st, const double *V, const long long *F, long long nf, double *cen) {
  hipLaunchKernelGGL(k_mesh_centroids, dim3(nblk(nf, kBlock)), dim3(kBlock), 0, st, V, F, nf, cen);
}

void launch_mesh_gather(hipStream_t st, const double *V, const long long *F, long long nf, const unsigned *perm,
                        double *const out[9]) {
  FaceOut o;
  for (int k = 0; k < 9; ++k) o.p[k] = out[k];
  hipLaunchKernelGGL(k_mesh_gather, dim3(nblk(nf, kBlock)), dim3(kBlock), 0, st, V, F, nf, perm, o);
}

void launch_mesh_boxes(hipStream_t st, const MeshTree &T, double *box, double *eta) {
  hipLaunchKernelGGL(k_mesh_leaf_boxes, dim3(nblk(T.L.lvl_n[0], kBlock)), dim3(kBlock), 0, st, T, box, eta);
  for (int l = 1; l <= T.L.top; ++l) {
    hipLaunchKernelGGL(k_eval_level_boxes, dim3(nblk(T.L.lvl_n[l], kBlock)), dim3(kBlock), 0, st, T.L, l, box);
    hipLaunchKernelGGL(k_mesh_level_eta, dim3(nblk(T.L.lvl_n[l], kBlock)), dim3(kBlock), 0, st, T, l, eta);
  }
}

void launch_mesh_nearest(hipStream_t st, const MeshTree &T, const EvalQuery &Q, long long nq, int brute, double *dist) {
  if (nq <= 0) return;
  if (brute)
    hipLaunchKernelGGL(k_mesh_brute, dim3(nblk(nq, kBlock * kPerLane)), dim3(kBlock), 0, st, T, Q, nq, dist);
  else
    hipLaunchKernelGGL(k_mesh_nearest, dim3(nblk(nq, kBlock)), dim3(kBlock), 0, st, T, Q, nq, dist);
}

}  // namespace lt
