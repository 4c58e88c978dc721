// lt_kernels_eval.hip -- device side of limap.evaluation (evaluation/point_cloud_evaluator.cc, base_evaluator.cc,
// refline_evaluator.cc of the reference): the point index (Morton order, buckets, an implicit AABB hierarchy), exact
// nearest-point queries on it, and the brute-force minima of point-to-segment distances.  DESIGN §14.
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
  if (b >= T.lvl_n[0]) return;
  const long long p0 = b * kEvalBucket;
  const long long p1 = p0 + kEvalBucket < T.n ? p0 + kEvalBucket : T.n;
  double lo[3] = {T.x[p0], T.y[p0], T.z[p0]}, hi[3] = {lo[0], lo[1], lo[2]};
  for (long long p = p0 + 1; p < p1; ++p) {
    const double v[3] = {T.x[p], T.y[p], T.z[p]};
    for (int k = 0; k < 3; ++k) {
      lo[k] = v[k] < lo[k] ? v[k] : lo[k];
      hi[k] = v[k] > hi[k] ? v[k] : hi[k];
    }
  }
  double *o = box + 6 * (T.lvl_off[0] + b);
  for (int k = 0; k < 3; ++k) {
    o[k] = lo[k];
    o[3 + k] = hi[k];
  }
}

__global__ __launch_bounds__(kBlock) void k_eval_level_boxes(EvalTree T, int l, double *box) {
  const long long j = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (j >= T.lvl_n[l]) return;
  const long long c0 = j * kEvalFanout;
  const long long c1 = c0 + kEvalFanout < T.lvl_n[l - 1] ? c0 + kEvalFanout : T.lvl_n[l - 1];
  const double *c = box + 6 * (T.lvl_off[l - 1] + c0);
  double b[6] = {c[0], c[1], c[2], c[3], c[4], c[5]};
  for (long long i = 1; i < c1 - c0; ++i)
    for (int k = 0; k < 3; ++k) {
      b[k] = c[6 * i + k] < b[k] ? c[6 * i + k] : b[k];
      b[3 + k] = c[6 * i + 3 + k] > b[3 + k] ? c[6 * i + 3 + k] : b[3 + k];
    }
  double *o = box + 6 * (T.lvl_off[l] + j);
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
  const long long p1 = p0 + kEvalBucket < T.n ? p0 + kEvalBucket : T.n;
  for (long long j = p0; j < p1; ++j) {
    const double dx = p[0] - T.x[j], dy = p[1] - T.y[j], dz = p[2] - T.z[j];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    best = d2 < best ? d2 : best;
  }
  return best;
}

// exact minimum squared distance of p to the cloud: a greedy descent to one bucket for a first bound, then a
// depth-first walk of the implicit hierarchy (no stack: the next node follows from (level, index) alone) that skips
// subtrees whose bound exceeds the best.  Each node is visited at most once: the walk is bounded by T.total.
__device__ double nearest2(const EvalTree &T, const double p[3]) {
  long long j = 0;
  for (int l = T.top; l > 0; --l) {
    const long long c0 = j * kEvalFanout;
    const long long c1 = c0 + kEvalFanout < T.lvl_n[l - 1] ? c0 + kEvalFanout : T.lvl_n[l - 1];
    long long bj = c0;
    double bb = INFINITY;
    for (long long c = c0; c < c1; ++c) {
      const double v = box_bound2(T.box + 6 * (T.lvl_off[l - 1] + c), p);
      if (v < bb) { bb = v; bj = c; }
    }
    j = bj;
  }
  const long long first = j;
  double best = scan_bucket(T, first, p, INFINITY);
  int l = T.top;
  j = 0;
  for (long long it = 0; it < T.total; ++it) {
    const double lb = box_bound2(T.box + 6 * (T.lvl_off[l] + j), p);
    if (!(lb > best)) {
      if (l > 0) {  // descend to the first child
        --l;
        j *= kEvalFanout;
        continue;
      }
      if (j != first) best = scan_bucket(T, j, p, best);
    }
    // next: the following sibling, else up to the parent's following sibling
    bool done = true;
    for (int u = 0; u < kEvalMaxLevels && l < T.top; ++u) {
      if ((j + 1) % kEvalFanout != 0 && j + 1 < T.lvl_n[l]) {
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
  hipLaunchKernelGGL(k_eval_leaf_boxes, dim3(nblk(T.lvl_n[0], kBlock)), dim3(kBlock), 0, st, T, box);
  for (int l = 1; l <= T.top; ++l)
    hipLaunchKernelGGL(k_eval_level_boxes, dim3(nblk(T.lvl_n[l], kBlock)), dim3(kBlock), 0, st, T, l, box);
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

}  // namespace lt
