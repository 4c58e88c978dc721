// lt_kernels_bpt.hip -- device side of the 2D point-line bipartites (limap.structures.PL_Bipartite2d,
// structures/pl_bipartite.cc of the reference).  DESIGN §16.
//   k_bpt_prep         per line: direction, length, homogeneous coordinates (Line2d::direction / length / coords)
//   k_bpt_assoc        add_keypoint (:56-67): every keypoint against every line of its image, Line2d::point_distance
//   k_bpt_intersect    intersect() (:166-204) over the upper triangle of an image's line pairs, in the order of :112-124
//   k_bpt_candidates   the junction candidates (endpoints, then intersections) and their grid cells
//   k_bpt_close_pairs  the candidate pairs that pass the distance test of :135-137, found through a uniform grid
//   k_bpt_nearest      KDTree::point_distance (util/kd_tree.h:96-98) of the merged junctions, as the exact minimum
// Every kernel that compacts does it in two passes (count, then fill at the host's prefix sums), so the layout of its
// output is a function of the inputs alone: no atomic decides an order.  FP64 throughout, -ffp-contract=off.

#include "lt_bpt.h"
#include "lt_geom.h"

#include <cfloat>

#include <rocprim/device/device_radix_sort.hpp>

namespace lt {

namespace {

__global__ void __launch_bounds__(kBptBlock) k_bpt_prep(const double *__restrict__ lines4, long long n,
                                                        BptLine *__restrict__ out) {
  const long long k = (long long)blockIdx.x * kBptBlock + threadIdx.x;
  if (k >= n) return;
  L2 l{mk2(lines4[4 * k], lines4[4 * k + 1]), mk2(lines4[4 * k + 2], lines4[4 * k + 3])};
  const d2 d = dir(l);
  const d3 c = unit(cross(mk3(l.s.x, l.s.y, 1.0), mk3(l.e.x, l.e.y, 1.0)));
  BptLine r;
  r.sx = l.s.x; r.sy = l.s.y; r.ex = l.e.x; r.ey = l.e.y;
  r.dx = d.x; r.dy = d.y; r.len = len(l);
  r.c0 = c.x; r.c1 = c.y; r.c2 = c.z;
  out[k] = r;
}

// Line2d::point_distance (linebase.cc:20-33) with direction() and length() hoisted
__device__ __forceinline__ double point_line_dist(double px, double py, double sx, double sy, double ex, double ey,
                                                  double dx, double dy, double ln) {
  const double projection = (px - sx) * dx + (py - sy) * dy;
  double qx, qy;
  if (projection < 0) {
    qx = sx; qy = sy;
  } else if (projection > ln) {
    qx = ex; qy = ey;
  } else {
    qx = sx + projection * dx; qy = sy + projection * dy;
  }
  const double ux = px - qx, uy = py - qy;
  return sqrt(ux * ux + uy * uy);
}

template <int FILL>
__global__ void __launch_bounds__(kBptBlock) k_bpt_assoc(const BptBlock *__restrict__ blk,
                                                         const long long *__restrict__ line_off,
                                                         const BptLine *__restrict__ lines,
                                                         const double *__restrict__ pts, double th,
                                                         int *__restrict__ cnt, const long long *__restrict__ off,
                                                         int *__restrict__ edge) {
  __shared__ double s_l[7][kBptLineTile];
  const BptBlock b = blk[blockIdx.x];
  const long long l0 = line_off[b.img], l1 = line_off[b.img + 1];
  const long long p = b.begin + threadIdx.x;
  const bool live = p < b.end;
  double px = 0.0, py = 0.0;
  if (live) {
    px = pts[2 * p];
    py = pts[2 * p + 1];
  }
  int n = 0;
  int *dst = (FILL && live) ? edge + off[p] : nullptr;
  for (long long t0 = l0; t0 < l1; t0 += kBptLineTile) {
    const int m = (int)(l1 - t0 < kBptLineTile ? l1 - t0 : kBptLineTile);
    __syncthreads();
    for (int k = threadIdx.x; k < m; k += kBptBlock) {
      const BptLine L = lines[t0 + k];
      s_l[0][k] = L.sx; s_l[1][k] = L.sy; s_l[2][k] = L.ex; s_l[3][k] = L.ey;
      s_l[4][k] = L.dx; s_l[5][k] = L.dy; s_l[6][k] = L.len;
    }
    __syncthreads();
    if (live) {
      for (int k = 0; k < m; ++k) {
        const double dist =
            point_line_dist(px, py, s_l[0][k], s_l[1][k], s_l[2][k], s_l[3][k], s_l[4][k], s_l[5][k], s_l[6][k]);
        if (!(dist > th)) {  // add_keypoint: `if (dist > threshold_keypoints) continue;`
          if (FILL) dst[n] = (int)(t0 - l0) + k;
          ++n;
        }
      }
    }
  }
  if (!FILL && live) cnt[p] = n;
}

// PL_Bipartite2d::intersect (pl_bipartite.cc:166-204)
__device__ __forceinline__ bool intersect(const BptLine &a, const BptLine &b, double th, double *ox, double *oy) {
  if (bpt_norm2(a.sx - b.sx, a.sy - b.sy) <= th) { *ox = (a.sx + b.sx) / 2.0; *oy = (a.sy + b.sy) / 2.0; return true; }
  if (bpt_norm2(a.ex - b.sx, a.ey - b.sy) <= th) { *ox = (a.ex + b.sx) / 2.0; *oy = (a.ey + b.sy) / 2.0; return true; }
  if (bpt_norm2(a.sx - b.ex, a.sy - b.ey) <= th) { *ox = (a.sx + b.ex) / 2.0; *oy = (a.sy + b.ey) / 2.0; return true; }
  if (bpt_norm2(a.ex - b.ex, a.ey - b.ey) <= th) { *ox = (a.ex + b.ex) / 2.0; *oy = (a.ey + b.ey) / 2.0; return true; }
  const d3 h = unit(cross(mk3(a.c0, a.c1, a.c2), mk3(b.c0, b.c1, b.c2)));
  const double px = h.x / (h.z + kEps), py = h.y / (h.z + kEps);
  const double proj1 = (px - a.sx) * a.dx + (py - a.sy) * a.dy;
  double error1 = 0.0;
  if (proj1 < 0.0) error1 = -proj1;
  if (proj1 > a.len) error1 = proj1 - a.len;
  const double proj2 = (px - b.sx) * b.dx + (py - b.sy) * b.dy;
  double error2 = 0.0;
  if (proj2 < 0.0) error2 = -proj2;
  if (proj2 > b.len) error2 = proj2 - b.len;
  if (error1 + error2 > th) return false;
  *ox = px; *oy = py;
  return true;
}

// the exclusive rank of this lane's flag among the block's flags in thread order, and the block's total
__device__ __forceinline__ int block_rank(bool flag, int *s_wave, int *total) {
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // s_wave of the previous round has been read
  if (lane == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < kBptBlock / 64; ++w) {
    const int c = s_wave[w];
    if (w < wave) base += c;
    tot += c;
  }
  *total = tot;
  return base + __popcll(m & ((1ull << lane) - 1ull));
}

template <int FILL>
__global__ void __launch_bounds__(kBptBlock) k_bpt_intersect(const int *__restrict__ row_img,
                                                             const long long *__restrict__ line_off,
                                                             const BptLine *__restrict__ lines, double th,
                                                             int *__restrict__ cnt, const long long *__restrict__ off,
                                                             BptInter *__restrict__ out, int *__restrict__ flag) {
  __shared__ int s_wave[kBptBlock / 64];
  const long long row = blockIdx.x;
  const int img = row_img[row];
  const long long l0 = line_off[img], l1 = line_off[img + 1];
  const BptLine a = lines[row];
  const int i = (int)(row - l0), M = (int)(l1 - l0);
  long long pos = FILL ? off[row] : 0;
  int n = 0;
  for (int j0 = i + 1; j0 < M; j0 += kBptBlock) {  // uniform trip count: every lane reaches the barriers
    const int j = j0 + threadIdx.x;
    double x = 0.0, y = 0.0;
    bool hit = false;
    if (j < M) hit = intersect(a, lines[l0 + j], th, &x, &y);
    int tot;
    const int r = block_rank(hit, s_wave, &tot);
    if (FILL && hit) {
      if (!(isfinite(x) && isfinite(y))) *flag = 1;
      out[pos + r] = BptInter{x, y, i, j};
    }
    pos += tot;
    n += tot;
  }
  if (!FILL && threadIdx.x == 0) cnt[row] = n;
}

__device__ __forceinline__ int image_of(const long long *off, int n, long long k) {  // off[img] <= k < off[img + 1]
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= k) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kBptBlock) k_bpt_candidates(int n_img, long long n_cand,
                                                              const long long *__restrict__ cand_off,
                                                              const long long *__restrict__ line_off,
                                                              const long long *__restrict__ inter_off,
                                                              const BptLine *__restrict__ lines,
                                                              const BptInter *__restrict__ inter,
                                                              const BptGrid *__restrict__ grid,
                                                              double *__restrict__ cand_xy,
                                                              unsigned long long *__restrict__ keys,
                                                              unsigned *__restrict__ idx) {
  const long long c = (long long)blockIdx.x * kBptBlock + threadIdx.x;
  if (c >= n_cand) return;
  const int img = image_of(cand_off, n_img, c);
  const long long k = c - cand_off[img];
  const long long M = line_off[img + 1] - line_off[img];
  double x, y;
  if (k < 2 * M) {
    const BptLine &L = lines[line_off[img] + (k >> 1)];
    x = (k & 1) ? L.ex : L.sx;
    y = (k & 1) ? L.ey : L.sy;
  } else {
    const BptInter &I = inter[inter_off[img] + (k - 2 * M)];
    x = I.x; y = I.y;
  }
  cand_xy[2 * c] = x;
  cand_xy[2 * c + 1] = y;
  const BptGrid g = grid[img];
  keys[c] = bpt_key_of(img, x, y, g);
  idx[c] = (unsigned)c;
}

// one lane per candidate (in cell order, so that the lanes of a wave read the same neighbourhood)
template <int FILL>
__global__ void __launch_bounds__(kBptBlock) k_bpt_close_pairs(long long n_cand,
                                                               const unsigned long long *__restrict__ keys,
                                                               const unsigned *__restrict__ idx,
                                                               const double *__restrict__ cand_xy, double th,
                                                               int *__restrict__ cnt,
                                                               const long long *__restrict__ off,
                                                               unsigned long long *__restrict__ out) {
  const long long s = (long long)blockIdx.x * kBptBlock + threadIdx.x;
  if (s >= n_cand) return;
  const unsigned c = idx[s];
  const int n = bpt_close_pairs_of(n_cand, keys, idx, cand_xy, th, s, FILL ? out + off[c] : nullptr);
  if (!FILL) cnt[c] = n;
}

__global__ void __launch_bounds__(kBptBlock) k_bpt_nearest(const BptBlock *__restrict__ blk,
                                                           const long long *__restrict__ kp_off,
                                                           const double *__restrict__ kps,
                                                           const double *__restrict__ junc_xy,
                                                           double *__restrict__ dist) {
  __shared__ double s_x[kBptPointTile], s_y[kBptPointTile];
  const BptBlock b = blk[blockIdx.x];
  const long long k0 = kp_off[b.img], k1 = kp_off[b.img + 1];
  const long long q = b.begin + threadIdx.x;
  const bool live = q < b.end;
  double x = 0.0, y = 0.0;
  if (live) {
    x = junc_xy[2 * q];
    y = junc_xy[2 * q + 1];
  }
  double best = DBL_MAX;  // squared: nanoflann's L2_Simple metric, (dx*dx + dy*dy) + dz*dz with dz = 0
  for (long long t0 = k0; t0 < k1; t0 += kBptPointTile) {
    const int m = (int)(k1 - t0 < kBptPointTile ? k1 - t0 : kBptPointTile);
    __syncthreads();
    for (int k = threadIdx.x; k < m; k += kBptBlock) {
      s_x[k] = kps[2 * (t0 + k)];
      s_y[k] = kps[2 * (t0 + k) + 1];
    }
    __syncthreads();
    if (live)
      for (int k = 0; k < m; ++k) {
        const double ux = x - s_x[k], uy = y - s_y[k];
        const double d2v = (ux * ux + uy * uy) + 0.0 * 0.0;
        best = d2v < best ? d2v : best;
      }
  }
  // (query_pt - query_nearest(query_pt)).norm(): the square root of the smallest squared distance
  if (live) dist[q] = k1 > k0 ? sqrt(best) : DBL_MAX;
}

inline int grid_of(long long n) { return (int)((n + kBptBlock - 1) / kBptBlock); }

}  // namespace

void launch_bpt_prep(hipStream_t st, const double *lines4, long long n_lines, BptLine *out) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_bpt_prep, dim3(grid_of(n_lines)), dim3(kBptBlock), 0, st, lines4, n_lines, out);
}

void launch_bpt_assoc(hipStream_t st, int fill, const BptBlock *blk, int n_blk, const long long *line_off,
                      const BptLine *lines, const double *pts, double th, int *cnt, const long long *off, int *edge) {
  if (n_blk <= 0) return;
  if (fill)
    hipLaunchKernelGGL(k_bpt_assoc<1>, dim3(n_blk), dim3(kBptBlock), 0, st, blk, line_off, lines, pts, th, cnt, off,
                       edge);
  else
    hipLaunchKernelGGL(k_bpt_assoc<0>, dim3(n_blk), dim3(kBptBlock), 0, st, blk, line_off, lines, pts, th, cnt, off,
                       edge);
}

void launch_bpt_intersect(hipStream_t st, int fill, long long n_rows, const int *row_img, const long long *line_off,
                          const BptLine *lines, double th, int *cnt, const long long *off, BptInter *out, int *flag) {
  if (n_rows <= 0) return;
  if (fill)
    hipLaunchKernelGGL(k_bpt_intersect<1>, dim3((unsigned)n_rows), dim3(kBptBlock), 0, st, row_img, line_off, lines,
                       th, cnt, off, out, flag);
  else
    hipLaunchKernelGGL(k_bpt_intersect<0>, dim3((unsigned)n_rows), dim3(kBptBlock), 0, st, row_img, line_off, lines,
                       th, cnt, off, out, flag);
}

void launch_bpt_candidates(hipStream_t st, int n_img, long long n_cand, const long long *cand_off,
                           const long long *line_off, const long long *inter_off, const BptLine *lines,
                           const BptInter *inter, const BptGrid *grid, double *cand_xy, unsigned long long *keys,
                           unsigned *idx) {
  if (n_cand <= 0) return;
  hipLaunchKernelGGL(k_bpt_candidates, dim3(grid_of(n_cand)), dim3(kBptBlock), 0, st, n_img, n_cand, cand_off,
                     line_off, inter_off, lines, inter, grid, cand_xy, keys, idx);
}

size_t bpt_sort_pairs_temp_bytes(long long n) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                  (unsigned *)nullptr, (unsigned *)nullptr, (size_t)n, 0, 64, (hipStream_t)0);
  return bytes;
}

int launch_bpt_sort_pairs(hipStream_t st, void *temp, size_t temp_bytes, long long n, const unsigned long long *k_in,
                          unsigned long long *k_out, const unsigned *v_in, unsigned *v_out) {
  if (n <= 0) return 0;
  return (int)rocprim::radix_sort_pairs(temp, temp_bytes, k_in, k_out, v_in, v_out, (size_t)n, 0, 64, st);
}

size_t bpt_sort_keys_temp_bytes(long long n) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_keys(nullptr, bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                 (size_t)n, 0, 64, (hipStream_t)0);
  return bytes;
}

int launch_bpt_sort_keys(hipStream_t st, void *temp, size_t temp_bytes, long long n, const unsigned long long *k_in,
                         unsigned long long *k_out) {
  if (n <= 0) return 0;
  return (int)rocprim::radix_sort_keys(temp, temp_bytes, k_in, k_out, (size_t)n, 0, 64, st);
}

void launch_bpt_close_pairs(hipStream_t st, int fill, long long n_cand, const unsigned long long *keys,
                            const unsigned *idx, const double *cand_xy, double th, int *cnt, const long long *off,
                            unsigned long long *out) {
  if (n_cand <= 0) return;
  if (fill)
    hipLaunchKernelGGL(k_bpt_close_pairs<1>, dim3(grid_of(n_cand)), dim3(kBptBlock), 0, st, n_cand, keys, idx,
                       cand_xy, th, cnt, off, out);
  else
    hipLaunchKernelGGL(k_bpt_close_pairs<0>, dim3(grid_of(n_cand)), dim3(kBptBlock), 0, st, n_cand, keys, idx,
                       cand_xy, th, cnt, off, out);
}

void launch_bpt_nearest(hipStream_t st, const BptBlock *blk, int n_blk, const long long *kp_off, const double *kps,
                        const double *junc_xy, double *dist) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(k_bpt_nearest, dim3(n_blk), dim3(kBptBlock), 0, st, blk, kp_off, kps, junc_xy, dist);
}

}  // namespace lt
