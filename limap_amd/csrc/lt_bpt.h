// lt_bpt.h -- records shared by the host side (lt_bpt.cpp) and the device side (lt_kernels_bpt.hip) of the 2D
// point-line bipartites (limap.structures: PL_Bipartite2d::add_keypoints_with_point3D_ids and
// compute_intersection_with_points, structures/pl_bipartite.cc).  DESIGN §16.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "lt_geom.h"

namespace lt {

constexpr int kBptBlock = 256;         // lanes per workgroup: one point / junction / line pair / candidate each
constexpr int kBptLineTile = 512;      // lines staged in LDS at a time by k_bpt_assoc (7 doubles each: 28 KiB)
constexpr int kBptPointTile = 1024;    // keypoints staged in LDS at a time by k_bpt_nearest (16 KiB)
constexpr int kBptCellBits = 20;       // grid cells per axis of k_bpt_close_pairs: 2^20
constexpr double kBptCellSlack = 1.25; // cell >= slack * threshold_merge_junctions: a pair within the threshold lies
                                       // in adjacent cells whatever the rounding of the cell coordinate
constexpr double kBptCellMin = 0x1p-500;  // no smaller cell: below 2^-511 the square of a coordinate difference
                                          // underflows, and the reference's norm accepts pairs many thresholds apart

// one 2D line, prepared on the device once (k_bpt_prep): direction, length and homogeneous coordinates as
// Line2d::direction() / length() / coords() compute them (base/linebase.h:24-26, linebase.cc:35-39)
struct BptLine {
  double sx, sy, ex, ey;
  double dx, dy, len;
  double c0, c1, c2;
};
static_assert(sizeof(BptLine) == 80, "BptLine layout");

// a workgroup's share: items [begin, end) of image img (points, junctions), the image's first item is at base
struct BptBlock {
  int img, pad_;
  long long begin, end;
};
static_assert(sizeof(BptBlock) == 24, "BptBlock layout");

// the uniform grid of one image's junction candidates: cell coordinate = clamp(floor((x - lo) / cell), 0, 2^20 - 1)
struct BptGrid {
  double lox, loy, cell;
};

// ---- the grid of k_bpt_close_pairs, shared by the device, lt_bpt_junctions and the host twins of lt_bpt.cpp
// (lt_fn_bpt_grid_keys, lt_fn_bpt_close_pairs_host), so that tests reach it without a GPU ----

// the grid of an image with the lines lines4[0 .. 4 n_lines): lo = the smallest endpoint coordinates
inline BptGrid bpt_grid_of(const double *lines4, long long n_lines, double th_m) {
  double lo[2] = {DBL_MAX, DBL_MAX}, hi[2] = {-DBL_MAX, -DBL_MAX};
  for (long long k = 0; k < n_lines; ++k)
    for (int c = 0; c < 4; ++c) {
      lo[c & 1] = std::min(lo[c & 1], lines4[4 * k + c]);
      hi[c & 1] = std::max(hi[c & 1], lines4[4 * k + c]);
    }
  BptGrid g{0.0, 0.0, 1.0};
  if (n_lines > 0) {
    const double ext = std::max(hi[0] - lo[0], hi[1] - lo[1]);
    double cell = std::max(kBptCellSlack * th_m, ext / (double)((1 << kBptCellBits) - 2));
    if (!(cell > 0.0)) cell = 1.0;
    if (cell < kBptCellMin) cell = kBptCellMin;
    g = BptGrid{lo[0], lo[1], cell};
  }
  return g;
}

LT_HD unsigned bpt_cell_of(double v, double lo, double cell) {
  const double u = floor((v - lo) / cell);
  const double hi = (double)((1u << kBptCellBits) - 1u);
  return (unsigned)(u < 0.0 ? 0.0 : (u > hi ? hi : u));  // (a NaN never gets here: the host stops at the flag)
}

// the sort key of a candidate: image << 40 | cell y << 20 | cell x
LT_HD unsigned long long bpt_key_of(int img, double x, double y, const BptGrid &g) {
  return ((unsigned long long)img << (2 * kBptCellBits)) |
         ((unsigned long long)bpt_cell_of(y, g.loy, g.cell) << kBptCellBits) | bpt_cell_of(x, g.lox, g.cell);
}

LT_HD double bpt_norm2(double x, double y) { return sqrt(x * x + y * y); }

LT_HD long long bpt_lower_bound(const unsigned long long *a, long long n, unsigned long long v) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the close pairs (c, j > c) of the candidate at position s of the cell order (keys, idx sorted): the 3 x 3 cells
// around c, one binary search per cell row.  Returns their number; dst (may be null) receives c << 32 | j
LT_HD int bpt_close_pairs_of(long long n_cand, const unsigned long long *keys, const unsigned *idx,
                             const double *cand_xy, double th, long long s, unsigned long long *dst) {
  const unsigned long long key = keys[s];
  const unsigned c = idx[s];
  const double x = cand_xy[2 * (long long)c], y = cand_xy[2 * (long long)c + 1];
  const unsigned mask = (1u << kBptCellBits) - 1u;
  const unsigned cx = (unsigned)key & mask, cy = (unsigned)(key >> kBptCellBits) & mask;
  const unsigned long long img_bits = key >> (2 * kBptCellBits) << (2 * kBptCellBits);
  const unsigned x0 = cx > 0 ? cx - 1 : 0, x1 = cx < mask ? cx + 1 : mask;
  int n = 0;
  for (int dy = -1; dy <= 1; ++dy) {
    if ((dy < 0 && cy == 0) || (dy > 0 && cy == mask)) continue;
    const unsigned long long rowk = img_bits | ((unsigned long long)(cy + dy) << kBptCellBits);
    long long q = bpt_lower_bound(keys, n_cand, rowk | x0);
    const unsigned long long last = rowk | x1;
    for (; q < n_cand && keys[q] <= last; ++q) {
      const unsigned j = idx[q];
      if (j <= c) continue;
      // (intersections[i].p - intersections[j].p).norm() > threshold_merge_junctions, i < j  (:135-137)
      const double dist = bpt_norm2(x - cand_xy[2 * (long long)j], y - cand_xy[2 * (long long)j + 1]);
      if (dist > th) continue;
      if (dst) dst[n] = ((unsigned long long)c << 32) | j;
      ++n;
    }
  }
  return n;
}

// a junction candidate that came from a line pair (the endpoints need no record)
struct BptInter {
  double x, y;
  int l1, l2;  // line indices within the image, l1 < l2
};
static_assert(sizeof(BptInter) == 24, "BptInter layout");

void launch_bpt_prep(hipStream_t st, const double *lines4, long long n_lines, BptLine *out);
// fill = 0: cnt[p] = lines within the threshold of point p; fill = 1: their indices (within the image), ascending, at
// edge[off[p] ..)
void launch_bpt_assoc(hipStream_t st, int fill, const BptBlock *blk, int n_blk, const long long *line_off,
                      const BptLine *lines, const double *pts, double th, int *cnt, const long long *off, int *edge);
// one workgroup per line (row i of its image's upper triangle).  fill = 0: cnt[row] = accepted pairs (i, j > i);
// fill = 1: the records in ascending j at out[off[row] ..).  flag: set to 1 when an accepted junction is not finite
void launch_bpt_intersect(hipStream_t st, int fill, long long n_rows, const int *row_img, const long long *line_off,
                          const BptLine *lines, double th, int *cnt, const long long *off, BptInter *out, int *flag);
// candidates of image m: 2 M endpoints (start, end per line) then its intersections; cand[c] = x, y.  Writes the
// candidate coordinates and their sort keys (image << 40 | cell y << 20 | cell x)
void launch_bpt_candidates(hipStream_t st, int n_img, long long n_cand, const long long *cand_off,
                           const long long *line_off, const long long *inter_off, const BptLine *lines,
                           const BptInter *inter, const BptGrid *grid, double *cand_xy, unsigned long long *keys,
                           unsigned *idx);
size_t bpt_sort_pairs_temp_bytes(long long n);
int launch_bpt_sort_pairs(hipStream_t st, void *temp, size_t temp_bytes, long long n, const unsigned long long *k_in,
                          unsigned long long *k_out, const unsigned *v_in, unsigned *v_out);
size_t bpt_sort_keys_temp_bytes(long long n);
int launch_bpt_sort_keys(hipStream_t st, void *temp, size_t temp_bytes, long long n, const unsigned long long *k_in,
                         unsigned long long *k_out);
// over the candidates in cell order (keys, idx sorted): fill = 0: cnt[c] = candidates j > c of the 3 x 3 cells around
// c with !(|p_c - p_j| > th); fill = 1: the pairs (c << 32 | j) at out[off[c] ..), global candidate indices
void launch_bpt_close_pairs(hipStream_t st, int fill, long long n_cand, const unsigned long long *keys,
                            const unsigned *idx, const double *cand_xy, double th, int *cnt, const long long *off,
                            unsigned long long *out);
// dist[q] = min over the image's keypoints of KDTree::point_distance(junction q), DBL_MAX without keypoints
void launch_bpt_nearest(hipStream_t st, const BptBlock *blk, int n_blk, const long long *kp_off, const double *kps,
                        const double *junc_xy, double *dist);

}  // namespace lt
