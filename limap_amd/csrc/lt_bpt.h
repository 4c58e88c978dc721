// lt_bpt.h -- records shared by the host side (lt_bpt.cpp) and the device side (lt_kernels_bpt.hip) of the 2D
// point-line bipartites (limap.structures: PL_Bipartite2d::add_keypoints_with_point3D_ids and
// compute_intersection_with_points, structures/pl_bipartite.cc).  DESIGN §16.
#pragma once

#include <hip/hip_runtime.h>

namespace lt {

constexpr int kBptBlock = 256;         // lanes per workgroup: one point / junction / line pair / candidate each
constexpr int kBptLineTile = 512;      // lines staged in LDS at a time by k_bpt_assoc (7 doubles each: 28 KiB)
constexpr int kBptPointTile = 1024;    // keypoints staged in LDS at a time by k_bpt_nearest (16 KiB)
constexpr int kBptCellBits = 20;       // grid cells per axis of k_bpt_close_pairs: 2^20
constexpr double kBptCellSlack = 1.25; // cell >= slack * threshold_merge_junctions: a pair within the threshold lies
                                       // in adjacent cells whatever the rounding of the cell coordinate

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
