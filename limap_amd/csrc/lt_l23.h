// lt_l23.h -- 2D-3D line matching for localization (limap_amd.localization): the pair test of
// optimize/hybrid_localization/functions.py (compute_epipolar_IoU above a threshold, a track behind the database line)
// and the reprojection filter with its three distances.  Every expression is LT_HD: lt_kernels_l23.hip compiles it
// for the device, lt_l23.cpp for the host twin, both with -ffp-contract=off, so the two agree bit for bit.
#pragma once

#include "lt_geom.h"

#include <cstdint>

namespace lt {

enum { kL23AllPairs = 0, kL23Listed = 1, kL23ListedFiltered = 2 };
enum { kL23NoFilter = 0, kL23Perpendicular = 1, kL23Midpoint = 2, kL23MidpointPerpendicular = 3 };
constexpr int kL23Block = 256;  // four waves: one (task, query line) unit or one keyed line each

struct L23Cfg {
  int mode, filter;
  double iou_thr, dist_thres, sine_thres, angle_scale;
};

// What the pair test reads of a database segment: the endpoints and Line2d::coords() (64 B)
struct L23DbSeg {
  double x1, y1, x2, y2;
  double lc[3];
  double pad_;
};
static_assert(sizeof(L23DbSeg) == 64, "L23DbSeg layout");

LT_HD void l23_dbseg_build(const Cam &c, const double *s4, L23DbSeg *r) {
  Seg s;
  seg_build(c, s4[0], s4[1], s4[2], s4[3], &s);
  r->x1 = s.x1; r->y1 = s.y1; r->x2 = s.x2; r->y2 = s.y2;
  r->lc[0] = s.lc[0]; r->lc[1] = s.lc[1]; r->lc[2] = s.lc[2];
  r->pad_ = 0.0;
}

// compute_epipolar_IoU(l_i, view_q, l_j, view_d) > IoU_threshold (functions.py:20-21,46-49): strict, a NaN fails.
// epipolar_iou reads the endpoints of the query segment, the endpoints and coords() of the database segment.
LT_HD bool l23_iou_test(const L23Cfg &c, const double *qs4, const L23DbSeg &d, const double *F) {
  Seg s1, s2;
  s1.x1 = qs4[0]; s1.y1 = qs4[1]; s1.x2 = qs4[2]; s1.y2 = qs4[3];
  s2.x1 = d.x1; s2.y1 = d.y1; s2.x2 = d.x2; s2.y2 = d.y2;
  s2.lc[0] = d.lc[0]; s2.lc[1] = d.lc[1]; s2.lc[2] = d.lc[2];
  return epipolar_iou(s1, s2, F) > c.iou_thr;
}

// ---- the reprojection filter (functions.py:66-140).  NumPy's norm, dot, cross and clip on 2-vectors are the plain
// left-to-right FP64 expressions here; Line2d's members are lt_geom.h's len / dir (linebase.cc) ----
LT_HD double l23_cross(d2 a, d2 b) { return a.x * b.y - a.y * b.x; }
LT_HD d2 l23_mid(const L2 &l) { return scale(add(l.s, l.e), 0.5); }

LT_HD double l23_dist(int kind, const L2 &ref, const L2 &tgt) {
  if (kind == kL23Midpoint) {  // :66-67
    const d2 v = sub(l23_mid(ref), l23_mid(tgt));
    return sqrt(v.x * v.x + v.y * v.y);
  }
  const d2 dv = dir(tgt);
  if (kind == kL23MidpointPerpendicular)  // :70-75: divided by the QUERY line's length
    return fabs(l23_cross(dv, sub(tgt.s, l23_mid(ref)))) / len(ref);
  // :78-83: not divided
  return 0.5 * (fabs(l23_cross(dv, sub(tgt.s, ref.s))) + fabs(l23_cross(dv, sub(tgt.s, ref.e))));
}

constexpr double kL23Inf = __builtin_huge_val();

// The loss of one candidate track of a query line (:115-133); +inf where upstream skips it and where the loss is a NaN
// (which never wins upstream's strict `<`).  The projection is CameraView::projection: no cheirality test.
LT_HD double l23_cand_loss(const L23Cfg &c, const Cam &cam, const L2 &ref, const double *t6) {
  const L2 l2d{cam_project(cam, mk3(t6[0], t6[1], t6[2])), cam_project(cam, mk3(t6[3], t6[4], t6[5]))};
  const double dist = l23_dist(c.filter, ref, l2d);
  double loss = dist;
  if (c.filter == kL23Midpoint) {
    const double length = len(l2d);
    double cosine = dot(dir(ref), dir(l2d));
    cosine = cosine < -1.0 ? -1.0 : (cosine > 1.0 ? 1.0 : cosine);
    const double sine = sqrt(1.0 - cosine * cosine);
    loss = loss + c.angle_scale * length * sine;
    if (sine > c.sine_thres) return kL23Inf;
  }
  if (dist > c.dist_thres) return kL23Inf;
  return loss == loss ? loss : kL23Inf;
}

// the order of the filter's minimum: (loss, track id) lexicographically -- equal losses go to the smaller id, and
// duplicates of a track are equal pairs
LT_HD bool l23_better(double la, int ta, double lb, int tb) { return la < lb || (la == lb && ta < tb); }

// the range of the CSR offsets off[0 .. n] that holds x: the largest k < n with off[k] <= x (empty ranges are passed over)
LT_HD long long l23_find(const long long *off, long long n, long long x) {
  long long lo = 0, hi = n;  // off[lo] <= x < off[hi]
  while (hi - lo > 1) {
    const long long mid = lo + (hi - lo) / 2;
    if (off[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the arrays of one call, device or host
struct L23Dev {
  L23Cfg cfg;
  long long n_db, n_query, n_task, n_dbseg, n_qseg, n_units, n_pairs, n_tracks;
  const double *db_cam11, *q_cam11, *db_seg4, *q_seg4, *track6;
  const long long *db_seg_off, *q_seg_off, *task_off, *unit_off, *pair_off;
  const int *task_db, *task_q, *db_track, *pairs2;
  Cam *db_cam, *q_cam;
  L23DbSeg *db_rec;
  double *task_F;          // 9 per task
  // all_pairs
  unsigned *count;         // per unit (task, query line): survivors
  unsigned *unit_pos;      // per unit: first row of the unit within its query
  int *first;              // per query segment: first task with a survivor (the query's task count where none)
  long long *tot;          // per query segment: survivors of the line
  // keyed lines: slot q_seg_off[q] + p is the p-th line of query q in key order
  int *kl_line;
  long long *kl_start;     // first row of the line within its query
  long long *kl_cnt;
  long long *q_total;      // per query: [0] rows, [1] keyed lines
  const long long *q_row0; // per query: its first row in rows2 (set before the fill)
  int *rows2;              // (line, track) per row
  long long rows_cap;      // rows rows2 has room for
  unsigned char *keep;     // listed modes: per listed pair
  // filter
  int *win_track;          // per slot, -1: none
  double *win_loss;
  int *out_rows2;          // per slot, compacted per query from q_seg_off[q]
  double *out_loss;
  long long *out_cnt;      // per query
};

#ifndef LT_HOST_ONLY
void launch_l23_build(hipStream_t st, const L23Dev &d);
void launch_l23_count(hipStream_t st, const L23Dev &d);
void launch_l23_scan(hipStream_t st, const L23Dev &d);
void launch_l23_fill(hipStream_t st, const L23Dev &d);
void launch_l23_listed(hipStream_t st, const L23Dev &d);
void launch_l23_filter(hipStream_t st, const L23Dev &d);
#endif

}  // namespace lt
