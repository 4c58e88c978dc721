// lt_fit.h -- records shared by the host side (lt_fit.cpp) and the device side (lt_kernels_fit.hip) of the line fitter
// (limap.fitting, fitting/fitting.py:8-53, fitting/line3d_estimator.cc).  DESIGN §12.
#pragma once

#include <hip/hip_runtime.h>

#include "lt_geom.h"

namespace lt {

constexpr int kFitLds = 256;  // points a workgroup keeps in LDS (32 B each); longer sets use the global scratch

struct FitCfg {  // LORansacOptions plus the front half's parameters, as the kernel reads them
  double t2_points;  // squared inlier threshold of the point-set path
  double ransac_th, min_pct, var2d;
  double pmiss;  // 1 - success_probability_
  double mult;   // threshold_multiplier_
  int min_it, max_it, num_lo, num_lsq, min_smp_mult, nonmin_mult, lo_start, final_ls;
  unsigned long long seed;
};

struct FitImg {  // one image of a depth batch
  const void *map;
  long long h, w, stride;  // stride in elements
  long long seg_begin, seg_end;  // segments of the image inside the batch
  int dtype;  // 0 float32, 1 float64
  int img_id;
  int cam;  // index into the camera table
  int pad_;
};

struct ScanImg {  // one image of a scan batch (estimate_seg3d_from_points3d)
  const void *map;
  long long h, w;          // the scan's rows and columns
  long long rs, ps, cs;    // row, pixel and channel strides in elements
  long long img_h, img_w;  // the camera's image size (the keep filter, the uncertainty)
  long long seg_begin, seg_end;
  double pose[12];  // Tr[:3, :4] row-major when use_pose
  int dtype;        // 0 float32, 1 float64
  int img_id;
  int cam;
  int use_pose;
};

void launch_fit_depth(hipStream_t st, long long n_segs, int n_img, const FitImg *imgs, const double *segs,
                      const Cam *cams, const FitCfg &cfg, double *scratch, unsigned long long scratch_cap,
                      unsigned long long *scratch_cnt, double *seg3d, int *status, int *stats);
void launch_fit_scan(hipStream_t st, long long n_segs, int n_img, const ScanImg *imgs, const double *segs,
                     const Cam *cams, const FitCfg &cfg, double *scratch, unsigned long long scratch_cap,
                     unsigned long long *scratch_cnt, double *seg3d, int *status, int *stats);
void launch_fit_points(hipStream_t st, long long n_sets, const long long *off, const double *xyz, const FitCfg &cfg,
                       double *scratch, unsigned long long scratch_cap, unsigned long long *scratch_cnt, double *seg3d,
                       int *status, int *stats, unsigned char *mask);

}  // namespace lt
