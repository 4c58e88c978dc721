// lt_kernels_loc.hip -- the point-line pose refinement on the device: every expression comes from
// lt_loc.h, which lt_loc.cpp compiles for the host path too.
//   k_loc_lm   the whole Levenberg-Marquardt loop of a problem: one wave64 per problem, lanes over its residual blocks
//              (lane l takes blocks l, l + 64, ... in ascending order), the 27 sums of a linearisation reduced by a
//              fixed xor tree of shuffles, the 6x6 solve done by every lane on the same bits.  No atomics, no spinning,
//              no host round trip per iteration.
//   k_loc_score  JointPoseEstimator::EvaluateModelOnPoint for H poses x N correspondences: one wave64 per pose, lanes over
//              the correspondences (coalesced stores into the pose's row of the table); the MSAC score summed like the
//              sums above (lane stride ascending, then the xor tree), the inlier counts by integer shuffles
// All stores are ordinary vector stores of the lanes.

#include "lt_loc.h"

namespace lt {

namespace {

// k_loc_lm's own group; its host twin is LcGroup over LmHostLanes.  With LcGroup over the wave's lanes the kernel keeps
// its registers and scratch and is 1.5 - 3 % slower
struct DevGroup {
  const LcDev &dev;
  const LcProb &pr;
  const double *k;
  int lane;
  __device__ __forceinline__ double cost(const double p[7]) const {
    double part = 0.0;
    for (int i = lane; i < pr.n; i += kLcWidth) part = part + lc_cost_term(dev.cfg, k, p, lc_load(dev.tab, dev.stride, pr.b0 + i));
    return 0.5 * lm_group_sum<kLcWidth>(part);
  }
  __device__ __forceinline__ void linearise(const double p[7], double acc[kLcSums]) const {
    for (int c = 0; c < kLcSums; ++c) acc[c] = 0.0;
    for (int i = lane; i < pr.n; i += kLcWidth) lc_accumulate(dev.cfg, k, p, lc_load(dev.tab, dev.stride, pr.b0 + i), acc);
    for (int c = 0; c < kLcSums; ++c) acc[c] = lm_group_sum<kLcWidth>(acc[c]);
  }
};

__global__ void __launch_bounds__(kLcWidth) k_loc_lm(LcDev dev, LcOut *__restrict__ out) {
  const long long pi = blockIdx.x;
  if (pi >= dev.n_probs) return;
  const LcProb pr = dev.probs[pi];
  double k[4], p[7], F0, F1;
  int it, code;
  for (int c = 0; c < 4; ++c) k[c] = dev.kvec[4 * pi + c];
  for (int c = 0; c < 4; ++c) p[c] = out[pi].q[c];
  for (int c = 0; c < 3; ++c) p[4 + c] = out[pi].t[c];
  DevGroup grp{dev, pr, k, (int)threadIdx.x};
  lc_lm(grp, pr.n, dev.cfg.max_iter, p, &F0, &F1, &it, &code);
  if (threadIdx.x == 0) {
    for (int c = 0; c < 4; ++c) out[pi].q[c] = p[c];
    for (int c = 0; c < 3; ++c) out[pi].t[c] = p[4 + c];
    out[pi].cost0 = F0;
    out[pi].cost1 = F1;
    out[pi].iters = it;
    out[pi].code = code;
  }
}

__global__ void __launch_bounds__(kLcWidth) k_loc_score(LcScoreDev dev, double *__restrict__ table,
                                                       double *__restrict__ scores, int *__restrict__ inliers) {
  const long long h = blockIdx.x;
  if (h >= dev.n_poses) return;
  const int lane = threadIdx.x;
  const long long N = (long long)dev.sc.n_points + dev.sc.n_lines;
  int in0 = 0, in1 = 0;
  const double part = lc_msac_sum(LmWaveLanes<kLcWidth>{lane}, dev.sc, dev.k, dev.qvec + 4 * h, dev.tvec + 3 * h, dev.tab,
                                  dev.stride, 0, dev.sc.n_points, dev.sc.n_lines, [&](int i, bool is_point, double r2) {
    table[h * N + i] = r2;
    if (dev.sc.want_msac && r2 < dev.sc.thr2[is_point ? 0 : 1]) (is_point ? in0 : in1) += 1;
  });
  if (dev.sc.want_msac) {
#pragma unroll
    for (int m = kLcWidth / 2; m >= 1; m >>= 1) {
      in0 += __shfl_xor(in0, m, kLcWidth);
      in1 += __shfl_xor(in1, m, kLcWidth);
    }
    if (lane == 0) {
      scores[h] = part;
      inliers[2 * h] = in0;
      inliers[2 * h + 1] = in1;
    }
  }
}

}  // namespace

void launch_loc_score(hipStream_t st, const LcScoreDev &dev, double *table, double *scores, int *inliers) {
  if (dev.n_poses <= 0) return;
  hipLaunchKernelGGL(k_loc_score, dim3((unsigned)dev.n_poses), dim3(kLcWidth), 0, st, dev, table, scores, inliers);
}

void launch_loc_lm(hipStream_t st, const LcDev &dev, LcOut *out) {
  if (dev.n_probs <= 0) return;
  hipLaunchKernelGGL(k_loc_lm, dim3((unsigned)dev.n_probs), dim3(kLcWidth), 0, st, dev, out);
}

}  // namespace lt
