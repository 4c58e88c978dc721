// lt_kernels_est.hip -- the minimal pose solvers on the device: every expression comes from lt_est.h,
// which lt_est.cpp compiles for the host twin too.
//   k_est_minimal  one lane per sample: the lane loads its sample from the field-major table (coalesced), runs es_solve
//                  and stores its poses and its count.  The solver's arrays (the Sturm chain, the 6 x 13 rows) live in
//                  scratch; lanes of a wave diverge only in the number of real roots.  No atomics, no LDS.
//   k_est_draw     a round's first step: one lane per (query, iteration slot) draws the solver type and the sample and
//                  solves it (eh_draw_solve)
//   k_est_score    the second: one wave64 per (query, slot, pose) scores the pose against every correspondence of its
//                  query, lanes over the correspondences, the MSAC sum in lane order then the xor tree
//   k_est_replay   the third: one wave64 per query replays the round's iterations in order (eh_replay); the local
//                  optimisation's refinements are lc_lm on the wave, its inlier tests run between them on the device
// All stores are ordinary vector stores of the lanes; the one atomic is the count of finished queries the host polls.

#include "lt_est_loop.h"

namespace lt {

namespace {

__global__ void __launch_bounds__(kEsBlock) k_est_minimal(EsDev dev, double *__restrict__ poses, int *__restrict__ counts) {
  const long long i = (long long)blockIdx.x * kEsBlock + threadIdx.x;
  if (i >= dev.n) return;
  double x[3][3], X[3][3], l[3][3], C[3][3], V[3][3], out[kEsMaxSol][kEsPoseDoubles];
  es_load(dev, i, x, X, l, C, V);
  const int n = es_solve(es_num_points(dev.kind), x, X, l, C, V, out);
  double *dst = poses + i * (long long)(kEsMaxSol * kEsPoseDoubles);
  for (int s = 0; s < kEsMaxSol; ++s)
    for (int c = 0; c < kEsPoseDoubles; ++c) dst[s * kEsPoseDoubles + c] = s < n ? out[s][c] : 0.0;
  counts[i] = n;
}

typedef EhWave<LmWaveLanes<kLcWidth>> DevWave;

__global__ void __launch_bounds__(kEsBlock) k_est_draw(EhDev d) {
  const long long idx = (long long)blockIdx.x * kEsBlock + threadIdx.x;
  if (idx >= d.n_queries * d.opt.round_size) return;
  eh_draw_solve(d, idx / d.opt.round_size, (int)(idx % d.opt.round_size));
}

__global__ void __launch_bounds__(kLcWidth) k_est_score(EhDev d) {
  const long long idx = blockIdx.x;  // (query, slot, pose)
  const long long ri = idx / kEsMaxSol, q = ri / d.opt.round_size;
  const int m = (int)(idx % kEsMaxSol);
  if (q >= d.n_queries || m >= d.r_counts[ri]) return;
  const EhQuery &qr = d.qs[q];
  const DevWave g{{(int)threadIdx.x}, d, qr, eh_score_cfg(d.opt, qr)};
  const double sc = g.score_impl(d.r_poses + (ri * kEsMaxSol + m) * kEsPoseDoubles, false);
  if (threadIdx.x == 0) d.r_scores[ri * kEsMaxSol + m] = sc;
}

__global__ void __launch_bounds__(kLcWidth) k_est_replay(EhDev d) {
  const long long q = blockIdx.x;
  if (q >= d.n_queries) return;
  EhState s = d.st[q];
  if (s.done) return;
  const EhQuery &qr = d.qs[q];
  DevWave g{{(int)threadIdx.x}, d, qr, eh_score_cfg(d.opt, qr)};
  eh_replay(g, d, q, s);
  if (threadIdx.x == 0) {
    d.st[q] = s;
    if (s.done) atomicAdd(d.n_done, 1);
  }
}

}  // namespace

void launch_est_round(hipStream_t st, const EhDev &dev) {
  if (dev.n_queries <= 0) return;
  const long long slots = dev.n_queries * dev.opt.round_size;
  hipLaunchKernelGGL(k_est_draw, dim3((unsigned)((slots + kEsBlock - 1) / kEsBlock)), dim3(kEsBlock), 0, st, dev);
  hipLaunchKernelGGL(k_est_score, dim3((unsigned)(slots * kEsMaxSol)), dim3(kLcWidth), 0, st, dev);
  hipLaunchKernelGGL(k_est_replay, dim3((unsigned)dev.n_queries), dim3(kLcWidth), 0, st, dev);
}

void launch_est_minimal(hipStream_t st, const EsDev &dev, double *poses, int *counts) {
  if (dev.n <= 0) return;
  const long long blocks = (dev.n + kEsBlock - 1) / kEsBlock;
  hipLaunchKernelGGL(k_est_minimal, dim3((unsigned)blocks), dim3(kEsBlock), 0, st, dev, poses, counts);
}

}  // namespace lt
