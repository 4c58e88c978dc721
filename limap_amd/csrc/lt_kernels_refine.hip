// lt_kernels_refine.hip -- the geometric line refinement on the device: every expression comes from
// lt_refine.h, which lt_refine.cpp compiles for the host path too.
//   k_refine_prep  per support: the 3x6 projection matrix of its view, the 2D endpoints and the weight into the SoA
//                  table; per track: MinimalInfiniteLine3d of its line
//   k_refine_lm    the whole Levenberg-Marquardt loop of a track: kRfWidth lanes of a wave64 per track, lanes over the
//                  supports, the 14 sums of a linearisation reduced by a fixed xor tree of shuffles, the 4x4 solve done
//                  by every lane of the group on the same bits
//   k_refine_cut   GetLineSegmentFromInfiniteLine3d: the two order statistics by rank counting, no sort
// and for a call with the VP or the heatmap term (k_refine_lm and its tables are not involved in what they add):
//   k_refine_prep_terms  per support: the view's unit quaternion, the direction of its vanishing point and the flag
//   k_refine_lm_terms    k_refine_lm with the blocks of the two terms, kRfTermWidth lanes per track; instantiated
//                        without the heatmap term and with it for binary16 and float texels.  The geometric and the VP
//                        term are switches of the launch, the same in every lane.  A lane loads the 4 (cost) or 8
//                        (linearisation) texels of a sample together, before the first of them is used
// and for a call with the feature-consistency term:
//   k_refine_lm_feat     one wave64 per track, four tracks per workgroup: the supports' blocks on the first kRfTermWidth
//                        lanes as above, then one block of 128 residuals per (sample, target) with two channels per
//                        lane -- a texel's channels are one 256-byte (binary16) or 512-byte (float) load of the wave --
//                        its 15 sums reduced by the xor tree over the wave before the loss' derivative scales them
// All stores are ordinary vector stores of the lanes.

#include "lt_refine.h"

namespace lt {

namespace {

__global__ void __launch_bounds__(256) k_refine_prep(const double *__restrict__ kvec, const double *__restrict__ qvec,
                                                     const double *__restrict__ tvec, const int *__restrict__ sup_cam,
                                                     const double *__restrict__ l2d4, long long n_sup,
                                                     double *__restrict__ tab, long long stride,
                                                     const double *__restrict__ line6, long long n_tracks,
                                                     RfOut *__restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_sup) {
    const int cam = sup_cam[i];
    rf_view_matrix(kvec + 4 * (long long)cam, qvec + 4 * (long long)cam, tvec + 3 * (long long)cam, tab + i, stride);
    const double x1 = l2d4[4 * i], y1 = l2d4[4 * i + 1], x2 = l2d4[4 * i + 2], y2 = l2d4[4 * i + 3];
    tab[18 * stride + i] = x1; tab[19 * stride + i] = y1;
    tab[20 * stride + i] = x2; tab[21 * stride + i] = y2;
    const double dx = x2 - x1, dy = y2 - y1;
    tab[22 * stride + i] = sqrt(dx * dx + dy * dy) / 30.0;  // ComputeLineWeights (linetrack.cc:315-322)
  }
  if (i < n_tracks) {
    double p[6];
    rf_minimal(line6 + 6 * i, p);
    for (int c = 0; c < 6; ++c) out[i].p[c] = p[c];
  }
}

// a group whose track ends leaves rf_lm's loop while the other groups of its wave go on; the wave retires with its
// last track
__global__ void __launch_bounds__(kRfBlock) k_refine_lm(RfDev dev, RfOut *__restrict__ out) {
  const long long ti = ((long long)blockIdx.x * kRfBlock + threadIdx.x) / kRfWidth;
  const int lane = threadIdx.x % kRfWidth;
  if (ti >= dev.n_tracks) return;  // a whole group leaves together
  const RfTrack t = dev.tracks[ti];
  double p[6], F0, F1;
  int it, code;
  for (int c = 0; c < 6; ++c) p[c] = out[ti].p[c];
  RfGroup<LmWaveLanes<kRfWidth>> grp{{lane}, dev.sup, dev.stride, t, dev.alpha};
  rf_lm(grp, t.constant != 0, dev.max_iter, p, &F0, &F1, &it, &code);
  if (lane == 0) {
    for (int c = 0; c < 6; ++c) out[ti].p[c] = p[c];
    out[ti].cost0 = F0;
    out[ti].cost1 = F1;
    out[ti].iters = it;
    out[ti].code = code;
  }
}

__global__ void __launch_bounds__(256) k_refine_prep_terms(const double *__restrict__ kvec, const double *__restrict__ qvec,
                                                           const int *__restrict__ sup_cam, const int *__restrict__ vp_flag,
                                                           const double *__restrict__ vp3, long long n_sup,
                                                           double *__restrict__ ext, long long stride) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_sup) return;
  const int cam = sup_cam[i];
  rf_ext_prep(kvec + 4 * (long long)cam, qvec + 4 * (long long)cam, vp_flag[i] != 0, vp3 + 3 * i, ext + i, stride);
}

// the device group of k_refine_lm_terms; its host twin is RfGroupTerms over LmHostLanes.  It is written out here, as is
// the supports' half of DevGroupFeat below: with RfGroupTerms over the wave's lanes in either of the two,
// k_refine_lm_feat<true, unsigned short> gains scratch and spilled registers
template <bool HM, class Tx>
struct DevGroupTerms {
  const RfDev &dev;
  const RfDevTerms &tr;
  const RfTrack &t;
  int lane;
  __device__ __forceinline__ RfGrid<Tx> grid(long long s) const {
    if (!HM) return RfGrid<Tx>{nullptr, 1, 1};
    const RfHm hm = tr.hm[tr.sup_hm[s]];
    return RfGrid<Tx>{static_cast<const Tx *>(tr.texels) + hm.off, hm.h, hm.w};
  }
  __device__ __forceinline__ double cost(const double p[6]) const {
    double dm[6];
    rf_plucker<double>(p, p + 4, dm);
    double part = 0.0;
    for (int k = lane; k < t.n; k += kRfTermWidth) {
      const long long s = t.s0 + k;
      part = part + rf_cost_terms<HM, Tx>(rf_load(dev.sup, dev.stride, s), rf_load_ext(tr.ext, dev.stride, s), grid(s),
                                          tr.cfg, dm, dev.alpha);
    }
    return 0.5 * lm_group_sum<kRfTermWidth>(part);
  }
  __device__ __forceinline__ void linearise(const double p[6], double acc[kRfSums]) const {
    Rf4 u[4], w[2], dm[6];
    rf_seed(p, u, w);
    rf_plucker<Rf4>(u, w, dm);
    for (int c = 0; c < kRfSums; ++c) acc[c] = 0.0;
    for (int k = lane; k < t.n; k += kRfTermWidth) {
      const long long s = t.s0 + k;
      rf_accumulate_terms<HM, Tx>(rf_load(dev.sup, dev.stride, s), rf_load_ext(tr.ext, dev.stride, s), grid(s), tr.cfg, dm,
                                  dev.alpha, acc);
    }
    for (int c = 0; c < kRfSums; ++c) acc[c] = lm_group_sum<kRfTermWidth>(acc[c]);
  }
};

template <bool HM, class Tx>
__global__ void __launch_bounds__(kRfBlock) k_refine_lm_terms(RfDev dev, RfDevTerms tr, RfOut *__restrict__ out) {
  const long long ti = ((long long)blockIdx.x * kRfBlock + threadIdx.x) / kRfTermWidth;
  const int lane = threadIdx.x % kRfTermWidth;
  if (ti >= dev.n_tracks) return;  // a whole group leaves together
  const RfTrack t = dev.tracks[ti];
  double p[6], F0, F1;
  int it, code;
  for (int c = 0; c < 6; ++c) p[c] = out[ti].p[c];
  DevGroupTerms<HM, Tx> grp{dev, tr, t, lane};
  rf_lm_terms(grp, t.constant != 0, dev.max_iter, p, &F0, &F1, &it, &code);
  if (lane == 0) {
    for (int c = 0; c < 6; ++c) out[ti].p[c] = p[c];
    out[ti].cost0 = F0;
    out[ti].cost1 = F1;
    out[ti].iters = it;
    out[ti].code = code;
  }
}

__device__ __forceinline__ double wave_get(double v, int src) { return __shfl(v, src, kRfFeatLanes); }
__device__ __forceinline__ Rf4 wave_get(const Rf4 &a, int src) {
  Rf4 r;
  r.v = wave_get(a.v, src);
  for (int i = 0; i < 4; ++i) r.d[i] = wave_get(a.d[i], src);
  return r;
}

// a wave64 on one track with the feature term.  The supports' blocks go to the first kRfTermWidth lanes exactly as in
// DevGroupTerms -- the other lanes add zeros to the tree, so a track without feature blocks gets k_refine_lm_terms'
// bits.  Lane i < n_img projects the line into image i once per evaluation; a block reads its two projections from
// those lanes.  The geometry of a block is the same in every lane, the texels and the sums are the lane's two channels.
template <bool HM, class Tx>
struct DevGroupFeat {
  const RfDev &dev;
  const RfDevTerms &tr;
  const RfDevFeat &ft;
  const RfTrack &t;
  const RfFTrack &f;
  int lane;
  __device__ __forceinline__ RfGrid<Tx> grid(long long s) const {
    if (!HM) return RfGrid<Tx>{nullptr, 1, 1};
    const RfHm hm = tr.hm[tr.sup_hm[s]];
    return RfGrid<Tx>{static_cast<const Tx *>(tr.texels) + hm.off, hm.h, hm.w};
  }
  __device__ __forceinline__ double cost(const double p[6]) const {
    double dm[6];
    rf_plucker<double>(p, p + 4, dm);
    double part = 0.0;
    if (lane < kRfTermWidth)
      for (int k = lane; k < t.n; k += kRfTermWidth) {
        const long long s = t.s0 + k;
        part = part + rf_cost_terms<HM, Tx>(rf_load(dev.sup, dev.stride, s), rf_load_ext(tr.ext, dev.stride, s), grid(s),
                                            tr.cfg, dm, dev.alpha);
      }
    double total = lm_group_sum<kRfFeatLanes>(part);
    if (f.n_smp == 0) return 0.5 * total;
    double d[3], m[3], mine[3] = {0.0, 0.0, 0.0};
    rf_plucker_c<double>(p, p + 4, d, m);
    const RfFImg *imgs = ft.imgs + f.img0;
    if (lane < f.n_img) rf_w2p<double>(ft.views[imgs[lane].cam], d, m, mine);
    bool ok = true;
    for (int si = 0; si < f.n_smp; ++si) {
      const RfFSample s = ft.smps[f.smp0 + si];
      const RfFImg gr = imgs[s.ref];
      const double cr[3] = {wave_get(mine[0], s.ref), wave_get(mine[1], s.ref), wave_get(mine[2], s.ref)};
      double x, y, lx, ly, fref[2];
      const bool ok_ref = rf_feat_ref_xy<double>(cr, s, gr, &x, &y, &lx, &ly);
      rf_feat_value<Tx>(gr, ly, lx, lane, fref);
      for (int ti = 0; ti < s.n_tgt; ++ti) {
        const int tg = ft.tgts[s.tgt0 + ti];
        const RfFImg gt = imgs[tg];
        const double ct[3] = {wave_get(mine[0], tg), wave_get(mine[1], tg), wave_get(mine[2], tg)};
        double tx, ty;
        const bool ok_tgt = rf_feat_tgt_xy<double>(ct, ft.pairs + 9 * (f.pair0 + (long long)s.ref * f.n_img + tg), x, y, gt, &tx, &ty);
        const double sq = lm_group_sum<kRfFeatLanes>(rf_feat_sq_lane<Tx>(gt, tx, ty, fref, lane));
        if (ok_ref && ok_tgt) total = total + rf_rho(s.weight, sq);
        else ok = false;
      }
    }
    return ok ? 0.5 * total : __builtin_inf();
  }
  __device__ __forceinline__ void linearise(const double p[6], double acc[kRfSums]) const {
    Rf4 u[4], w[2], dm[6];
    rf_seed(p, u, w);
    rf_plucker<Rf4>(u, w, dm);
    for (int c = 0; c < kRfSums; ++c) acc[c] = 0.0;
    if (lane < kRfTermWidth)
      for (int k = lane; k < t.n; k += kRfTermWidth) {
        const long long s = t.s0 + k;
        rf_accumulate_terms<HM, Tx>(rf_load(dev.sup, dev.stride, s), rf_load_ext(tr.ext, dev.stride, s), grid(s), tr.cfg, dm,
                                    dev.alpha, acc);
      }
    for (int c = 0; c < kRfSums; ++c) acc[c] = lm_group_sum<kRfFeatLanes>(acc[c]);
    if (f.n_smp == 0) return;
    Rf4 d[3], m[3], mine[3];
    rf_plucker_c<Rf4>(u, w, d, m);
    for (int c = 0; c < 3; ++c) mine[c] = Rf4(0.0);
    const RfFImg *imgs = ft.imgs + f.img0;
    if (lane < f.n_img) rf_w2p<Rf4>(ft.views[imgs[lane].cam], d, m, mine);
    for (int si = 0; si < f.n_smp; ++si) {
      const RfFSample s = ft.smps[f.smp0 + si];
      const RfFImg gr = imgs[s.ref];
      const Rf4 cr[3] = {wave_get(mine[0], s.ref), wave_get(mine[1], s.ref), wave_get(mine[2], s.ref)};
      Rf4 x, y, lx, ly;
      const bool ok_ref = rf_feat_ref_xy<Rf4>(cr, s, gr, &x, &y, &lx, &ly);
      RfFRef ref;
      rf_feat_ref_lane<Tx>(gr, lx, ly, lane, &ref);
      for (int ti = 0; ti < s.n_tgt; ++ti) {
        const int tg = ft.tgts[s.tgt0 + ti];
        const RfFImg gt = imgs[tg];
        const Rf4 ct[3] = {wave_get(mine[0], tg), wave_get(mine[1], tg), wave_get(mine[2], tg)};
        Rf4 tx, ty;
        const bool ok_tgt = rf_feat_tgt_xy<Rf4>(ct, ft.pairs + 9 * (f.pair0 + (long long)s.ref * f.n_img + tg), x, y, gt, &tx, &ty);
        double blk[kRfFeatSums];
        for (int c = 0; c < kRfFeatSums; ++c) blk[c] = 0.0;
        rf_feat_block_lane<Tx>(gt, tx, ty, ref, lane, blk);
        for (int c = 0; c < kRfFeatSums; ++c) blk[c] = lm_group_sum<kRfFeatLanes>(blk[c]);
        if (ok_ref && ok_tgt) {  // a failed block adds nothing
          const double rho1 = rf_rho1(s.weight, blk[kRfSums]);
          for (int c = 0; c < kRfSums; ++c) acc[c] = acc[c] + rho1 * blk[c];
        }
      }
    }
  }
};

// every lane of a wave holds its track's state; the waves of a workgroup do not talk to each other
template <bool HM, class Tx>
__global__ void __launch_bounds__(kRfFeatBlock) k_refine_lm_feat(RfDev dev, RfDevTerms tr, RfDevFeat ft, RfOut *__restrict__ out) {
  const long long ti = (long long)blockIdx.x * kRfFeatTracks + threadIdx.x / kRfFeatLanes;
  const int lane = threadIdx.x % kRfFeatLanes;
  if (ti >= dev.n_tracks) return;  // a whole wave leaves together
  const RfTrack t = dev.tracks[ti];
  const RfFTrack f = ft.ftracks[ti];
  double p[6], F0, F1;
  int it, code;
  for (int c = 0; c < 6; ++c) p[c] = out[ti].p[c];
  DevGroupFeat<HM, Tx> grp{dev, tr, ft, t, f, lane};
  rf_lm_terms(grp, t.constant != 0, dev.max_iter, p, &F0, &F1, &it, &code);
  if (lane == 0) {
    for (int c = 0; c < 6; ++c) out[ti].p[c] = p[c];
    out[ti].cost0 = F0;
    out[ti].cost1 = F1;
    out[ti].iters = it;
    out[ti].code = code;
  }
}

__global__ void __launch_bounds__(kRfBlock) k_refine_cut(RfDev dev, RfOut *__restrict__ out) {
  const long long ti = ((long long)blockIdx.x * kRfBlock + threadIdx.x) / kRfWidth;
  const int lane = threadIdx.x % kRfWidth;
  if (ti >= dev.n_tracks) return;
  const RfTrack t = dev.tracks[ti];
  double p[6];
  for (int c = 0; c < 6; ++c) p[c] = out[ti].p[c];
  d3 dir, m;
  rf_infinite(p, &dir, &m);
  const double *l3 = dev.l3d + 6 * t.s0;
  const d3 pref = rf_pref(dir, m, mk3(l3[0], l3[1], l3[2]));
  const long long n = 2 * (long long)t.n, lo = dev.num_outliers, hi = n - 1 - dev.num_outliers;
  // every endpoint has at most one writer (rf_rank_test); where no value takes a rank -- a NaN among them -- lane 0
  // writes NaN, as the host does
  bool any_lo = false, any_hi = false;
  for (long long i = lane; i < n; i += kRfWidth) {
    double v;
    bool is_lo, is_hi;
    rf_rank_test(l3, n, i, pref, dir, lo, hi, &v, &is_lo, &is_hi);
    if (is_lo) {
      out[ti].seg[0] = pref.x + dir.x * v; out[ti].seg[1] = pref.y + dir.y * v; out[ti].seg[2] = pref.z + dir.z * v;
    }
    if (is_hi) {
      out[ti].seg[3] = pref.x + dir.x * v; out[ti].seg[4] = pref.y + dir.y * v; out[ti].seg[5] = pref.z + dir.z * v;
    }
    any_lo |= is_lo;
    any_hi |= is_hi;
  }
  int found = (any_lo ? 1 : 0) | (any_hi ? 2 : 0);
#pragma unroll
  for (int m = kRfWidth / 2; m >= 1; m >>= 1) found |= __shfl_xor(found, m, kRfWidth);
  if (lane == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (!(found & 1)) { out[ti].seg[0] = nan; out[ti].seg[1] = nan; out[ti].seg[2] = nan; }
    if (!(found & 2)) { out[ti].seg[3] = nan; out[ti].seg[4] = nan; out[ti].seg[5] = nan; }
  }
}

inline unsigned grid_of(long long n, int block) { return (unsigned)((n + block - 1) / block); }

}  // namespace

void launch_refine_prep(hipStream_t st, const double *kvec, const double *qvec, const double *tvec, const int *sup_cam,
                        const double *l2d4, long long n_sup, double *sup_tab, long long stride, const double *line6,
                        long long n_tracks, RfOut *out) {
  const long long n = n_sup > n_tracks ? n_sup : n_tracks;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_refine_prep, dim3(grid_of(n, 256)), dim3(256), 0, st, kvec, qvec, tvec, sup_cam, l2d4, n_sup,
                     sup_tab, stride, line6, n_tracks, out);
}

void launch_refine_lm(hipStream_t st, const RfDev &dev, RfOut *out) {
  if (dev.n_tracks <= 0) return;
  hipLaunchKernelGGL(k_refine_lm, dim3(grid_of(dev.n_tracks * kRfWidth, kRfBlock)), dim3(kRfBlock), 0, st, dev, out);
}

void launch_refine_prep_terms(hipStream_t st, const double *kvec, const double *qvec, const int *sup_cam,
                              const int *vp_flag, const double *vp3, long long n_sup, double *ext, long long stride) {
  if (n_sup <= 0) return;
  hipLaunchKernelGGL(k_refine_prep_terms, dim3(grid_of(n_sup, 256)), dim3(256), 0, st, kvec, qvec, sup_cam, vp_flag, vp3,
                     n_sup, ext, stride);
}

void launch_refine_lm_terms(hipStream_t st, const RfDev &dev, const RfDevTerms &terms, bool texel_f32, RfOut *out) {
  if (dev.n_tracks <= 0) return;
  const dim3 grid(grid_of(dev.n_tracks * kRfTermWidth, kRfBlock)), block(kRfBlock);
  if (!terms.cfg.use_heatmap)
    hipLaunchKernelGGL((k_refine_lm_terms<false, float>), grid, block, 0, st, dev, terms, out);
  else if (texel_f32)
    hipLaunchKernelGGL((k_refine_lm_terms<true, float>), grid, block, 0, st, dev, terms, out);
  else
    hipLaunchKernelGGL((k_refine_lm_terms<true, unsigned short>), grid, block, 0, st, dev, terms, out);
}

void launch_refine_lm_feat(hipStream_t st, const RfDev &dev, const RfDevTerms &terms, const RfDevFeat &feat, bool texel_f32,
                           RfOut *out) {
  if (dev.n_tracks <= 0) return;
  const dim3 grid(grid_of(dev.n_tracks, kRfFeatTracks)), block(kRfFeatBlock);
  if (!terms.cfg.use_heatmap) {
    if (texel_f32) hipLaunchKernelGGL((k_refine_lm_feat<false, float>), grid, block, 0, st, dev, terms, feat, out);
    else hipLaunchKernelGGL((k_refine_lm_feat<false, unsigned short>), grid, block, 0, st, dev, terms, feat, out);
  } else {
    if (texel_f32) hipLaunchKernelGGL((k_refine_lm_feat<true, float>), grid, block, 0, st, dev, terms, feat, out);
    else hipLaunchKernelGGL((k_refine_lm_feat<true, unsigned short>), grid, block, 0, st, dev, terms, feat, out);
  }
}

void launch_refine_cut(hipStream_t st, const RfDev &dev, RfOut *out) {
  if (dev.n_tracks <= 0) return;
  hipLaunchKernelGGL(k_refine_cut, dim3(grid_of(dev.n_tracks * kRfWidth, kRfBlock)), dim3(kRfBlock), 0, st, dev, out);
}

}  // namespace lt
