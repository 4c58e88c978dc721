// lt_kernels_sold2.hip -- device side of the SOLD2 line detection (limap_amd.line2d).  A whole scene, with
// ragged junction counts and heatmap sizes, goes through one launch of each kernel; nothing returns to the host
// between the stages.
//   k_s2_block_scale    one workgroup per (image, refinement block): maximum and count of the values above
//                       valid_thresh, radix select of the k-th largest on the float bits (256-bin histograms in LDS,
//                       four passes), the top-share sum in 64-bit fixed point (order independent), the block's scale
//   k_s2_refine_pixels  one lane per pixel: the clamped quotients of the covering blocks in the reference's loop order
//   k_s2_suppress       one wave per junction pair i < j: lanes run over the other junctions from an LDS table
//   k_s2_score          one wave per surviving candidate, one lane per sample: local-max or bilinear sample, the wave's
//                       fixed summation tree, the mean and inlier tests
//   k_s2_compact        one workgroup per image: prefix sum of the detections in candidate order (no atomics)
//   k_s2_refine_junc    one workgroup per detected segment: num_perturbs^4 perturbed segments dealt over the lanes,
//                       arg-max with the lowest index on equal means; the heatmap window in LDS where it fits
//   k_s2_descinfo       one wave per point: bilinear grid_sample of a channel-last descriptor map, L2 normalisation
// Every expression is lt_sold2.h's.

#include "lt_sold2.h"

namespace lt {

namespace {

__device__ __forceinline__ float wave_tree_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, kS2Wave);
  return __shfl(v, 0, kS2Wave);
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kS2Block) k_s2_block_scale(long long n_blocks, const S2Img *__restrict__ imgs,
                                                             const int *__restrict__ blk_img,
                                                             const S2Cfg *__restrict__ cfgp, float *__restrict__ scales) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_max;
  __shared__ unsigned s_cnt;
  __shared__ unsigned s_prefix, s_mask, s_above;
  __shared__ unsigned long long s_want, s_sum;
  const long long b = blockIdx.x;
  if (b >= n_blocks) return;
  const S2Img &im = imgs[blk_img[b]];
  const int lb = (int)(b - im.blk0);
  const int a = lb / im.nb, c = lb % im.nb;
  const int r0 = im.r0[a], r1 = im.r1[a], c0 = im.c0[c], c1 = im.c1[c];
  const int bw = c1 - c0;
  const long long count = (long long)(r1 - r0) * bw;
  const float vt = cfgp->valid_thresh;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_max = 0u;
    s_cnt = 0u;
    s_sum = 0ull;
  }
  __syncthreads();
  // values above valid_thresh >= 0 are positive: their bits order like the values
  unsigned my_max = 0u, my_cnt = 0u;
  for (long long p = tid; p < count; p += kS2Block) {
    const float v = im.heat[(long long)(r0 + (int)(p / bw)) * im.heat_stride + c0 + (int)(p % bw)];
    if (v > vt) {
      ++my_cnt;
      const unsigned u = s2_bits(v);
      my_max = u > my_max ? u : my_max;
    }
  }
  atomicMax(&s_max, my_max);
  atomicAdd(&s_cnt, my_cnt);
  __syncthreads();
  const unsigned n_valid = s_cnt;
  if (n_valid == 0u) {  // the block's maximum is not above valid_thresh
    if (tid == 0) scales[b] = -1.f;
    return;
  }
  double kd = ceil((double)n_valid * cfgp->ratio);
  long long k = (long long)kd;
  if (k > (long long)n_valid) k = n_valid;
  if (k < 1) k = 1;
  // radix select of the k-th largest value: 8 bits a pass from the top
  if (tid == 0) {
    s_prefix = 0u;
    s_mask = 0u;
    s_want = (unsigned long long)k;
    s_above = 0u;
  }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hist[tid] = 0u;
    __syncthreads();
    const unsigned prefix = s_prefix, mask = s_mask;
    for (long long p = tid; p < count; p += kS2Block) {
      const float v = im.heat[(long long)(r0 + (int)(p / bw)) * im.heat_stride + c0 + (int)(p % bw)];
      if (v > vt) {
        const unsigned u = s2_bits(v);
        if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 0xffu], 1u);
      }
    }
    __syncthreads();
    if (tid == 0) {
      unsigned long long want = s_want;
      int d = 255;
      for (; d > 0; --d) {
        if (hist[d] >= want) break;
        want -= hist[d];
      }
      s_above += (unsigned)(s_want - want);  // values above the chosen digit are above the k-th value
      s_want = want;
      s_prefix = prefix | ((unsigned)d << shift);
      s_mask = mask | (0xffu << shift);
    }
    __syncthreads();
  }
  const unsigned kth = s_prefix;
  float kth_f;
  __builtin_memcpy(&kth_f, &kth, 4);
  float vmax;
  {
    const unsigned m = s_max;
    __builtin_memcpy(&vmax, &m, 4);
  }
  const int sh = s2_sum_shift(vt, vmax, (long long)n_valid);
  unsigned long long my_sum = 0ull;
  for (long long p = tid; p < count; p += kS2Block) {
    const float v = im.heat[(long long)(r0 + (int)(p / bw)) * im.heat_stride + c0 + (int)(p % bw)];
    if (v > vt && s2_bits(v) > kth) my_sum += s2_fixed(v, sh);
  }
  atomicAdd(&s_sum, my_sum);
  __syncthreads();
  if (tid == 0) {
    const unsigned long long rest = (unsigned long long)k - (unsigned long long)s_above;
    scales[b] = s2_scale(s_sum + rest * s2_fixed(kth_f, sh), sh, k);
  }
}

__global__ void __launch_bounds__(kS2Block) k_s2_refine_pixels(const S2Img *__restrict__ imgs,
                                                               const float *__restrict__ scales) {
  const S2Img &im = imgs[blockIdx.y];
  if (im.nb == 0) return;
  const long long n = (long long)im.H * im.W;
  for (long long p = (long long)blockIdx.x * kS2Block + threadIdx.x; p < n; p += (long long)gridDim.x * kS2Block) {
    const int y = (int)(p / im.W), x = (int)(p % im.W);
    im.refined[p] = s2_refined_pixel(im, scales, y, x, im.heat[(long long)y * im.heat_stride + x]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kS2Block) k_s2_suppress(const S2Img *__restrict__ imgs, const S2Cfg *__restrict__ cfgp,
                                                          unsigned char *__restrict__ cand) {
  __shared__ float tab[kS2Tab * 2];
  const S2Img &im = imgs[blockIdx.y];
  const int n = im.n;
  const long long n_pairs = (long long)n * (n - 1) / 2;
  const int lane = threadIdx.x & (kS2Wave - 1), wave = threadIdx.x / kS2Wave;
  const long long first = (long long)blockIdx.x * (kS2Block / kS2Wave);
  if (first >= n_pairs) return;  // the whole workgroup leaves: no barrier is left behind
  const long long p = first + wave;
  const bool live = p < n_pairs;
  int i = 0, j = 1;
  if (live) s2_pair_decode(n, p, i, j);
  const float ih = im.junc[2 * i], iw = im.junc[2 * i + 1], jh = im.junc[2 * j], jw = im.junc[2 * j + 1];
  const float tol = cfgp->nms_tol;
  bool hit = false;
  for (int base = 0; base < n; base += kS2Tab) {
    const int m = n - base < kS2Tab ? n - base : kS2Tab;
    __syncthreads();
    for (int t = threadIdx.x; t < 2 * m; t += kS2Block) tab[t] = im.junc[2 * base + t];
    __syncthreads();
    if (live)
      for (int t = lane; t < m; t += kS2Wave) {
        const int k = base + t;
        if (k != i && k != j && s2_suppresses(ih, iw, jh, jw, tab[2 * t], tab[2 * t + 1], tol)) hit = true;
      }
  }
  const bool any = __any(hit);
  if (live && lane == 0) cand[im.pair0 + p] = any ? 0 : 1;
}

__global__ void __launch_bounds__(kS2Block) k_s2_score(const S2Img *__restrict__ imgs, const S2Cfg *__restrict__ cfgp,
                                                       const unsigned char *__restrict__ cand,
                                                       unsigned char *__restrict__ det) {
  const S2Img &im = imgs[blockIdx.y];
  const int n = im.n;
  const long long n_pairs = (long long)n * (n - 1) / 2;
  const int lane = threadIdx.x & (kS2Wave - 1), wave = threadIdx.x / kS2Wave;
  const long long p = (long long)blockIdx.x * (kS2Block / kS2Wave) + wave;
  if (p >= n_pairs) return;
  if (!cand[im.pair0 + p]) {
    if (lane == 0) det[im.pair0 + p] = 0;
    return;
  }
  const S2Cfg &c = *cfgp;
  int i, j;
  s2_pair_decode(n, p, i, j);
  const float sh = im.junc[2 * i], sw = im.junc[2 * i + 1], eh = im.junc[2 * j], ew = im.junc[2 * j + 1];
  const S2HeatGlobal heat{im.stage, im.stage_stride};
  float v = 0.f;
  if (lane < c.num_samples) {
    const float h = s2_sample_pos(sh, eh, c.sampler[lane], (float)(im.H - 1));
    const float w = s2_sample_pos(sw, ew, c.sampler[lane], (float)(im.W - 1));
    v = c.bilinear ? s2_bilinear(heat, h, w)
                   : s2_local_max(heat, h, w, im.H, im.W, c.radius, s2_dist_thresh(c, sh, sw, eh, ew, im.diag));
  }
  const float mean = wave_tree_sum(v) / (float)c.num_samples;
  bool ok = mean > c.detect_thresh;
  if (c.inlier_thresh > 0.f) {
    const unsigned long long b = __ballot(lane < c.num_samples && v > c.detect_thresh);
    ok = ok && ((float)__popcll(b) / (float)c.num_samples >= c.inlier_thresh);
  }
  if (lane == 0) det[im.pair0 + p] = ok ? 1 : 0;
}

// the detections of an image in candidate order: list[pair0 + r] = pair of the r-th detection, seg_cnt[img] = count
__global__ void __launch_bounds__(kS2Block) k_s2_compact(const S2Img *__restrict__ imgs,
                                                         const unsigned char *__restrict__ det,
                                                         unsigned *__restrict__ list, long long *__restrict__ seg_cnt) {
  __shared__ unsigned wsum[kS2Block / kS2Wave];
  __shared__ unsigned s_base;
  const S2Img &im = imgs[blockIdx.x];
  const long long n_pairs = (long long)im.n * (im.n - 1) / 2;
  const int tid = threadIdx.x, lane = tid & (kS2Wave - 1), wave = tid / kS2Wave;
  if (tid == 0) s_base = 0u;
  __syncthreads();
  for (long long base = 0; base < n_pairs; base += kS2Block) {
    const long long p = base + tid;
    const bool d = p < n_pairs && det[im.pair0 + p];
    const unsigned long long b = __ballot(d);
    const unsigned before = (unsigned)__popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = (unsigned)__popcll(b);
    __syncthreads();
    unsigned off = s_base;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (d) list[im.pair0 + off + before] = (unsigned)p;
    __syncthreads();
    if (tid == 0) {
      unsigned t = 0;
      for (int w = 0; w < kS2Block / kS2Wave; ++w) t += wsum[w];
      s_base += t;
    }
    __syncthreads();
  }
  if (tid == 0) seg_cnt[blockIdx.x] = s_base;
}

// seg_off[0 .. n_img] from the counts (in place: seg_off[i + 1] holds count i on entry)
__global__ void k_s2_seg_offsets(int n_img, long long *seg_off) {
  if (threadIdx.x || blockIdx.x) return;
  long long acc = 0;
  seg_off[0] = 0;
  for (int i = 0; i < n_img; ++i) {
    acc += seg_off[i + 1];
    seg_off[i + 1] = acc;
  }
}

struct S2HeatWindow {
  const float *win;
  int y0, x0, ww;
  __device__ __forceinline__ float operator()(int y, int x) const { return win[(y - y0) * ww + (x - x0)]; }
};

template <class Heat>
__device__ __forceinline__ void best_perturbation(const S2Cfg &c, const Heat &heat, float sh, float sw, float eh, float ew,
                                                  int H, int W, int total, float &best, int &best_idx) {
  for (int idx = threadIdx.x; idx < total; idx += kS2Block) {
    float seg[4];
    s2_perturbed(c, idx, sh, sw, eh, ew, H, W, seg);
    const float sc = s2_perturb_score(c, heat, seg, H, W);
    if (best_idx < 0 || sc > best) {  // idx grows: an equal mean keeps the lower index
      best = sc;
      best_idx = idx;
    }
  }
}

__global__ void __launch_bounds__(kS2Block) k_s2_refine_junc(int n_img, const S2Img *__restrict__ imgs,
                                                             const S2Cfg *__restrict__ cfgp,
                                                             const unsigned *__restrict__ list,
                                                             const long long *__restrict__ seg_off,
                                                             S2Seg *__restrict__ segs, int refine) {
  __shared__ float win[kS2WinFloats];
  __shared__ float r_val[kS2Block];
  __shared__ int r_idx[kS2Block];
  const S2Cfg &c = *cfgp;
  const long long total_segs = seg_off[n_img];
  const int tid = threadIdx.x;
  for (long long s = blockIdx.x; s < total_segs; s += gridDim.x) {
    int lo = 0, hi = n_img - 1;  // the image of segment s: the last one whose offset is <= s
    while (lo < hi) {
      const int mid = (lo + hi + 1) / 2;
      if (seg_off[mid] <= s) lo = mid; else hi = mid - 1;
    }
    const S2Img &im = imgs[lo];
    const long long p = list[im.pair0 + (s - seg_off[lo])];
    int i, j;
    s2_pair_decode(im.n, p, i, j);
    const float sh = im.junc[2 * i], sw = im.junc[2 * i + 1], eh = im.junc[2 * j], ew = im.junc[2 * j + 1];
    if (!refine) {
      if (tid == 0) segs[s] = S2Seg{sh, sw, eh, ew, i, j, -1, lo};
      continue;
    }
    const int P = c.num_perturbs, total = P * P * P * P;
    // the window every sample of every perturbed segment reads: the clamped bounding box, widened by the reach of the
    // perturbations, plus the ceil neighbour
    float reach = 0.f;
    for (int q = 0; q < P; ++q) reach = s2_max(reach, c.perturb[q] < 0.f ? -c.perturb[q] : c.perturb[q]);
    const int y0 = s2_clampi((int)floorf((sh < eh ? sh : eh) - reach) - 2, 0, im.H - 1);
    const int y1 = s2_clampi((int)ceilf((sh > eh ? sh : eh) + reach) + 2, 0, im.H - 1);
    const int x0 = s2_clampi((int)floorf((sw < ew ? sw : ew) - reach) - 2, 0, im.W - 1);
    const int x1 = s2_clampi((int)ceilf((sw > ew ? sw : ew) + reach) + 2, 0, im.W - 1);
    const int wh = y1 - y0 + 1, ww = x1 - x0 + 1;
    float best = 0.f;
    int best_idx = -1;
    __syncthreads();  // the window and the reduction arrays of the previous segment are no longer read
    const bool finite = s2_finite(sh) && s2_finite(sw) && s2_finite(eh) && s2_finite(ew);
    if (finite && wh > 0 && ww > 0 && (long long)wh * ww <= (long long)c.win_floats) {
      for (int t = tid; t < wh * ww; t += kS2Block) win[t] = im.stage[(long long)(y0 + t / ww) * im.stage_stride + x0 + t % ww];
      __syncthreads();
      best_perturbation(c, S2HeatWindow{win, y0, x0, ww}, sh, sw, eh, ew, im.H, im.W, total, best, best_idx);
    } else {
      best_perturbation(c, S2HeatGlobal{im.stage, im.stage_stride}, sh, sw, eh, ew, im.H, im.W, total, best, best_idx);
    }
    r_val[tid] = best;
    r_idx[tid] = best_idx;
    __syncthreads();
    for (int off = kS2Block / 2; off >= 1; off >>= 1) {
      if (tid < off) {
        const float ov = r_val[tid + off];
        const int oi = r_idx[tid + off];
        const int mi = r_idx[tid];
        if (oi >= 0 && (mi < 0 || ov > r_val[tid] || (ov == r_val[tid] && oi < mi))) {
          r_val[tid] = ov;
          r_idx[tid] = oi;
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      float seg[4];
      s2_perturbed(c, r_idx[0], sh, sw, eh, ew, im.H, im.W, seg);
      segs[s] = S2Seg{seg[0], seg[1], seg[2], seg[3], i, j, r_idx[0], lo};
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// pts: (h, w) of every point; pt_off[n_img + 1]; maps[img]: address of the channel-last map; dims[4 img ..] = Hd, Wd,
// C, grid_size; outs[img]: address of the image's (C, points) output
__global__ void __launch_bounds__(kS2Block) k_s2_descinfo(long long n_pts, int n_img, const float *__restrict__ pts,
                                                          const long long *__restrict__ pt_off,
                                                          const long long *__restrict__ maps, const int *__restrict__ dims,
                                                          const long long *__restrict__ outs) {
  const int lane = threadIdx.x & (kS2Wave - 1), wave = threadIdx.x / kS2Wave;
  const long long p = (long long)blockIdx.x * (kS2Block / kS2Wave) + wave;
  if (p >= n_pts) return;
  int lo = 0, hi = n_img - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (pt_off[mid] <= p) lo = mid; else hi = mid - 1;
  }
  const int Hd = dims[4 * lo], Wd = dims[4 * lo + 1], C = dims[4 * lo + 2], grid = dims[4 * lo + 3];
  const float *map = reinterpret_cast<const float *>(maps[lo]);
  const long long n_loc = pt_off[lo + 1] - pt_off[lo], loc = p - pt_off[lo];
  const float iy = s2_desc_coord(pts[2 * p], (float)(Hd * grid), Hd);
  const float ix = s2_desc_coord(pts[2 * p + 1], (float)(Wd * grid), Wd);
  float acc = 0.f;
  for (int ch = lane; ch < C; ch += kS2Wave) {
    const float v = s2_desc_sample(map, Hd, Wd, C, iy, ix, ch);
    acc = acc + v * v;
  }
  const float norm = sqrtf(wave_tree_sum(acc));
  const float den = norm > 1e-12f ? norm : 1e-12f;
  float *o = reinterpret_cast<float *>(outs[lo]);
  for (int ch = lane; ch < C; ch += kS2Wave) o[(long long)ch * n_loc + loc] = s2_desc_sample(map, Hd, Wd, C, iy, ix, ch) / den;
}

}  // namespace

void launch_s2_block_scale(hipStream_t st, long long n_blocks, const S2Img *imgs, const int *blk_img, const S2Cfg *cfg,
                           float *scales) {
  if (n_blocks > 0)
    hipLaunchKernelGGL(k_s2_block_scale, dim3((unsigned)n_blocks), dim3(kS2Block), 0, st, n_blocks, imgs, blk_img, cfg, scales);
}

void launch_s2_refine_pixels(hipStream_t st, int n_img, int grid_x, const S2Img *imgs, const float *scales) {
  if (n_img > 0 && grid_x > 0)
    hipLaunchKernelGGL(k_s2_refine_pixels, dim3((unsigned)grid_x, (unsigned)n_img), dim3(kS2Block), 0, st, imgs, scales);
}

static unsigned pair_grid(long long max_pairs) {
  const int per = kS2Block / kS2Wave;
  return (unsigned)((max_pairs + per - 1) / per);
}

void launch_s2_suppress(hipStream_t st, int n_img, long long max_pairs, const S2Img *imgs, const S2Cfg *cfg,
                        unsigned char *cand) {
  if (n_img > 0 && max_pairs > 0)
    hipLaunchKernelGGL(k_s2_suppress, dim3(pair_grid(max_pairs), (unsigned)n_img), dim3(kS2Block), 0, st, imgs, cfg, cand);
}

void launch_s2_score(hipStream_t st, int n_img, long long max_pairs, const S2Img *imgs, const S2Cfg *cfg,
                     const unsigned char *cand, unsigned char *det) {
  if (n_img > 0 && max_pairs > 0)
    hipLaunchKernelGGL(k_s2_score, dim3(pair_grid(max_pairs), (unsigned)n_img), dim3(kS2Block), 0, st, imgs, cfg, cand, det);
}

void launch_s2_compact(hipStream_t st, int n_img, const S2Img *imgs, const unsigned char *det, unsigned *list,
                       long long *seg_off) {
  if (n_img <= 0) return;
  hipLaunchKernelGGL(k_s2_compact, dim3((unsigned)n_img), dim3(kS2Block), 0, st, imgs, det, list, seg_off + 1);
  hipLaunchKernelGGL(k_s2_seg_offsets, dim3(1), dim3(1), 0, st, n_img, seg_off);
}

void launch_s2_refine_junc(hipStream_t st, int n_img, int grid, const S2Img *imgs, const S2Cfg *cfg, const unsigned *list,
                           const long long *seg_off, S2Seg *segs, int refine) {
  if (n_img > 0 && grid > 0)
    hipLaunchKernelGGL(k_s2_refine_junc, dim3((unsigned)grid), dim3(kS2Block), 0, st, n_img, imgs, cfg, list, seg_off, segs,
                       refine);
}

void launch_s2_descinfo(hipStream_t st, long long n_pts, int n_img, const float *pts, const long long *pt_off,
                        const long long *maps, const int *dims, const long long *outs) {
  const int per = kS2Block / kS2Wave;
  if (n_pts > 0)
    hipLaunchKernelGGL(k_s2_descinfo, dim3((unsigned)((n_pts + per - 1) / per)), dim3(kS2Block), 0, st, n_pts, n_img, pts,
                       pt_off, maps, dims, outs);
}

}  // namespace lt
