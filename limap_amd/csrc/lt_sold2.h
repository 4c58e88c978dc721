// lt_sold2.h -- records and every expression of the SOLD2 line detection from junctions and heatmaps (limap_amd.line2d;
// LineSegmentDetectionModule of line2d/SOLD2/model/line_detection.py, compute_descriptors of line_matching.py), shared
// by the host side (lt_sold2.cpp) and the device side (lt_kernels_sold2.hip).  DESIGN §23 is the definition; both sides
// compile the same inline functions with -ffp-contract=off, so every stage is the same bits on both.  FP32 with +, -,
// *, /, sqrtf, floorf, ceilf, rintf and comparisons only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lt {

constexpr int kS2Wave = 64;          // lanes of a wave: samples of a candidate, junctions of a suppression pass
constexpr int kS2MaxSamples = 64;    // one lane per sample
constexpr int kS2MaxPerturbs = 9;    // 9^4 perturbed segments per detected segment
constexpr int kS2MaxRadius = 4;      // local-max patch radius
constexpr int kS2MaxBlocks = 32;     // heatmap refinement blocks per axis
constexpr int kS2Block = 256;        // lanes per workgroup of every kernel
constexpr int kS2Tab = 128;          // junctions of one LDS table pass of the suppression
constexpr int kS2WinFloats = 12288;  // LDS heatmap window of the junction refinement (48 KB: three workgroups per CU)
constexpr int kS2MaxDim = 1 << 15;   // tallest / widest heatmap taken (pixel indexes stay inside 31 bits)

// the configuration as the kernels read it: thresholds already in FP32, as torch compares an FP32 tensor with a scalar
struct S2Cfg {
  float detect_thresh, inlier_thresh, lambda_radius, nms_tol, valid_thresh, patch_c;  // patch_c = float(0.5 * 2 ** 0.5)
  double ratio;
  int num_samples, bilinear, radius, num_perturbs, win_floats, pad_;
  float sampler[kS2MaxSamples];
  float perturb[kS2MaxPerturbs];
  float pad2_;
};

// one image of a scene.  heat / junc are device addresses (device side) or host addresses (host side); stage is the
// heatmap the stages 3 and 4 read: the refined copy, or the input where refinement is off
struct S2Img {
  const float *heat, *junc, *stage;
  float *refined;
  long long heat_stride, stage_stride;  // floats per row
  long long pair0, blk0;                // first pair and first refinement block of the image in the scene's arrays
  int n, H, W, nb;                      // junctions, heatmap size, refinement blocks per axis (0: refinement off)
  float diag;                           // float(sqrt(H^2 + W^2))
  int pad_;
  int r0[kS2MaxBlocks], r1[kS2MaxBlocks], c0[kS2MaxBlocks], c1[kS2MaxBlocks];  // row and column ranges of the blocks
};

// a detected segment after junction refinement
struct S2Seg {
  float h1, w1, h2, w2;
  int i, j, perturb, img;
};
static_assert(sizeof(S2Seg) == 32, "S2Seg layout");

#define LT_S2_HD __host__ __device__ __forceinline__

LT_S2_HD unsigned s2_bits(float x) {
  unsigned u;
  __builtin_memcpy(&u, &x, 4);
  return u;
}
LT_S2_HD float s2_clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
LT_S2_HD int s2_clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }
LT_S2_HD float s2_max(float a, float b) { return b > a ? b : a; }

// pairs i < j of n junctions in row-major order: pair p -> (i, j)
LT_S2_HD long long s2_pair_row0(long long n, long long i) { return i * (2 * n - i - 1) / 2; }
LT_S2_HD void s2_pair_decode(int n, long long p, int &i, int &j) {
  // i = the largest row whose first pair is <= p; the FP64 root is off by one at most
  const double b = 2.0 * n - 1.0;
  long long r = (long long)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
  if (r < 0) r = 0;
  if (r > n - 2) r = n - 2;
  while (r > 0 && s2_pair_row0(n, r) > p) --r;
  while (r < n - 2 && s2_pair_row0(n, r + 1) <= p) ++r;
  i = (int)r;
  j = (int)(p - s2_pair_row0(n, r)) + i + 1;
}

// ---- stage 1: heatmap refinement ----
// the value v > 0 as a multiple of 2^shift, truncated (exact whenever shift <= exponent(v) - 23)
LT_S2_HD unsigned long long s2_fixed(float v, int shift) {
  const unsigned u = s2_bits(v);
  const int ef = (int)((u >> 23) & 0xffu);
  const unsigned long long m = ef ? ((u & 0x7fffffu) | 0x800000u) : (u & 0x7fffffu);
  const int e = (ef ? ef : 1) - 150;  // v = m 2^e
  const int s = e - shift;
  if (s >= 0) return s >= 40 ? 0ull : (m << s);  // (s >= 40 cannot happen with the shift of s2_sum_shift)
  return -s >= 64 ? 0ull : (m >> (-s));
}
// the quantum of a block's top-share sum: the ulp of the smallest value that counts, unless count values up to the
// block's maximum would pass 2^63 in it
LT_S2_HD int s2_sum_shift(float valid_thresh, float vmax, long long count) {
  const unsigned ut = s2_bits(valid_thresh), um = s2_bits(vmax);
  const int et = (int)((ut >> 23) & 0xffu), em = (int)((um >> 23) & 0xffu);
  const int exact = (et ? et : 1) - 150;  // values above valid_thresh are multiples of 2^exact
  int lg = 0;
  while ((1ll << lg) < count) ++lg;
  const int room = (em ? em : 1) - 126 + lg - 63;  // count * vmax < 2^(em - 126 + lg)
  return exact > room ? exact : room;
}
// mean of the k largest values from the fixed-point sum: FP64 product and quotient, rounded to FP32 once
LT_S2_HD float s2_scale(unsigned long long sum, int shift, long long k) {
  double s = (double)sum;
  int sh = shift;
  while (sh > 0) { s *= 2.0; --sh; }
  while (sh < 0) { s *= 0.5; ++sh; }
  return (float)(s / (double)k);
}

// the refined pixel: blocks in the reference's loop order (row blocks outer, column blocks inner); scale < 0 marks a
// block whose maximum is not above valid_thresh
LT_S2_HD float s2_refined_pixel(const S2Img &im, const float *scales, int y, int x, float h) {
  float acc = 0.f;
  int cnt = 0;
  for (int a = 0; a < im.nb; ++a) {
    if (y < im.r0[a] || y >= im.r1[a]) continue;
    for (int b = 0; b < im.nb; ++b) {
      if (x < im.c0[b] || x >= im.c1[b]) continue;
      const float sc = scales[im.blk0 + (long long)a * im.nb + b];
      acc = acc + (sc < 0.f ? h : s2_clampf(h / sc, 0.f, 1.f));
      ++cnt;
    }
  }
  return s2_clampf(acc / (float)cnt, 0.f, 1.f);
}

// ---- stage 2: candidate suppression ----
// does junction k (kh, kw) suppress the candidate (ih, iw) - (jh, jw)?  k is neither i nor j.
LT_S2_HD bool s2_suppresses(float ih, float iw, float jh, float jw, float kh, float kw, float tol) {
  const float d0 = jh - ih, d1 = jw - iw;
  const float c0 = kh - ih, c1 = kw - iw;
  if (c0 == 0.f && c1 == 0.f) return false;  // the reference's acos(0 / 0): NaN, never counted
  const float len2 = d0 * d0 + d1 * d1;
  const float len = sqrtf(len2);
  const float dot = c0 * d0 + c1 * d1;
  const float proj = dot / len2;  // NaN for a candidate of length 0: nothing suppresses it
  const float cross = c0 * d1 - c1 * d0;
  const float dist = (cross < 0.f ? -cross : cross) / len;
  return proj >= 0.f && proj <= 1.f && dist <= tol;
}

// ---- stages 3 and 4: sampling ----
// (a position that is not a number goes to 0: it indexes the heatmap)
LT_S2_HD float s2_sample_pos(float start, float end, float s, float hi) {
  const float v = start * s + end * (1.0f - s);
  return !(v >= 0.f) ? 0.f : (v > hi ? hi : v);
}
LT_S2_HD bool s2_finite(float x) { return (s2_bits(x) & 0x7f800000u) != 0x7f800000u; }

// the reference's bilinear form: both weights of an integer coordinate are 0
template <class Heat>
LT_S2_HD float s2_bilinear(const Heat &heat, float h, float w) {
  const float hf = floorf(h), hc = ceilf(h), wf = floorf(w), wc = ceilf(w);
  const int yf = (int)hf, yc = (int)hc, xf = (int)wf, xc = (int)wc;
  return heat(yf, xf) * (hc - h) * (wc - w) + heat(yf, xc) * (hc - h) * (w - wf) + heat(yc, xf) * (h - hf) * (wc - w) +
         heat(yc, xc) * (h - hf) * (w - wf);
}

template <class Heat>
LT_S2_HD float s2_local_max(const Heat &heat, float h, float w, int H, int W, int radius, float dist_thresh) {
  const float rh = rintf(h), rw = rintf(w);
  float best = 0.f;  // a masked patch point counts as 0
  for (int dh = -radius; dh <= radius; ++dh)
    for (int dw = -radius; dw <= radius; ++dw) {
      if (dh * dh + dw * dw > radius * radius) continue;
      const float ph = rh + (float)dh, pw = rw + (float)dw;
      const float eh = h - ph, ew = w - pw;
      const float dist = sqrtf(eh * eh + ew * ew);
      const float v = heat(s2_clampi((int)ph, 0, H - 1), s2_clampi((int)pw, 0, W - 1));
      best = s2_max(best, dist < dist_thresh ? v : 0.f);
    }
  return best;
}

LT_S2_HD float s2_dist_thresh(const S2Cfg &c, float sh, float sw, float eh, float ew, float diag) {
  const float a = sh - eh, b = sw - ew;
  const float len = sqrtf(a * a + b * b);
  return c.patch_c + c.lambda_radius * (len / diag);
}

// the fixed summation tree of a wave: level off adds lane l + off to lane l, off = 32 .. 1 (host form over 64 slots)
inline float s2_tree_sum_host(float *v) {
  for (int off = 32; off >= 1; off >>= 1)
    for (int l = 0; l < off; ++l) v[l] = v[l] + v[l + off];
  return v[0];
}

// a perturbation index -> the perturbed, clamped segment (the reference's meshgrid order)
LT_S2_HD void s2_perturbed(const S2Cfg &c, int idx, float sh, float sw, float eh, float ew, int H, int W, float out[4]) {
  const int P = c.num_perturbs;
  const int d = idx % P, cc = (idx / P) % P, b = (idx / (P * P)) % P, a = idx / (P * P * P);
  out[0] = s2_clampf(sh + c.perturb[a], 0.f, (float)(H - 1));
  out[1] = s2_clampf(sw + c.perturb[b], 0.f, (float)(W - 1));
  out[2] = s2_clampf(eh + c.perturb[cc], 0.f, (float)(H - 1));
  out[3] = s2_clampf(ew + c.perturb[d], 0.f, (float)(W - 1));
}

// the score of a perturbed segment: bilinear samples summed left to right, divided by their number
template <class Heat>
LT_S2_HD float s2_perturb_score(const S2Cfg &c, const Heat &heat, const float seg[4], int H, int W) {
  float acc = 0.f;
  for (int s = 0; s < c.num_samples; ++s) {
    const float h = s2_sample_pos(seg[0], seg[2], c.sampler[s], (float)(H - 1));
    const float w = s2_sample_pos(seg[1], seg[3], c.sampler[s], (float)(W - 1));
    acc = acc + s2_bilinear(heat, h, w);
  }
  return acc / (float)c.num_samples;
}

struct S2HeatGlobal {
  const float *p;
  long long stride;
  LT_S2_HD float operator()(int y, int x) const { return p[(long long)y * stride + x]; }
};

// ---- descriptor sampling (compute_descriptors): grid_sample, bilinear, zero padding, align_corners=False ----
// pixel coordinate of the descriptor map for an image coordinate v of an image of size `img` (= map size * grid_size)
LT_S2_HD float s2_desc_coord(float v, float img, int size) {
  const float g = v * 2.0f / img - 1.0f;
  return ((g + 1.0f) * (float)size - 1.0f) / 2.0f;
}
// one channel at (iy, ix): map is channel-last (Hd, Wd, C)
LT_S2_HD float s2_desc_tap(const float *map, int Hd, int Wd, int C, int y, int x, int c) {
  return (y >= 0 && y < Hd && x >= 0 && x < Wd) ? map[((long long)y * Wd + x) * C + c] : 0.f;
}
LT_S2_HD float s2_desc_sample(const float *map, int Hd, int Wd, int C, float iy, float ix, int c) {
  const float y0 = floorf(iy), x0 = floorf(ix);
  const float y1 = y0 + 1.0f, x1 = x0 + 1.0f;
  const float nw = (x1 - ix) * (y1 - iy), ne = (ix - x0) * (y1 - iy), sw = (x1 - ix) * (iy - y0), se = (ix - x0) * (iy - y0);
  const int yi = (int)y0, xi = (int)x0;
  return s2_desc_tap(map, Hd, Wd, C, yi, xi, c) * nw + s2_desc_tap(map, Hd, Wd, C, yi, xi + 1, c) * ne +
         s2_desc_tap(map, Hd, Wd, C, yi + 1, xi, c) * sw + s2_desc_tap(map, Hd, Wd, C, yi + 1, xi + 1, c) * se;
}

// launch wrappers (lt_kernels_sold2.hip)
void launch_s2_block_scale(hipStream_t st, long long n_blocks, const S2Img *imgs, const int *blk_img, const S2Cfg *cfg,
                           float *scales);
void launch_s2_refine_pixels(hipStream_t st, int n_img, int max_pixels_blocks, const S2Img *imgs, const float *scales);
void launch_s2_suppress(hipStream_t st, int n_img, long long max_pairs, const S2Img *imgs, const S2Cfg *cfg,
                        unsigned char *cand);
void launch_s2_score(hipStream_t st, int n_img, long long max_pairs, const S2Img *imgs, const S2Cfg *cfg,
                     const unsigned char *cand, unsigned char *det);
void launch_s2_compact(hipStream_t st, int n_img, const S2Img *imgs, const unsigned char *det, unsigned *list,
                       long long *seg_off);
void launch_s2_refine_junc(hipStream_t st, int n_img, int grid, const S2Img *imgs, const S2Cfg *cfg, const unsigned *list,
                           const long long *seg_off, S2Seg *segs, int refine);
void launch_s2_descinfo(hipStream_t st, long long n_pts, int n_img, const float *pts, const long long *pt_off,
                        const long long *maps, const int *dims, const long long *outs);

}  // namespace lt
