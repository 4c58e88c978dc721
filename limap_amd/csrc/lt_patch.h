// lt_patch.h -- records and every expression of the line patch extraction (limap.features: line_patch_extractor.cc,
// featurepatch.h over ceresbase/interpolation.h's BiLinearInterpolator), shared by the host side (lt_patch.cpp) and the
// device side (lt_kernels_patch.hip).  DESIGN §24 is the definition; both sides compile the same inline functions with
// -ffp-contract=off, so a texel is the same bits on both.  Only +, -, *, /, sqrt, floor, ceil and trunc on FP64, exact
// widenings of the input texels and one rounding to the output type.
#pragma once

#include "lt_geom.h"

#include <cstdint>

namespace lt {

constexpr int kPtBlock = 256;          // lanes per workgroup of k_patch_gather
constexpr int kPtBlockItems = 2048;    // lane items (one texel's channel group each) a block-table entry aims at
constexpr int kPtMaxH = 1 << 20;       // tallest patch taken (rows along the line)
constexpr int kPtMaxPerp = 1 << 12;    // widest range_perp taken
constexpr int kPtF16 = 0, kPtF32 = 1, kPtF64 = 2;  // LT_PATCH_F16 / _F32 / _F64

// geometry of one patch: R = [perp; direc] (rows), tvec = corner, h rows along the line (w = range_perp + 1 of all)
struct PtGeom {
  double R[4];
  double tvec[2];
  int h, pad_;
};
static_assert(sizeof(PtGeom) == 56, "PtGeom layout");

// one patch of a launch: its geometry and the first element of its (h, w, c) array in the packed output
struct PtPatch {
  double px, py, dx, dy, cx, cy;  // perp, direc, corner
  long long out_off;
  int h, pad_;
};
static_assert(sizeof(PtPatch) == 64, "PtPatch layout");

// one entry of the block table: rows [y0, y0 + rows) of patch `patch`
struct PtBlock {
  int patch, y0, rows, pad_;
};
static_assert(sizeof(PtBlock) == 16, "PtBlock layout");

// the feature map as the gather reads it: strides in elements
struct PtMap {
  const void *ptr;
  long long row_stride, pix_stride, chan_stride;
  int h, w, c, dtype;
};

#define LT_PT_HD __host__ __device__ __forceinline__

LT_PT_HD bool pt_finite(double x) {
  unsigned long long u;
  __builtin_memcpy(&u, &x, 8);
  return (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// std::round of a value that is not negative: halves go up
LT_PT_HD double pt_round(double v) {
  double r = __builtin_trunc(v);
  if (v - r >= 0.5) r += 1.0;
  return r;
}

// ExtractLinePatch's geometry (line_patch_extractor.cc:24-46).  hd is round(|e2 - s2|) + 1 as a double: the caller
// refuses what does not fit before it converts.
LT_PT_HD void pt_geometry(double x1, double y1, double x2, double y2, double k_stretch, int t_stretch, int range_perp,
                          PtGeom &g, double &hd) {
  const d2 s{x1, y1}, e{x2, y2};
  const d2 d = sub(e, s);
  const double L = sqrt(d.x * d.x + d.y * d.y);
  const d2 direc = unit(d);  // d / L, d itself for L == 0
  const d2 perp{direc.y, -direc.x};
  const d2 mid{0.5 * (s.x + e.x), 0.5 * (s.y + e.y)};
  const double fl = __builtin_ceil(dmax(L * k_stretch, L + (double)t_stretch));  // std::max(a, b)
  const d2 s2{mid.x - direc.x * fl / 2.0, mid.y - direc.y * fl / 2.0};
  const d2 e2{mid.x + direc.x * fl / 2.0, mid.y + direc.y * fl / 2.0};
  const double rp = (double)range_perp;
  const d2 corner{s2.x - perp.x * rp / 2.0, s2.y - perp.y * rp / 2.0};
  const d2 dd = sub(s2, e2);  // Line2d::length(): (start - end).norm()
  hd = pt_round(sqrt(dd.x * dd.x + dd.y * dd.y)) + 1.0;
  g.R[0] = perp.x; g.R[1] = perp.y; g.R[2] = direc.x; g.R[3] = direc.y;
  g.tvec[0] = corner.x; g.tvec[1] = corner.y;
  g.h = 0;
  g.pad_ = 0;
}

// R^T (x, y) + corner: the products summed left to right, then the corner
LT_PT_HD void pt_global(const PtPatch &p, int x, int y, double &gx, double &gy) {
  gx = (p.px * (double)x + p.dx * (double)y) + p.cx;
  gy = (p.py * (double)x + p.dy * (double)y) + p.cy;
}

// Grid2D's clamp of a floor that is still a double, then the conversion (a NaN, which the host's checks exclude, is 0)
LT_PT_HD int pt_clamp(double v, int n) {
  const double hi = (double)(n - 1);
  return !(v > 0.0) ? 0 : (v > hi ? n - 1 : (int)v);
}

// the four texels and the two weights of BiLinearInterpolator::Evaluate(r = gy, c = gx)
struct PtTaps {
  int r0, r1, c0, c1;
  double dx, dy;
};
LT_PT_HD PtTaps pt_taps(double gx, double gy, int H, int W) {
  const double row = __builtin_floor(gy), col = __builtin_floor(gx);
  PtTaps t;
  t.dy = gy - row;
  t.dx = gx - col;
  t.r0 = pt_clamp(row, H);
  t.r1 = pt_clamp(row + 1.0, H);
  t.c0 = pt_clamp(col, W);
  t.c1 = pt_clamp(col + 1.0, W);
  return t;
}
LT_PT_HD double pt_blend(double dx, double dy, double ll, double lr, double ul, double ur) {
  const double v0 = (1.0 - dx) * ll + dx * lr;
  const double v1 = (1.0 - dx) * ul + dx * ur;
  return (1.0 - dy) * v0 + dy * v1;
}

// ---- widening of a binary16 texel (exact) ----
LT_PT_HD double pt_half_bits_to_double(unsigned short h) {
#if defined(__HIP_DEVICE_COMPILE__)
  _Float16 v;
  __builtin_memcpy(&v, &h, 2);
  return (double)(float)v;
#else
  const unsigned long long sign = (unsigned long long)(h & 0x8000u) << 48;
  const unsigned e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  unsigned long long u;
  if (e == 0x1fu) {
    u = sign | 0x7ff0000000000000ull | ((unsigned long long)m << 42);
  } else if (e != 0u) {
    u = sign | ((unsigned long long)(e + 1008u) << 52) | ((unsigned long long)m << 42);
  } else if (m == 0u) {
    u = sign;
  } else {  // subnormal: m * 2^-24
    int k = 0;
    unsigned mm = m;
    while (!(mm & 0x400u)) { mm <<= 1; ++k; }
    u = sign | ((unsigned long long)(1009 - k) << 52) | ((unsigned long long)(mm & 0x3ffu) << 42);
  }
  double d;
  __builtin_memcpy(&d, &u, 8);
  return d;
#endif
}

// ---- narrowing of the FP64 result: ONE rounding to nearest-even ----
// binary16 (the hardware has no double-to-half conversion; through float would round twice).  The host works on the
// bits: the 53-bit significand is cut at the half's quantum -- 2^(E - 10) for a normal result, 2^-24 below 2^-14 -- and rounded on the
// remainder; a carry runs into the exponent field, 65520 and above become infinity.  A NaN keeps its sign and the top
// of its payload and stays a NaN, as NumPy's conversion does.
LT_PT_HD unsigned short pt_double_to_half_bits(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  // The device reaches the same value with a quarter of the instructions: round-to-odd into float, then the hardware's
  // float-to-half conversion.  A float keeps 24 bits where a half keeps 11, so the sticky last bit of the odd rounding
  // decides every tie of the second rounding the way the exact value would: the result is the single rounding of v.
  float f = (float)v;
  const double back = (double)f;
  if (back != v && v == v) {  // inexact: the truncation toward zero with its last bit set
    unsigned w;
    __builtin_memcpy(&w, &f, 4);
    if (__builtin_fabs(back) > __builtin_fabs(v)) w -= 1u;  // (an infinity steps back to the largest float)
    w |= 1u;
    __builtin_memcpy(&f, &w, 4);
  }
  const _Float16 hv = (_Float16)f;
  unsigned short hb;
  __builtin_memcpy(&hb, &hv, 2);
  return hb;
#else
  unsigned long long u;
  __builtin_memcpy(&u, &v, 8);
  const unsigned sign = (unsigned)(u >> 48) & 0x8000u;
  const int e = (int)((u >> 52) & 0x7ffull);
  const unsigned long long m = u & 0x000fffffffffffffull;
  if (e == 0x7ff) {
    if (m == 0ull) return (unsigned short)(sign | 0x7c00u);
    unsigned r = 0x7c00u + (unsigned)(m >> 42);
    if (r == 0x7c00u) r += 1u;
    return (unsigned short)(sign | r);
  }
  const int E = e - 1023;
  if (E >= 16) return (unsigned short)(sign | 0x7c00u);
  if (e == 0) return (unsigned short)sign;
  const int shift = E >= -14 ? 42 : 42 + (-14 - E);
  if (shift >= 54) return (unsigned short)sign;  // below half of the smallest subnormal
  const unsigned long long sig = m | 0x0010000000000000ull;
  unsigned long long q = sig >> shift;
  const unsigned long long rem = sig & ((1ull << shift) - 1ull), half = 1ull << (shift - 1);
  if (rem > half || (rem == half && (q & 1ull))) q += 1ull;
  unsigned hbits = E >= -14 ? (unsigned)((unsigned long long)(E + 14) << 10) + (unsigned)q : (unsigned)q;
  if (hbits >= 0x7c00u) hbits = 0x7c00u;
  return (unsigned short)(sign | hbits);
#endif
}
// binary32: the conversion instruction of either side rounds once, to nearest-even
LT_PT_HD float pt_double_to_float(double v) { return (float)v; }

// ---- GetLine2DRange (line_patch_extractor.cc:143-170) ----
// the projection g of the 3D line and, over the n supports seg4[k] = (x1, y1, x2, y2), the range on it.  Returns 0, 1
// without a support, 2 when an endpoint is not in front of the camera or a coordinate of the range is not finite.
LT_PT_HD int pt_range(const Cam &cam, const double line6[6], long long n, const double *seg4, const int *sup_img,
                      int image_id, double out4[4]) {
  const d3 p0{line6[0], line6[1], line6[2]}, p1{line6[3], line6[4], line6[5]};
  const d2 gs = cam_project(cam, p0), ge = cam_project(cam, p1);
  const d2 u = unit(sub(ge, gs));
  bool any = false;
  double lo = 0.0, hi = 0.0;
  for (long long k = 0; k < n; ++k) {
    if (sup_img[k] != image_id) continue;
    const double a = dot(sub(mk2(seg4[4 * k], seg4[4 * k + 1]), gs), u);
    const double b = dot(sub(mk2(seg4[4 * k + 2], seg4[4 * k + 3]), gs), u);
    if (!any) { lo = hi = a; any = true; }
    if (a < lo) lo = a;
    if (hi < a) hi = a;
    if (b < lo) lo = b;
    if (hi < b) hi = b;
  }
  out4[0] = out4[1] = out4[2] = out4[3] = 0.0;
  if (!any) return 1;
  const d2 dd = sub(gs, ge);
  const double len = sqrt(dd.x * dd.x + dd.y * dd.y);
  const double a = dmax(0.0, lo), b = dmin(len, hi);  // std::max(0.0, min), std::min(g.length(), max)
  out4[0] = gs.x + u.x * a;
  out4[1] = gs.y + u.y * a;
  out4[2] = gs.x + u.x * b;
  out4[3] = gs.y + u.y * b;
  if (!(cam_depth(cam, p0) > 0.0) || !(cam_depth(cam, p1) > 0.0)) return 2;
  for (int k = 0; k < 4; ++k)
    if (!pt_finite(out4[k])) return 2;
  return 0;
}

// launch wrapper of lt_kernels_patch.hip: all patches of one feature map in one launch.  vec != 0: the vector form
// (the caller has checked chan_stride == 1, c a multiple of the lane's channel count, 16-byte alignment of the base, the
// row and the pixel stride).  out: the packed output of the launch's patches.
void launch_patch_gather(hipStream_t st, const PtMap &map, int out_dtype, int vec, int patch_w, int n_blocks,
                         const PtBlock *blocks, const PtPatch *patches, void *out);
// the yardstick of the measurement (tools/time_patch.py): a copy of n16 16-byte items, one per lane
void launch_patch_copy16(hipStream_t st, long long n16, const void *src, void *dst);

}  // namespace lt
