// lt_undist.h -- records and every expression of the undistortion (limap.undistortion over COLMAP's camera models,
// UndistortCamera, WarpImageBetweenCameras and Bitmap::InterpolateBilinear), shared by the host side (lt_undist.cpp,
// lt_undist_host.cpp) and the device side (lt_kernels_undist.hip).  DESIGN §22 is the definition; both sides compile
// the same inline functions with -ffp-contract=off, so a pixel, a point, a status and an iteration count are the
// same bits on both.  Only +, -, *, /, comparisons, floor and trunc on FP64: nothing here calls a math library.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lt {

constexpr int kUdBlock = 256;     // lanes per workgroup of both kernels
constexpr int kUdRun = 4;         // consecutive target pixels of one row a lane of k_undist_warp owns
constexpr int kUdMaxIter = 100;   // COLMAP's kNumIterations of IterativeUndistortion
constexpr int kUdMaxDim = 1 << 20;  // widest / tallest image taken (row offsets stay far inside 63 bits)
constexpr unsigned long long kUdNaNBits = 0x7ff8000000000000ull;  // the canonical quiet NaN of a failed point

// COLMAP model ids
constexpr int kUdSimplePinhole = 0, kUdPinhole = 1, kUdSimpleRadial = 2, kUdRadial = 3, kUdOpenCV = 4,
              kUdFullOpenCV = 6;

// one camera of the per-camera table: the model and its parameters, the focal lengths and the principal point
// brought into one form (a single focal length stands in both), the other parameters in COLMAP's order
struct UdCam {
  int model, pad_;
  double fx, fy, cx, cy;
  double k[8];
};
static_assert(sizeof(UdCam) == 104, "UdCam layout");

// one image of a warp batch: byte offsets of the source and the target from the bases the kernel is given, both
// sizes, the channel count, the row strides in bytes, the source and target cameras' rows of the camera table, and
// the first of the image's work units (a unit is a run of kUdRun target pixels of one row)
struct UdImage {
  long long src_off, dst_off, src_stride, dst_stride, unit0;
  int sw, sh, tw, th, ch, cam_src, cam_dst, pad_;
};
static_assert(sizeof(UdImage) == 72, "UdImage layout");

#define LT_UD_HD __host__ __device__ __forceinline__

LT_UD_HD bool ud_finite(double x) {
  unsigned long long u;
  __builtin_memcpy(&u, &x, 8);
  return (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
LT_UD_HD double ud_nan() {
  const unsigned long long u = kUdNaNBits;
  double x;
  __builtin_memcpy(&x, &u, 8);
  return x;
}

LT_UD_HD bool ud_is_pinhole(int model) { return model == kUdSimplePinhole || model == kUdPinhole; }

// the forward distortion of the normalised point (u, v): (du, dv), in the operation order DESIGN §22 writes down
LT_UD_HD void ud_distortion(const UdCam &c, double u, double v, double &du, double &dv) {
  if (c.model == kUdSimpleRadial) {
    const double r2 = u * u + v * v;
    const double rad = c.k[0] * r2;
    du = u * rad;
    dv = v * rad;
  } else if (c.model == kUdRadial) {
    const double r2 = u * u + v * v;
    const double rad = c.k[0] * r2 + c.k[1] * r2 * r2;
    du = u * rad;
    dv = v * rad;
  } else if (c.model == kUdOpenCV) {
    const double u2 = u * u, uv = u * v, v2 = v * v;
    const double r2 = u2 + v2;
    const double rad = c.k[0] * r2 + c.k[1] * r2 * r2;
    du = u * rad + 2.0 * c.k[2] * uv + c.k[3] * (r2 + 2.0 * u2);
    dv = v * rad + 2.0 * c.k[3] * uv + c.k[2] * (r2 + 2.0 * v2);
  } else if (c.model == kUdFullOpenCV) {
    const double u2 = u * u, uv = u * v, v2 = v * v;
    const double r2 = u2 + v2;
    const double r4 = r2 * r2;
    const double r6 = r4 * r2;
    const double rad = (1.0 + c.k[0] * r2 + c.k[1] * r4 + c.k[4] * r6) / (1.0 + c.k[5] * r2 + c.k[6] * r4 + c.k[7] * r6);
    du = u * rad + 2.0 * c.k[2] * uv + c.k[3] * (r2 + 2.0 * u2) - u;
    dv = v * rad + 2.0 * c.k[3] * uv + c.k[2] * (r2 + 2.0 * v2) - v;
  } else {
    du = 0.0;
    dv = 0.0;
  }
}

LT_UD_HD void ud_img_from_cam(const UdCam &c, double u, double v, double &x, double &y) {
  double du, dv;
  ud_distortion(c, u, v, du, dv);
  x = c.fx * (u + du) + c.cx;
  y = c.fy * (v + dv) + c.cy;
}

// J d = r for the 2x2 J by elimination with partial pivoting: the rows are exchanged when |J10| > |J00| (a tie keeps
// them), then m = J10 / J00, d1 = (r1 - m r0) / (J11 - m J01), d0 = (r0 - J01 d1) / J00.  A singular J divides by
// zero and gives a result that is not finite; the caller tests for that.
LT_UD_HD void ud_solve2(double j00, double j01, double j10, double j11, double r0, double r1, double &d0, double &d1) {
  if (__builtin_fabs(j10) > __builtin_fabs(j00)) {
    double t = j00; j00 = j10; j10 = t;
    t = j01; j01 = j11; j11 = t;
    t = r0; r0 = r1; r1 = t;
  }
  const double m = j10 / j00;
  const double a = j11 - m * j01;
  const double b = r1 - m * r0;
  d1 = b / a;
  d0 = (r0 - j01 * d1) / j00;
}

LT_UD_HD double ud_step(double x) {
  const double s = __builtin_fabs(1e-6 * x);
  return s > 2.220446049250313080847263336181640625e-16 ? s : 2.220446049250313080847263336181640625e-16;
}

// COLMAP's IterativeUndistortion from (u0, v0): -> status (0, or 1 with (u, v) the canonical NaN); iters is the number
// of Newton updates made.  The loop ends after the update whose squared length is below 1e-10, after kUdMaxIter
// updates, or after an update that is not finite.
LT_UD_HD int ud_iterative_undistortion(const UdCam &c, double u0, double v0, double &u, double &v, int &iters) {
  double x = u0, y = v0;
  int it = 0;
  bool bad = false;
  while (it < kUdMaxIter) {
    const double sx = ud_step(x), sy = ud_step(y);
    double dx, dy, dx0b, dy0b, dx0f, dy0f, dx1b, dy1b, dx1f, dy1f;
    ud_distortion(c, x, y, dx, dy);
    ud_distortion(c, x - sx, y, dx0b, dy0b);
    ud_distortion(c, x + sx, y, dx0f, dy0f);
    ud_distortion(c, x, y - sy, dx1b, dy1b);
    ud_distortion(c, x, y + sy, dx1f, dy1f);
    const double j00 = 1.0 + (dx0f - dx0b) / (2.0 * sx);
    const double j01 = (dx1f - dx1b) / (2.0 * sy);
    const double j10 = (dy0f - dy0b) / (2.0 * sx);
    const double j11 = 1.0 + (dy1f - dy1b) / (2.0 * sy);
    double d0, d1;
    ud_solve2(j00, j01, j10, j11, x + dx - u0, y + dy - v0, d0, d1);
    x -= d0;
    y -= d1;
    ++it;
    if (!ud_finite(d0) || !ud_finite(d1)) { bad = true; break; }
    if (d0 * d0 + d1 * d1 < 1e-10) break;
  }
  iters = it;
  if (bad || !ud_finite(x) || !ud_finite(y)) {
    u = ud_nan();
    v = ud_nan();
    return 1;
  }
  u = x;
  v = y;
  return 0;
}

LT_UD_HD int ud_cam_from_img(const UdCam &c, double x, double y, double &u, double &v, int &iters) {
  const double u0 = (x - c.cx) / c.fx, v0 = (y - c.cy) / c.fy;
  iters = 0;
  if (ud_is_pinhole(c.model)) {
    u = u0;
    v = v0;
    if (ud_finite(u) && ud_finite(v)) return 0;
    u = ud_nan();
    v = ud_nan();
    return 1;
  }
  return ud_iterative_undistortion(c, u0, v0, u, v, iters);
}

// UndistortPoint: the source camera's CamFromImg, then the target camera's ImgFromCam
LT_UD_HD int ud_point(const UdCam &src, const UdCam &dst, double x, double y, double &ox, double &oy, int &iters) {
  double u, v;
  int st = ud_cam_from_img(src, x, y, u, v, iters);
  if (st == 0) {
    ud_img_from_cam(dst, u, v, ox, oy);
    if (!ud_finite(ox) || !ud_finite(oy)) st = 1;
  }
  if (st != 0) {
    ox = ud_nan();
    oy = ud_nan();
  }
  return st;
}

// round (halves away from zero) of a value that is not negative, clamped to [0, 255]
LT_UD_HD unsigned ud_round_u8(double val) {
  double r = __builtin_trunc(val);
  if (val - r >= 0.5) r += 1.0;
  if (!(r >= 0.0)) r = 0.0;
  if (r > 255.0) r = 255.0;
  return (unsigned)(int)r;
}

// The target pixel (x, y) of a warp, its C channels packed into one word (channel c in bits 8 c ..): v is the row's
// normalised ordinate (y + 0.5 - cy) / fy of the target camera.  The in-range test is made on the doubles, before any
// conversion to an integer, so no address is formed from an unchecked coordinate.
template <int C>
LT_UD_HD unsigned ud_warp_pixel(const UdCam &cs, const UdCam &ct, const unsigned char *src, long long stride, int sw,
                                int sh, int x, double v) {
  const double u = ((double)x + 0.5 - ct.cx) / ct.fx;
  double px, py;
  ud_img_from_cam(cs, u, v, px, py);
  const double sx = px - 0.5, sy = py - 0.5;
  if (!(ud_finite(sx) && ud_finite(sy) && sx >= 0.0 && sx < (double)(sw - 1) && sy >= 0.0 && sy < (double)(sh - 1)))
    return 0u;
  const double fx0 = __builtin_floor(sx), fy0 = __builtin_floor(sy);
  const double dx = sx - fx0, dy = sy - fy0;
  const unsigned char *p0 = src + (long long)(int)fy0 * stride + (long long)(int)fx0 * C;
  const unsigned char *p1 = p0 + stride;
  unsigned out = 0u;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double v00 = (double)p0[c], v10 = (double)p0[C + c], v01 = (double)p1[c], v11 = (double)p1[C + c];
    const double val = (1.0 - dy) * ((1.0 - dx) * v00 + dx * v10) + dy * ((1.0 - dx) * v01 + dx * v11);
    out |= ud_round_u8(val) << (8 * c);
  }
  return out;
}

LT_UD_HD double ud_row_v(const UdCam &ct, int y) { return ((double)y + 0.5 - ct.cy) / ct.fy; }

// launch wrappers of lt_kernels_undist.hip
void launch_undist_warp(hipStream_t st, long long n_units, int n_img, const UdImage *imgs, const UdCam *cams,
                        const unsigned char *src_base, unsigned char *dst_base);
void launch_undist_points(hipStream_t st, long long n, const UdCam *cams, const double *xy, const int *cam_src,
                          const int *cam_dst, double *out_xy, int *status, int *iters);
// the yardstick of the warp's measurement: a copy of n16 16-byte items, one per lane
void launch_undist_copy16(hipStream_t st, long long n16, const void *src, void *dst);

}  // namespace lt
