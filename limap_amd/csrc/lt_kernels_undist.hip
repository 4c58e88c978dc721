// lt_kernels_undist.hip -- device side of the undistortion (limap.undistortion).
//   k_undist_warp    the hot path: a whole batch of images, which may differ in size, channel count and camera, in one
//                    launch.  Work is divided over TARGET pixels and flattened over the batch: a work unit is a run of
//                    kUdRun consecutive target pixels of one row, a lane owns one unit and finds its image by binary
//                    search over the units' prefix (a 1x1 image beside a 4000x3000 one is one unit among three
//                    million).  The lane packs its run's bytes and writes them as whole dwords where the run is
//                    complete and starts on a dword: 4, 12 or 16 contiguous bytes per lane, 256 to 1024 contiguous
//                    bytes per wave and store instruction.  The four source taps are plain cached loads; neighbouring
//                    lanes read neighbouring source pixels, because the mapping is smooth.  Only the closed-form
//                    forward distortion runs per pixel.
//   k_undist_points  one lane per point: CamFromImg of the point's source camera (the Newton loop of
//                    ud_iterative_undistortion: every lane leaves on its own stop test), then ImgFromCam of its target
//                    camera; writes the point, the status and the iteration count.  Serves undistort_points, the
//                    scene-level call and the border scan of UndistortCamera.
// Every expression is lt_undist.h's; nothing here is atomic, so a result does not depend on scheduling.

#include "lt_undist.h"

namespace lt {

namespace {

template <int C>
__device__ __forceinline__ void warp_run(const UdCam &cs, const UdCam &ct, const UdImage &im,
                                         const unsigned char *__restrict__ src, unsigned char *__restrict__ dst, int y,
                                         int x0) {
  const int n = im.tw - x0 < kUdRun ? im.tw - x0 : kUdRun;
  const double v = ud_row_v(ct, y);
  unsigned px[kUdRun];
#pragma unroll
  for (int j = 0; j < kUdRun; ++j) px[j] = j < n ? ud_warp_pixel<C>(cs, ct, src, im.src_stride, im.sw, im.sh, x0 + j, v) : 0u;
  unsigned char *out = dst + (long long)y * im.dst_stride + (long long)x0 * C;
  if (n == kUdRun && (reinterpret_cast<unsigned long long>(out) & 3ull) == 0ull) {
    unsigned w[C];  // kUdRun * C bytes = C dwords (kUdRun == 4)
#pragma unroll
    for (int k = 0; k < C; ++k) w[k] = 0u;
#pragma unroll
    for (int j = 0; j < kUdRun; ++j)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int b = j * C + c;
        w[b >> 2] |= ((px[j] >> (8 * c)) & 0xffu) << (8 * (b & 3));
      }
    unsigned *o32 = reinterpret_cast<unsigned *>(out);
#pragma unroll
    for (int k = 0; k < C; ++k) o32[k] = w[k];
  } else {
#pragma unroll
    for (int j = 0; j < kUdRun; ++j)
      if (j < n) {
#pragma unroll
        for (int c = 0; c < C; ++c) out[j * C + c] = (unsigned char)((px[j] >> (8 * c)) & 0xffu);
      }
  }
}
static_assert(kUdRun == 4, "warp_run packs four pixels of C bytes into C dwords");

__global__ void __launch_bounds__(kUdBlock) k_undist_warp(long long n_units, int n_img,
                                                          const UdImage *__restrict__ imgs,
                                                          const UdCam *__restrict__ cams,
                                                          const unsigned char *__restrict__ src_base,
                                                          unsigned char *__restrict__ dst_base) {
  const long long unit = (long long)blockIdx.x * kUdBlock + threadIdx.x;
  if (unit >= n_units) return;
  int lo = 0, hi = n_img;  // the last image whose first unit is not beyond this one
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (imgs[mid].unit0 <= unit) lo = mid; else hi = mid;
  }
  const UdImage im = imgs[lo];
  const long long local = unit - im.unit0;
  const int runs = (im.tw + kUdRun - 1) / kUdRun;
  const int y = (int)(local / runs);
  const int x0 = (int)(local - (long long)y * runs) * kUdRun;
  if (y >= im.th) return;  // (cannot happen with the host's prefix; keeps every address inside the target regardless)
  const UdCam cs = cams[im.cam_src], ct = cams[im.cam_dst];
  const unsigned char *src = src_base + im.src_off;
  unsigned char *dst = dst_base + im.dst_off;
  if (im.ch == 1) warp_run<1>(cs, ct, im, src, dst, y, x0);
  else if (im.ch == 3) warp_run<3>(cs, ct, im, src, dst, y, x0);
  else if (im.ch == 4) warp_run<4>(cs, ct, im, src, dst, y, x0);
}

__global__ void __launch_bounds__(kUdBlock) k_undist_points(long long n, const UdCam *__restrict__ cams,
                                                            const double *__restrict__ xy,
                                                            const int *__restrict__ cam_src,
                                                            const int *__restrict__ cam_dst,
                                                            double *__restrict__ out_xy, int *__restrict__ status,
                                                            int *__restrict__ iters) {
  const long long i = (long long)blockIdx.x * kUdBlock + threadIdx.x;
  if (i >= n) return;
  const UdCam cs = cams[cam_src[i]], cd = cams[cam_dst[i]];
  double ox, oy;
  int it;
  const int st = ud_point(cs, cd, xy[2 * i], xy[2 * i + 1], ox, oy, it);
  out_xy[2 * i] = ox;
  out_xy[2 * i + 1] = oy;
  status[i] = st;
  iters[i] = it;
}

// the measurement's yardstick (tools/time_undist.py): 16 bytes per lane, nothing else
__global__ void __launch_bounds__(kUdBlock) k_undist_copy16(long long n16, const uint4 *__restrict__ src,
                                                            uint4 *__restrict__ dst) {
  const long long i = (long long)blockIdx.x * kUdBlock + threadIdx.x;
  if (i < n16) dst[i] = src[i];
}

inline unsigned grid_of(long long n) { return (unsigned)((n + kUdBlock - 1) / kUdBlock); }

}  // namespace

void launch_undist_warp(hipStream_t st, long long n_units, int n_img, const UdImage *imgs, const UdCam *cams,
                        const unsigned char *src_base, unsigned char *dst_base) {
  if (n_units <= 0) return;
  hipLaunchKernelGGL(k_undist_warp, dim3(grid_of(n_units)), dim3(kUdBlock), 0, st, n_units, n_img, imgs, cams, src_base,
                     dst_base);
}

void launch_undist_points(hipStream_t st, long long n, const UdCam *cams, const double *xy, const int *cam_src,
                          const int *cam_dst, double *out_xy, int *status, int *iters) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_undist_points, dim3(grid_of(n)), dim3(kUdBlock), 0, st, n, cams, xy, cam_src, cam_dst, out_xy,
                     status, iters);
}

void launch_undist_copy16(hipStream_t st, long long n16, const void *src, void *dst) {
  if (n16 <= 0) return;
  hipLaunchKernelGGL(k_undist_copy16, dim3(grid_of(n16)), dim3(kUdBlock), 0, st, n16, static_cast<const uint4 *>(src),
                     static_cast<uint4 *>(dst));
}

}  // namespace lt
