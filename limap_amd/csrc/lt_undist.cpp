// lt_undist.cpp -- limap.undistortion (undistortion/undistort.{cc,py} over COLMAP's UndistortImage): the device path.
// DESIGN §22 is the definition.  lt_undist_warp undistorts a batch of images in one launch of k_undist_warp,
// lt_undist_points a set of points with one lane each (lt_kernels_undist.hip); the host path from the same inline
// expressions of lt_undist.h and the validation are in lt_undist_host.cpp.

#include "lt_host.h"
#include "lt_undist_host.h"

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

using namespace lt;
using namespace lt_impl;

namespace {

inline long long round_up(long long v, long long a) { return (v + a - 1) / a * a; }

}  // namespace

extern "C" {

int lt_undist_warp(lt_ctx *ctx, int n_cam, const lt_undist_camera *cams, int n_img, const lt_undist_image *imgs) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::string who = "lt_undist_warp: ";
  std::vector<UdCam> table;
  UdBatch batch;
  std::string msg;
  double t0 = now_ms();
  if (ud_prepare_cams(n_cam, cams, table, msg) || ud_prepare_images(table, n_img, imgs, batch, msg))
    return fail(ctx, LT_ERR_ARGUMENT, who + msg);
  lt_host::UdState &ud = ctx->ud;
  for (double &t : ud.timers) t = 0.0;
  if (n_img == 0) return LT_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;

  // ---- layout: device images are used in place (their offsets are their addresses, from a null base); host images are
  // packed behind one another, every image on a 16-byte boundary, the target rows padded to whole dwords ----
  long long src_bytes = 0, dst_bytes = 0;
  for (int i = 0; i < n_img; ++i) {
    UdImage &u = batch.imgs[(size_t)i];
    if (batch.on_device) {
      u.src_off = (long long)reinterpret_cast<uintptr_t>(imgs[i].src);
      u.dst_off = (long long)reinterpret_cast<uintptr_t>(imgs[i].dst);
    } else {
      u.src_off = src_bytes;
      u.dst_off = dst_bytes;
      u.src_stride = (long long)u.sw * u.ch;
      u.dst_stride = round_up((long long)u.tw * u.ch, 4);
      src_bytes = round_up(src_bytes + u.src_stride * u.sh, 16);
      dst_bytes = round_up(dst_bytes + u.dst_stride * u.th, 16);
    }
  }
  if (int rc = upload_vec(ctx, ud.d_cams, table)) return rc;
  if (int rc = upload_vec(ctx, ud.d_imgs, batch.imgs)) return rc;
  if (!batch.on_device) {
    ud.h_in.resize((size_t)src_bytes);
    for (int i = 0; i < n_img; ++i) {
      const UdImage &u = batch.imgs[(size_t)i];
      const unsigned char *s = static_cast<const unsigned char *>(imgs[i].src);
      for (int y = 0; y < u.sh; ++y)
        std::memcpy(ud.h_in.data() + u.src_off + (long long)y * u.src_stride, s + (long long)y * imgs[i].src_stride,
                    (size_t)u.src_stride);
    }
    if (int rc = upload_vec(ctx, ud.d_src, ud.h_in)) return rc;
    ENSURE(ctx, ud.d_dst, (size_t)dst_bytes);
  }
  Events<2> ev;
  if (int rc = ev.create(ctx)) return rc;
  double t1 = now_ms();
  if (int rc = ev.record(ctx, 0)) return rc;
  launch_undist_warp(st, batch.n_units, n_img, ud.d_imgs.as<UdImage>(), ud.d_cams.as<UdCam>(),
                     batch.on_device ? nullptr : ud.d_src.as<unsigned char>(),
                     batch.on_device ? nullptr : ud.d_dst.as<unsigned char>());
  if (int rc = ev.record(ctx, 1)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  double t2 = now_ms();
  if (!batch.on_device) {
    if (int rc = download(ctx, ud.h_out, ud.d_dst.p, (size_t)dst_bytes)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
    for (int i = 0; i < n_img; ++i) {
      const UdImage &u = batch.imgs[(size_t)i];
      unsigned char *d = static_cast<unsigned char *>(imgs[i].dst);
      for (int y = 0; y < u.th; ++y)
        std::memcpy(d + (long long)y * imgs[i].dst_stride, ud.h_out.data() + u.dst_off + (long long)y * u.dst_stride,
                    (size_t)u.tw * u.ch);
    }
  }
  ud.timers[0] = t1 - t0;
  ud.timers[1] = ev.ms(0, 1);
  ud.timers[2] = now_ms() - t2;
  ud.timers[3] = (double)batch.n_units;
  return LT_OK;
}

int lt_undist_points(lt_ctx *ctx, int n_cam, const lt_undist_camera *cams, int64_t n, const double *xy,
                     const int32_t *cam_src, const int32_t *cam_dst, double *out_xy, int32_t *status, int32_t *iters) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::string who = "lt_undist_points: ";
  std::vector<UdCam> table;
  std::string msg;
  double t0 = now_ms();
  if (ud_prepare_cams(n_cam, cams, table, msg) || ud_check_points(n_cam, n, xy, cam_src, cam_dst, out_xy, status, iters, msg))
    return fail(ctx, LT_ERR_ARGUMENT, who + msg);
  if ((n + kUdBlock - 1) / kUdBlock > (int64_t)INT32_MAX) return fail(ctx, LT_ERR_ARGUMENT, who + "more points than one launch takes");
  lt_host::UdState &ud = ctx->ud;
  for (double &t : ud.timers) t = 0.0;
  if (n == 0) return LT_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t N = (size_t)n;
  if (int rc = upload_vec(ctx, ud.d_cams, table)) return rc;
  ENSURE(ctx, ud.d_xy, 16 * N);
  ENSURE(ctx, ud.d_idx, 8 * N);
  ENSURE(ctx, ud.d_out, 16 * N);
  ENSURE(ctx, ud.d_stat, 8 * N);
  int *d_src = ud.d_idx.as<int>(), *d_dst = d_src + N, *d_status = ud.d_stat.as<int>(), *d_iters = d_status + N;
  HIPCHK(ctx, hipMemcpyAsync(ud.d_xy.p, xy, 16 * N, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_src, cam_src, 4 * N, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_dst, cam_dst, 4 * N, hipMemcpyHostToDevice, st));
  Events<2> ev;
  if (int rc = ev.create(ctx)) return rc;
  double t1 = now_ms();
  if (int rc = ev.record(ctx, 0)) return rc;
  launch_undist_points(st, (long long)n, ud.d_cams.as<UdCam>(), ud.d_xy.as<double>(), d_src, d_dst, ud.d_out.as<double>(),
                       d_status, d_iters);
  if (int rc = ev.record(ctx, 1)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  double t2 = now_ms();
  HIPCHK(ctx, hipMemcpyAsync(out_xy, ud.d_out.p, 16 * N, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(status, d_status, 4 * N, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(iters, d_iters, 4 * N, hipMemcpyDeviceToHost, st));
  if (int rc = stream_sync(ctx)) return rc;
  ud.timers[0] = t1 - t0;
  ud.timers[1] = ev.ms(0, 1);
  ud.timers[2] = now_ms() - t2;
  ud.timers[3] = (double)n;
  return LT_OK;
}

int lt_undist_copy_yardstick(lt_ctx *ctx, int64_t bytes, double *ms) {
  if (!ctx || !ms || bytes < 16) return ctx ? fail(ctx, LT_ERR_ARGUMENT, "lt_undist_copy_yardstick: bad arguments") : LT_ERR_ARGUMENT;
  lt_host::UdState &ud = ctx->ud;
  const long long n16 = bytes / 16;
  if ((n16 + kUdBlock - 1) / kUdBlock > (long long)INT32_MAX)
    return fail(ctx, LT_ERR_ARGUMENT, "lt_undist_copy_yardstick: more bytes than one launch takes");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ENSURE(ctx, ud.d_src, 16 * (size_t)n16);
  ENSURE(ctx, ud.d_dst, 16 * (size_t)n16);
  HIPCHK(ctx, hipMemsetAsync(ud.d_src.p, 1, 16 * (size_t)n16, ctx->stream));
  Events<2> ev;
  if (int rc = ev.create(ctx)) return rc;
  if (int rc = ev.record(ctx, 0)) return rc;
  launch_undist_copy16(ctx->stream, n16, ud.d_src.p, ud.d_dst.p);
  if (int rc = ev.record(ctx, 1)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  *ms = ev.ms(0, 1);
  return LT_OK;
}

int lt_undist_get_timers(lt_ctx *ctx, double out[4]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 4; ++k) out[k] = ctx->ud.timers[k];
  return LT_OK;
}

}  // extern "C"
