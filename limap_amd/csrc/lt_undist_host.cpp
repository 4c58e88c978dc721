// lt_undist_host.cpp -- the host-only half of limap_amd.undistortion: validation and the tables both paths
// start from (ud_prepare_cams, ud_prepare_images), the host path of the warp and of the points
// (lt_fn_undist_warp_host, lt_fn_undist_points_host: the inline expressions of lt_undist.h under OpenMP) and the scale
// rule of UndistortCamera (lt_fn_undist_scale).  Nothing here touches the device or the context, so this unit links
// on its own.

#include "lt_hostutil.h"
#include "lt_undist_host.h"
#include "lt_twin.h"

#include <climits>
#include <cmath>

#include <omp.h>

using namespace lt;
using namespace lt_impl;

namespace lt_impl {

int ud_prepare_cams(int n_cam, const lt_undist_camera *cams, std::vector<UdCam> &out, std::string &msg) {
  if (n_cam < 0 || (n_cam > 0 && !cams)) { msg = "null or negative camera table"; return 1; }
  out.assign((size_t)n_cam, UdCam{});
  for (int i = 0; i < n_cam; ++i) {
    const lt_undist_camera &c = cams[i];
    int want = -1, one_focal = 0;
    switch (c.model) {
      case kUdSimplePinhole: want = 3; one_focal = 1; break;
      case kUdPinhole: want = 4; break;
      case kUdSimpleRadial: want = 4; one_focal = 1; break;
      case kUdRadial: want = 5; one_focal = 1; break;
      case kUdOpenCV: want = 8; break;
      case kUdFullOpenCV: want = 12; break;
      default: break;
    }
    const std::string who = "camera " + std::to_string(i) + ": ";
    if (want < 0) { msg = who + "camera model " + std::to_string(c.model) + " is not built"; return 1; }
    if (c.n_params != want) {
      msg = who + "model " + std::to_string(c.model) + " takes " + std::to_string(want) + " parameters, got " +
            std::to_string(c.n_params);
      return 1;
    }
    if (!all_finite(c.params, want)) { msg = who + "non-finite camera parameter"; return 1; }
    UdCam &u = out[(size_t)i];
    u.model = c.model;
    const double *p = c.params;
    u.fx = p[0];
    u.fy = one_focal ? p[0] : p[1];
    p += one_focal ? 1 : 2;
    u.cx = p[0];
    u.cy = p[1];
    p += 2;
    for (int k = 0; k < 8; ++k) u.k[k] = k < want - (one_focal ? 3 : 4) ? p[k] : 0.0;
    if (u.fx == 0.0 || u.fy == 0.0) { msg = who + "a focal length is 0"; return 1; }
  }
  return 0;
}

int ud_prepare_images(const std::vector<UdCam> &cams, int n_img, const lt_undist_image *imgs, UdBatch &out,
                      std::string &msg) {
  if (n_img < 0 || (n_img > 0 && !imgs)) { msg = "null or negative image table"; return 1; }
  out.imgs.assign((size_t)n_img, UdImage{});
  out.n_units = 0;
  out.on_device = n_img > 0 ? (imgs[0].on_device ? 1 : 0) : 0;
  const int n_cam = (int)cams.size();
  for (int i = 0; i < n_img; ++i) {
    const lt_undist_image &m = imgs[i];
    const std::string who = "image " + std::to_string(i) + ": ";
    if (m.src_w < 1 || m.src_h < 1 || m.dst_w < 1 || m.dst_h < 1) { msg = who + "image size below 1"; return 1; }
    if (m.src_w > kUdMaxDim || m.src_h > kUdMaxDim || m.dst_w > kUdMaxDim || m.dst_h > kUdMaxDim) {
      msg = who + "image size above " + std::to_string(kUdMaxDim);
      return 1;
    }
    if (m.channels != 1 && m.channels != 3 && m.channels != 4) { msg = who + "channel count outside {1, 3, 4}"; return 1; }
    if (!m.src || !m.dst) { msg = who + "null image"; return 1; }
    if (m.src_stride < (int64_t)m.src_w * m.channels || m.dst_stride < (int64_t)m.dst_w * m.channels) {
      msg = who + "a row stride is shorter than a row";
      return 1;
    }
    if (m.src_cam < 0 || m.src_cam >= n_cam || m.dst_cam < 0 || m.dst_cam >= n_cam) {
      msg = who + "camera index outside the table";
      return 1;
    }
    if (!ud_is_pinhole(cams[(size_t)m.dst_cam].model)) { msg = who + "the target camera must be a pinhole model"; return 1; }
    if ((m.on_device ? 1 : 0) != out.on_device) { msg = "a warp batch mixes host and device images"; return 1; }
    UdImage &u = out.imgs[(size_t)i];
    u.src_stride = m.src_stride;
    u.dst_stride = m.dst_stride;
    u.sw = m.src_w; u.sh = m.src_h; u.tw = m.dst_w; u.th = m.dst_h;
    u.ch = m.channels;
    u.cam_src = m.src_cam;
    u.cam_dst = m.dst_cam;
    u.unit0 = out.n_units;
    out.n_units += (long long)m.dst_h * ((m.dst_w + kUdRun - 1) / kUdRun);
    if (out.n_units > (long long)INT_MAX * kUdBlock) { msg = "the batch has more work units than one launch takes"; return 1; }
  }
  return 0;
}

int ud_check_points(int n_cam, int64_t n, const double *xy, const int32_t *cam_src, const int32_t *cam_dst,
                    const double *out_xy, const int32_t *status, const int32_t *iters, std::string &msg) {
  if (n < 0) { msg = "negative point count"; return 1; }
  if (n > 0 && (!xy || !cam_src || !cam_dst || !out_xy || !status || !iters)) { msg = "null point arrays"; return 1; }
  for (int64_t i = 0; i < n; ++i)
    if (cam_src[i] < 0 || cam_src[i] >= n_cam || cam_dst[i] < 0 || cam_dst[i] >= n_cam) {
      msg = "point " + std::to_string((long long)i) + ": camera index outside the table";
      return 1;
    }
  return 0;
}

}  // namespace lt_impl

namespace {

thread_local HostError t_err;

template <int C>
void host_row(const UdCam &cs, const UdCam &ct, const lt_undist_image &m, int y) {
  const unsigned char *src = static_cast<const unsigned char *>(m.src);
  unsigned char *out = static_cast<unsigned char *>(m.dst) + (long long)y * m.dst_stride;
  const double v = ud_row_v(ct, y);
  for (int x = 0; x < m.dst_w; ++x) {
    const unsigned px = ud_warp_pixel<C>(cs, ct, src, m.src_stride, m.src_w, m.src_h, x, v);
    for (int c = 0; c < C; ++c) out[(long long)x * C + c] = (unsigned char)((px >> (8 * c)) & 0xffu);
  }
}

}  // namespace

extern "C" {

const char *lt_fn_undist_host_error(void) { return t_err.c_str(); }

int lt_fn_undist_warp_host(int n_cam, const lt_undist_camera *cams, int n_img, const lt_undist_image *imgs,
                           int n_threads) {
  t_err.clear();
  std::vector<UdCam> table;
  UdBatch batch;
  if (ud_prepare_cams(n_cam, cams, table, t_err.text) || ud_prepare_images(table, n_img, imgs, batch, t_err.text))
    return LT_ERR_ARGUMENT;
  if (batch.on_device) { t_err.text = "lt_fn_undist_warp_host: device images"; return LT_ERR_ARGUMENT; }
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
  for (int i = 0; i < n_img; ++i) {
    const lt_undist_image &m = imgs[i];
    const UdCam cs = table[(size_t)m.src_cam], ct = table[(size_t)m.dst_cam];
#pragma omp parallel for num_threads(nt) schedule(static)
    for (int y = 0; y < m.dst_h; ++y) {
      if (m.channels == 1) host_row<1>(cs, ct, m, y);
      else if (m.channels == 3) host_row<3>(cs, ct, m, y);
      else host_row<4>(cs, ct, m, y);
    }
  }
  return LT_OK;
}

int lt_fn_undist_points_host(int n_cam, const lt_undist_camera *cams, int64_t n, const double *xy,
                             const int32_t *cam_src, const int32_t *cam_dst, double *out_xy, int32_t *status,
                             int32_t *iters, int n_threads) {
  t_err.clear();
  std::vector<UdCam> table;
  if (ud_prepare_cams(n_cam, cams, table, t_err.text) || ud_check_points(n_cam, n, xy, cam_src, cam_dst, out_xy, status, iters, t_err.text))
    return LT_ERR_ARGUMENT;
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int64_t i = 0; i < n; ++i) {
    int it = 0;
    status[i] = ud_point(table[(size_t)cam_src[i]], table[(size_t)cam_dst[i]], xy[2 * i], xy[2 * i + 1], out_xy[2 * i],
                         out_xy[2 * i + 1], it);
    iters[i] = it;
  }
  return LT_OK;
}

int lt_fn_undist_scale(int32_t w, int32_t h, double cx, double cy, const double ext[8], double blank_pixels,
                       double min_scale, double max_scale, double out[4]) {
  t_err.clear();
  if (!ext || !out || w < 1 || h < 1) { t_err.text = "lt_fn_undist_scale: bad arguments"; return LT_ERR_ARGUMENT; }
  if (!(blank_pixels >= 0.0 && blank_pixels <= 1.0)) { t_err.text = "Check failed: blank_pixels in [0, 1]"; return LT_ERR_ARGUMENT; }
  if (!(min_scale > 0.0)) { t_err.text = "Check failed: min_scale > 0"; return LT_ERR_ARGUMENT; }
  if (!(min_scale <= max_scale) || !std::isfinite(max_scale)) { t_err.text = "Check failed: min_scale <= max_scale"; return LT_ERR_ARGUMENT; }
  if (!all_finite(ext, 8) || !std::isfinite(cx) || !std::isfinite(cy)) {
    t_err.text = "lt_fn_undist_scale: non-finite border";
    return LT_ERR_ARGUMENT;
  }
  const double dims[2] = {(double)w, (double)h}, c[2] = {cx, cy};
  for (int a = 0; a < 2; ++a) {
    const double *e = ext + 4 * a;  // low side min, low side max, high side min, high side max
    const double lo_a = c[a] / (c[a] - e[0]), lo_b = (dims[a] - 0.5 - c[a]) / (e[3] - c[a]);
    const double hi_a = c[a] / (c[a] - e[1]), hi_b = (dims[a] - 0.5 - c[a]) / (e[2] - c[a]);
    const double smin = lo_b < lo_a ? lo_b : lo_a;  // std::min(lo_a, lo_b)
    const double smax = hi_a < hi_b ? hi_b : hi_a;  // std::max(hi_a, hi_b)
    double s = 1.0 / (smin * blank_pixels + smax * (1.0 - blank_pixels));
    if (s != s) { t_err.text = "lt_fn_undist_scale: the border gives no scale"; return LT_ERR_ARGUMENT; }
    s = s < min_scale ? min_scale : (max_scale < s ? max_scale : s);  // std::clamp
    double n = s * dims[a];
    if (!(n >= 1.0)) n = 1.0;
    if (n > (double)kUdMaxDim) { t_err.text = "lt_fn_undist_scale: the undistorted image is too large"; return LT_ERR_ARGUMENT; }
    const double size = (double)(long long)n;  // size_t(max(1.0, scale * size))
    out[a] = size;
    out[2 + a] = c[a] * (size / dims[a]);
  }
  return LT_OK;
}

}  // extern "C"
