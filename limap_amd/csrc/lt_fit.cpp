// lt_fit.cpp -- limap.fitting on the GPU (fitting/fitting.py:8-102, fitting/line3d_estimator.cc): one 3D segment per 2D
// segment of the context from a depth map (lt_fit_segs) or a 3D point scan (lt_fit_scans) per image, and Fit3DPoints
// over a CSR of point sets (lt_fit_points).  The host validates, uploads and launches once per batch; every segment's
// work runs on the device (lt_kernels_fit.hip).  DESIGN §12, §13.

#include "lt_host.h"
#include "lt_fit.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

using namespace lt;
using namespace lt_impl;

namespace {

int check_cfg(lt_ctx *ctx, const lt_fit_config &c) {
  auto bad = [&](const char *what) { return fail(ctx, LT_ERR_ARGUMENT, std::string("lt_fit: ") + what); };
  if (!std::isfinite(c.ransac_th) || !std::isfinite(c.var2d) || !std::isfinite(c.min_percentage_inliers))
    return bad("ransac_th, var2d and min_percentage_inliers must be finite");
  if (!std::isfinite(c.squared_inlier_threshold) || c.squared_inlier_threshold < 0.0)
    return bad("squared_inlier_threshold must be finite and >= 0");
  if (!(c.success_probability >= 0.0 && c.success_probability <= 1.0)) return bad("success_probability outside [0, 1]");
  if (!std::isfinite(c.threshold_multiplier)) return bad("threshold_multiplier must be finite");
  if (c.min_num_iterations < 0 || c.max_num_iterations < 0 || c.min_num_iterations > 10000000 ||
      c.max_num_iterations > 10000000)
    return bad("iteration counts outside [0, 1e7]");
  if (c.num_lo_steps < 0 || c.num_lo_steps > 100000 || c.num_lsq_iterations < 0 || c.num_lsq_iterations > 100000)
    return bad("num_lo_steps / num_lsq_iterations outside [0, 1e5]");
  if (c.min_sample_multiplicator < 0 || c.min_sample_multiplicator > 1000000 || c.non_min_sample_multiplier < 0 ||
      c.non_min_sample_multiplier > 1000000 || c.lo_starting_iterations < 0)
    return bad("sample multipliers outside [0, 1e6] or lo_starting_iterations < 0");
  if (c.final_least_squares != 0 && c.final_least_squares != 1) return bad("final_least_squares must be 0 or 1");
  return LT_OK;
}

FitCfg dev_cfg(const lt_fit_config &c) {
  FitCfg f;
  f.t2_points = c.squared_inlier_threshold;
  f.ransac_th = c.ransac_th; f.min_pct = c.min_percentage_inliers; f.var2d = c.var2d;
  f.pmiss = 1.0 - c.success_probability;
  f.mult = c.threshold_multiplier;
  f.min_it = c.min_num_iterations; f.max_it = c.max_num_iterations;
  f.num_lo = c.num_lo_steps; f.num_lsq = c.num_lsq_iterations;
  f.min_smp_mult = c.min_sample_multiplicator; f.nonmin_mult = c.non_min_sample_multiplier;
  f.lo_start = c.lo_starting_iterations; f.final_ls = c.final_least_squares;
  f.seed = c.seed;
  return f;
}

// [seg3d 6 doubles | status int | stats 5 ints] per problem, 8-byte aligned blocks
struct OutLayout {
  size_t seg, status, stats, mask, bytes;
  OutLayout(long long n, long long n_mask) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    seg = 0;
    status = up(seg + 48 * (size_t)n);
    stats = up(status + 4 * (size_t)n);
    mask = up(stats + 20 * (size_t)n);
    bytes = up(mask + (size_t)n_mask) + 256;
  }
};

// the launch over a counted scratch of points (32 B each, behind a 256-B header), run again with the counted size when a
// long problem found no room; results do not depend on it
template <class Launch>
int run_with_scratch(lt_ctx *ctx, Launch launch, int *attempts) {
  // first try: what the buffer already holds, at least 2^18; LT_TEST_FIT_SCRATCH_CAP forces a small one
  unsigned long long cap = ctx->ft.d_scr.cap > 256 ? (ctx->ft.d_scr.cap - 256) / 32 : 0, used = 0;
  if (cap < (1ull << 18)) cap = 1ull << 18;
  if (const char *e = test_switch("LT_TEST_FIT_SCRATCH_CAP")) cap = std::max(1ull, std::strtoull(e, nullptr, 10));
  return run_counted(ctx, ctx->ft.d_scr, 256, 32, cap, [&](void *scr, unsigned long long room, unsigned long long *cnt) {
    return launch(static_cast<double *>(scr), room, cnt);
  }, &used, attempts);
}

// segs.astype(int) / linspace stay exact for coordinates below 2^29 (the reference would enumerate every pixel)
int check_segs(lt_ctx *ctx, const char *who, const double *segs, long long G) {
  for (long long g = 0; g < 4 * G; ++g)
    if (!(std::fabs(segs[g]) < 536870912.0))
      return fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": 2D segment coordinate not finite or beyond 2^29");
  return LT_OK;
}

// the host maps of a batch into one device buffer, 256-B aligned: bytes_of(k) (0: nothing to upload), set_dev(k, p)
template <class Bytes, class Ptr, class SetDev>
int upload_maps(lt_ctx *ctx, hipStream_t st, int n_maps, Bytes bytes_of, Ptr ptr_of, SetDev set_dev) {
  size_t total = 0;
  for (int k = 0; k < n_maps; ++k) total += (bytes_of(k) + 255) & ~(size_t)255;
  if (!total) return LT_OK;
  ENSURE(ctx, ctx->ft.d_maps, total);
  size_t at = 0;
  for (int k = 0; k < n_maps; ++k) {
    const size_t b = bytes_of(k);
    if (!b) continue;
    char *dst = ctx->ft.d_maps.as<char>() + at;
    HIPCHK(ctx, hipMemcpyAsync(dst, ptr_of(k), b, hipMemcpyHostToDevice, st));
    set_dev(k, dst);
    at += (b + 255) & ~(size_t)255;
  }
  return LT_OK;
}

// the outputs of G segments to the host, then the timers (ev: start, maps uploaded, kernel start, kernel end)
int finish_segs(lt_ctx *ctx, hipStream_t st, const char *out, const OutLayout &L, long long G, double *seg3d,
                int32_t *status, int32_t *stats, const Events<4> &ev, double t_start, int attempts) {
  if (G) {
    HIPCHK(ctx, hipMemcpyAsync(seg3d, out + L.seg, 48 * (size_t)G, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(status, out + L.status, 4 * (size_t)G, hipMemcpyDeviceToHost, st));
    if (stats) HIPCHK(ctx, hipMemcpyAsync(stats, out + L.stats, 20 * (size_t)G, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(ctx, hipStreamSynchronize(st));
  ctx->ft.timers[0] = ev.ms(2, 3);
  ctx->ft.timers[1] = ev.ms(0, 1);
  ctx->ft.timers[2] = now_ms() - t_start;
  ctx->ft.timers[3] = attempts;
  return LT_OK;
}

}  // namespace

extern "C" {

void lt_fit_config_default(lt_fit_config *c) {
  c->ransac_th = 0.75;
  c->min_percentage_inliers = 0.6;
  c->var2d = 5.0;
  c->squared_inlier_threshold = 1.0;
  c->success_probability = 0.9999;
  c->threshold_multiplier = std::sqrt(2.0);
  c->min_num_iterations = 100;
  c->max_num_iterations = 10000;
  c->num_lo_steps = 10;
  c->num_lsq_iterations = 4;
  c->min_sample_multiplicator = 7;
  c->non_min_sample_multiplier = 3;
  c->lo_starting_iterations = 50;
  c->final_least_squares = 0;
  c->seed = 0;
}

int lt_fit_segs(lt_ctx *ctx, int img_begin, int n_maps, const lt_depth_map *maps, const lt_fit_config *cfg,
                double *seg3d, int32_t *status, int32_t *stats) {
  if (!ctx->inited) return fail(ctx, LT_ERR_STATE, "lt_fit_segs before lt_init");
  if (!cfg || !seg3d || !status || (n_maps > 0 && !maps)) return fail(ctx, LT_ERR_ARGUMENT, "lt_fit_segs: null argument");
  if (img_begin < 0 || n_maps < 0 || img_begin + (long long)n_maps > ctx->n_img)
    return fail(ctx, LT_ERR_ARGUMENT, "lt_fit_segs: images outside the context");
  if (int rc = check_cfg(ctx, *cfg)) return rc;
  const double t_start = now_ms();
  const long long g0 = ctx->seg_off[(size_t)img_begin], g1 = ctx->seg_off[(size_t)(img_begin + n_maps)];
  const long long G = g1 - g0;
  std::vector<FitImg> imgs((size_t)n_maps);
  for (int k = 0; k < n_maps; ++k) {
    const lt_depth_map &m = maps[k];
    const std::string who = "lt_fit_segs: map of image " + std::to_string(ctx->img_ids[(size_t)(img_begin + k)]) + ": ";
    if (m.h < 0 || m.w < 0 || m.h >= (1ll << 31) || m.w >= (1ll << 31)) return fail(ctx, LT_ERR_ARGUMENT, who + "bad size");
    if (m.dtype != LT_DEPTH_F32 && m.dtype != LT_DEPTH_F64) return fail(ctx, LT_ERR_ARGUMENT, who + "dtype");
    if (m.on_device != 0 && m.on_device != 1) return fail(ctx, LT_ERR_ARGUMENT, who + "on_device must be 0 or 1");
    if (m.h > 0 && m.w > 0) {
      if (!m.ptr) return fail(ctx, LT_ERR_ARGUMENT, who + "null pointer");
      if (m.row_stride < m.w) return fail(ctx, LT_ERR_ARGUMENT, who + "row stride below the width");
    }
    FitImg &f = imgs[(size_t)k];
    f.map = m.ptr; f.h = m.h; f.w = m.w; f.stride = m.row_stride; f.dtype = m.dtype;
    f.img_id = ctx->img_ids[(size_t)(img_begin + k)];
    f.cam = img_begin + k;
    f.seg_begin = ctx->seg_off[(size_t)(img_begin + k)] - g0;
    f.seg_end = ctx->seg_off[(size_t)(img_begin + k) + 1] - g0;
    f.pad_ = 0;
  }
  const double *segs = ctx->h_segs_ptr + 4 * g0;
  if (int rc = check_segs(ctx, "lt_fit_segs", segs, G)) return rc;
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Events<4> ev;  // start, maps uploaded, kernel start, kernel end
  if (int rc = ev.create(ctx)) return rc;
  if (int rc = ev.record(ctx, 0)) return rc;
  if (int rc = upload_maps(ctx, st, n_maps, [&](int k) -> size_t {
        const lt_depth_map &m = maps[k];
        if (m.on_device || m.h == 0 || m.w == 0) return 0;
        return ((size_t)(m.h - 1) * (size_t)m.row_stride + (size_t)m.w) * (m.dtype ? 8 : 4);
      }, [&](int k) { return maps[k].ptr; }, [&](int k, char *p) { imgs[(size_t)k].map = p; }))
    return rc;
  if (int rc = ev.record(ctx, 1)) return rc;
  const OutLayout L(G, 0);
  ENSURE(ctx, ctx->ft.d_imgs, sizeof(FitImg) * (size_t)std::max(n_maps, 1));
  ENSURE(ctx, ctx->ft.d_in, 32 * (size_t)std::max<long long>(G, 1));
  ENSURE(ctx, ctx->ft.d_out, L.bytes);
  if (n_maps) HIPCHK(ctx, hipMemcpyAsync(ctx->ft.d_imgs.p, imgs.data(), sizeof(FitImg) * (size_t)n_maps, hipMemcpyHostToDevice, st));
  if (G) HIPCHK(ctx, hipMemcpyAsync(ctx->ft.d_in.p, segs, 32 * (size_t)G, hipMemcpyHostToDevice, st));
  const FitCfg fc = dev_cfg(*cfg);
  char *out = ctx->ft.d_out.as<char>();
  int attempts = 0;
  if (int rc = run_with_scratch(ctx, [&](double *scr, unsigned long long cap, unsigned long long *cnt) {
        if (int rc = ev.record(ctx, 2)) return rc;
        launch_fit_depth(st, G, n_maps, ctx->ft.d_imgs.as<FitImg>(), ctx->ft.d_in.as<double>(), ctx->d_cams.as<Cam>(),
                         fc, scr, cap, cnt, reinterpret_cast<double *>(out + L.seg),
                         reinterpret_cast<int *>(out + L.status), reinterpret_cast<int *>(out + L.stats));
        return ev.record(ctx, 3);
      }, &attempts))
    return rc;
  return finish_segs(ctx, st, out, L, G, seg3d, status, stats, ev, t_start, attempts);
}

int lt_fit_scans(lt_ctx *ctx, int img_begin, int n_maps, const lt_scan_map *maps, const double *scan_poses,
                 const lt_fit_config *cfg, double *seg3d, int32_t *status, int32_t *stats) {
  if (!ctx->inited) return fail(ctx, LT_ERR_STATE, "lt_fit_scans before lt_init");
  if (!cfg || !seg3d || !status || (n_maps > 0 && !maps)) return fail(ctx, LT_ERR_ARGUMENT, "lt_fit_scans: null argument");
  if (img_begin < 0 || n_maps < 0 || img_begin + (long long)n_maps > ctx->n_img)
    return fail(ctx, LT_ERR_ARGUMENT, "lt_fit_scans: images outside the context");
  if (int rc = check_cfg(ctx, *cfg)) return rc;
  const double t_start = now_ms();
  const long long g0 = ctx->seg_off[(size_t)img_begin], g1 = ctx->seg_off[(size_t)(img_begin + n_maps)];
  const long long G = g1 - g0;
  std::vector<ScanImg> imgs((size_t)n_maps);
  std::vector<size_t> host_bytes((size_t)n_maps, 0);
  for (int k = 0; k < n_maps; ++k) {
    const lt_scan_map &m = maps[k];
    const std::string who = "lt_fit_scans: scan of image " + std::to_string(ctx->img_ids[(size_t)(img_begin + k)]) + ": ";
    if (m.h < 2 || m.w < 2 || m.h >= (1ll << 31) || m.w >= (1ll << 31)) return fail(ctx, LT_ERR_ARGUMENT, who + "bad size");
    // the camera's size bounds the samples a segment visits (about 2 sqrt(h^2 + w^2)): int32 counts stay exact
    if (m.img_h < 2 || m.img_w < 2 || m.img_h > (1ll << 24) || m.img_w > (1ll << 24))
      return fail(ctx, LT_ERR_ARGUMENT, who + "image size outside [2, 2^24]");
    if (m.dtype != LT_DEPTH_F32 && m.dtype != LT_DEPTH_F64) return fail(ctx, LT_ERR_ARGUMENT, who + "dtype");
    if (m.on_device != 0 && m.on_device != 1) return fail(ctx, LT_ERR_ARGUMENT, who + "on_device must be 0 or 1");
    if (!m.ptr) return fail(ctx, LT_ERR_ARGUMENT, who + "null pointer");
    if (m.row_stride < 0 || m.pix_stride < 0 || m.chan_stride < 0 || m.row_stride >= (1ll << 40) ||
        m.pix_stride >= (1ll << 40) || m.chan_stride >= (1ll << 40))
      return fail(ctx, LT_ERR_ARGUMENT, who + "strides outside [0, 2^40)");
    const double *P = scan_poses ? scan_poses + 12 * (size_t)k : nullptr;
    if (P)
      for (int e = 0; e < 12; ++e)
        if (!std::isfinite(P[e])) return fail(ctx, LT_ERR_ARGUMENT, who + "scan pose not finite");
    ScanImg &f = imgs[(size_t)k];
    f.map = m.ptr; f.h = m.h; f.w = m.w;
    f.rs = m.row_stride; f.ps = m.pix_stride; f.cs = m.chan_stride;
    f.img_h = m.img_h; f.img_w = m.img_w;
    f.seg_begin = ctx->seg_off[(size_t)(img_begin + k)] - g0;
    f.seg_end = ctx->seg_off[(size_t)(img_begin + k) + 1] - g0;
    for (int e = 0; e < 12; ++e) f.pose[e] = P ? P[e] : 0.0;
    f.dtype = m.dtype;
    f.img_id = ctx->img_ids[(size_t)(img_begin + k)];
    f.cam = img_begin + k;
    f.use_pose = P ? 1 : 0;
    if (!m.on_device)  // one past the last element read
      host_bytes[(size_t)k] = (size_t)((m.h - 1) * m.row_stride + (m.w - 1) * m.pix_stride + 2 * m.chan_stride + 1) *
                              (m.dtype ? 8 : 4);
  }
  const double *segs = ctx->h_segs_ptr + 4 * g0;
  if (int rc = check_segs(ctx, "lt_fit_scans", segs, G)) return rc;
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Events<4> ev;
  if (int rc = ev.create(ctx)) return rc;
  if (int rc = ev.record(ctx, 0)) return rc;
  if (int rc = upload_maps(ctx, st, n_maps, [&](int k) { return host_bytes[(size_t)k]; },
                           [&](int k) { return maps[k].ptr; }, [&](int k, char *p) { imgs[(size_t)k].map = p; }))
    return rc;
  if (int rc = ev.record(ctx, 1)) return rc;
  const OutLayout L(G, 0);
  ENSURE(ctx, ctx->ft.d_imgs, sizeof(ScanImg) * (size_t)std::max(n_maps, 1));
  ENSURE(ctx, ctx->ft.d_in, 32 * (size_t)std::max<long long>(G, 1));
  ENSURE(ctx, ctx->ft.d_out, L.bytes);
  if (n_maps) HIPCHK(ctx, hipMemcpyAsync(ctx->ft.d_imgs.p, imgs.data(), sizeof(ScanImg) * (size_t)n_maps, hipMemcpyHostToDevice, st));
  if (G) HIPCHK(ctx, hipMemcpyAsync(ctx->ft.d_in.p, segs, 32 * (size_t)G, hipMemcpyHostToDevice, st));
  const FitCfg fc = dev_cfg(*cfg);
  char *out = ctx->ft.d_out.as<char>();
  int attempts = 0;
  if (int rc = run_with_scratch(ctx, [&](double *scr, unsigned long long cap, unsigned long long *cnt) {
        if (int rc = ev.record(ctx, 2)) return rc;
        launch_fit_scan(st, G, n_maps, ctx->ft.d_imgs.as<ScanImg>(), ctx->ft.d_in.as<double>(), ctx->d_cams.as<Cam>(),
                        fc, scr, cap, cnt, reinterpret_cast<double *>(out + L.seg),
                        reinterpret_cast<int *>(out + L.status), reinterpret_cast<int *>(out + L.stats));
        return ev.record(ctx, 3);
      }, &attempts))
    return rc;
  return finish_segs(ctx, st, out, L, G, seg3d, status, stats, ev, t_start, attempts);
}

int lt_fit_points(lt_ctx *ctx, int64_t n_sets, const int64_t *off, const double *xyz, const lt_fit_config *cfg,
                  double *seg3d, int32_t *status, int32_t *stats, uint8_t *inlier_mask) {
  if (!off || !cfg || !seg3d || !status || n_sets < 0) return fail(ctx, LT_ERR_ARGUMENT, "lt_fit_points: null argument");
  if (off[0] != 0) return fail(ctx, LT_ERR_ARGUMENT, "lt_fit_points: off[0] must be 0");
  for (int64_t s = 0; s < n_sets; ++s)
    if (off[s + 1] < off[s] || off[s + 1] - off[s] >= (1ll << 30))
      return fail(ctx, LT_ERR_ARGUMENT, "lt_fit_points: offsets must be non-decreasing, sets below 2^30 points");
  const int64_t N = off[n_sets];
  if (N > 0 && !xyz) return fail(ctx, LT_ERR_ARGUMENT, "lt_fit_points: null points");
  if (int rc = check_cfg(ctx, *cfg)) return rc;
  const double t_start = now_ms();
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const OutLayout L(n_sets, inlier_mask ? N : 0);
  const size_t off_bytes = ((size_t)(n_sets + 1) * 8 + 255) & ~(size_t)255;
  ENSURE(ctx, ctx->ft.d_in, off_bytes + 24 * (size_t)std::max<int64_t>(N, 1));
  ENSURE(ctx, ctx->ft.d_out, L.bytes);
  char *in = ctx->ft.d_in.as<char>(), *out = ctx->ft.d_out.as<char>();
  Events<2> ev;
  if (int rc = ev.create(ctx)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(in, off, (size_t)(n_sets + 1) * 8, hipMemcpyHostToDevice, st));
  if (N) HIPCHK(ctx, hipMemcpyAsync(in + off_bytes, xyz, 24 * (size_t)N, hipMemcpyHostToDevice, st));
  if (inlier_mask && N) HIPCHK(ctx, hipMemsetAsync(out + L.mask, 0, (size_t)N, st));
  const FitCfg fc = dev_cfg(*cfg);
  int attempts = 0;
  if (int rc = run_with_scratch(ctx, [&](double *scr, unsigned long long cap, unsigned long long *cnt) {
        if (int rc = ev.record(ctx, 0)) return rc;
        launch_fit_points(st, n_sets, reinterpret_cast<const long long *>(in),
                          reinterpret_cast<const double *>(in + off_bytes), fc, scr, cap, cnt,
                          reinterpret_cast<double *>(out + L.seg), reinterpret_cast<int *>(out + L.status),
                          reinterpret_cast<int *>(out + L.stats),
                          inlier_mask ? reinterpret_cast<unsigned char *>(out + L.mask) : nullptr);
        return ev.record(ctx, 1);
      }, &attempts))
    return rc;
  if (n_sets) {
    HIPCHK(ctx, hipMemcpyAsync(seg3d, out + L.seg, 48 * (size_t)n_sets, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(status, out + L.status, 4 * (size_t)n_sets, hipMemcpyDeviceToHost, st));
    if (stats) HIPCHK(ctx, hipMemcpyAsync(stats, out + L.stats, 20 * (size_t)n_sets, hipMemcpyDeviceToHost, st));
  }
  if (inlier_mask && N) HIPCHK(ctx, hipMemcpyAsync(inlier_mask, out + L.mask, (size_t)N, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  ctx->ft.timers[0] = ev.ms(0, 1);
  ctx->ft.timers[1] = 0.0;
  ctx->ft.timers[2] = now_ms() - t_start;
  ctx->ft.timers[3] = attempts;
  return LT_OK;
}

int lt_fit_get_timers(lt_ctx *ctx, double out[4]) {
  for (int k = 0; k < 4; ++k) out[k] = ctx->ft.timers[k];
  return LT_OK;
}

}  // extern "C"
