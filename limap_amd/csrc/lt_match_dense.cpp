// lt_match_dense.cpp -- the dense-warp line matcher (limap.line2d.dense: BaseDenseLineMatcher) for a batch of image
// pairs in one call: validation, the per-line terms and the tables made on the host in FP32, one upload, the launches of
// lt_kernels_dense.hip on the context's stream, the rows in the state lt_match_get / lt_match_get_scores /
// lt_match_get_timers read; and the host restatement lt_fn_match_dense_{pair,dists}_host of the same semantics (the
// expressions of lt_dense.h in plain loops).  DESIGN §17, "Dense".

#include "lt_host.h"
#include "lt_device.h"
#include "lt_dense.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace lt;
using namespace lt_impl;

namespace {

int check_config(const lt_match_dense_config *cfg, std::string &msg) {
  if (!cfg) { msg = "null configuration"; return 1; }
  if (cfg->n_samples < kDenseMinSamples || cfg->n_samples > kDenseMaxSamples) {
    msg = "n_samples outside [2, 64]";
    return 1;
  }
  if (std::isnan(cfg->segment_percentage_th) || std::isnan(cfg->pixel_th) || std::isnan(cfg->sample_thresh)) {
    msg = "segment_percentage_th, pixel_th or sample_thresh is NaN";
    return 1;
  }
  return 0;
}

// what is wrong with one direction's maps; empty when nothing is
std::string dims_msg(const int32_t *d) {
  if (d[0] < 1 || d[1] < 1) return "warp height and width must be at least 1";
  if (d[0] > kDenseMaxWarpDim || d[1] > kDenseMaxWarpDim) return "warp height or width above 16384";
  if (d[2] != d[0] || d[3] != d[1]) return "cert and warp shapes differ";
  return std::string();
}

// torch.linspace(0, 1, S) in FP32: the step once, the lower half counted up from 0, the upper half down from 1
// (dense/matcher.py:58), then the two tables by count
void make_tables(int S, float *tab) {
  const float step = 1.0f / (float)(S - 1);
  for (int k = 0; k < kDenseTabLen; ++k) tab[k] = 0.0f;
  for (int k = 0; k < S; ++k) {
    const float up = step * (float)k, down = step * (float)(S - 1 - k);
    tab[kDenseTabR + k] = k < S / 2 ? up : 1.0f - down;
  }
  for (int c = 0; c <= S; ++c) {
    tab[kDenseTabOvl + c] = (float)c / (float)S;
    tab[kDenseTabInv + c] = c ? 1.0f / (float)c : 0.0f;
  }
}

// dense/matcher.py:97-109, FP32, no contraction: a zero-length line gets non-finite terms and never overlaps
DenseLine make_line(const float *ln) {
  const float sx = ln[0], sy = ln[1], ex = ln[2], ey = ln[3];
  float dx = ex - sx, dy = ey - sy;
  const float dxx = dx * dx, dyy = dy * dy;
  const float nd = std::sqrt(dxx + dyy);
  dx = dx / nd;
  dy = dy / nd;
  DenseLine L;
  L.dx = dx;
  L.dy = dy;
  const float s0 = sx * dx, s1 = sy * dy, e0 = ex * dx, e1 = ey * dy;
  L.sp = s0 + s1;
  L.ep = e0 + e1;
  const float cx = sy - ey, cy = ex - sx;  // cross((sx, sy, 1), (ex, ey, 1))
  const float c0 = sx * ey, c1 = sy * ex;
  const float cz = c0 - c1;
  const float cxx = cx * cx, cyy = cy * cy;
  const float nl = std::sqrt(cxx + cyy);
  L.lx = cx / nl;
  L.ly = cy / nl;
  L.lz = cz / nl;
  L.pad_ = 0.0f;
  return L;
}

struct HostDir {  // one direction on the host: the warped samples [k * n + l] and the flag word per line
  std::vector<float> x, y;
  std::vector<unsigned long long> m;
};

void warp_lines(const float *lines, long long n, const int32_t *src_shape, const int32_t *dst_shape, const float *warp,
                const float *cert, const int32_t *dims, int S, float thresh, const float *tab, HostDir &D) {
  D.x.assign((size_t)(n * S), 0.0f);
  D.y.assign((size_t)(n * S), 0.0f);
  D.m.assign((size_t)n, 0ull);
  const float ax = (float)(2.0 / (double)src_shape[1]), ay = (float)(2.0 / (double)src_shape[0]);
  const float tw = (float)dst_shape[1], th = (float)dst_shape[0];
  for (long long l = 0; l < n; ++l)
    for (int k = 0; k < S; ++k) {
      float xs, ys, x, y;
      dense_sample(lines + 4 * l, tab[kDenseTabR + k], xs, ys);
      const bool ok = dense_warp_point(warp, cert, dims[0], dims[1], ax, ay, tw, th, thresh, xs, ys, x, y);
      D.x[(size_t)(k * n + l)] = x;
      D.y[(size_t)(k * n + l)] = y;
      D.m[(size_t)l] |= (unsigned long long)ok << k;
    }
}

int host_check(const float *lines1, int64_t n1, const int32_t *shape1, const float *lines2, int64_t n2,
               const int32_t *shape2, const float *warp12, const float *cert12, const int32_t *dims12,
               const float *warp21, const float *cert21, const int32_t *dims21, const lt_match_dense_config *cfg) {
  std::string msg;
  if (check_config(cfg, msg) || n1 < 0 || n2 < 0 || n1 > kMatchMaxLines || n2 > kMatchMaxLines) return LT_ERR_ARGUMENT;
  if ((n1 && !lines1) || (n2 && !lines2) || !shape1 || !shape2 || !dims12 || !dims21) return LT_ERR_ARGUMENT;
  if (!warp12 || !cert12 || !warp21 || !cert21) return LT_ERR_ARGUMENT;
  if (shape1[0] < 1 || shape1[1] < 1 || shape2[0] < 1 || shape2[1] < 1) return LT_ERR_ARGUMENT;
  if (!dims_msg(dims12).empty() || !dims_msg(dims21).empty()) return LT_ERR_ARGUMENT;
  return LT_OK;
}

// all five matrices of one pair on the host; d21 / o21 are (n2, n1)
void host_dists(const float *lines1, long long n1, const int32_t *shape1, const float *lines2, long long n2,
                const int32_t *shape2, const float *warp12, const float *cert12, const int32_t *dims12,
                const float *warp21, const float *cert21, const int32_t *dims21, const lt_match_dense_config *cfg,
                float *d12, float *o12, float *d21, float *o21, float *dists) {
  const int S = cfg->n_samples;
  float tab[kDenseTabLen];
  make_tables(S, tab);
  HostDir F, B;
  warp_lines(lines1, n1, shape1, shape2, warp12, cert12, dims12, S, cfg->sample_thresh, tab, F);
  warp_lines(lines2, n2, shape2, shape1, warp21, cert21, dims21, S, cfg->sample_thresh, tab, B);
  std::vector<DenseLine> t1((size_t)n1), t2((size_t)n2);
  for (long long i = 0; i < n1; ++i) t1[(size_t)i] = make_line(lines1 + 4 * i);
  for (long long j = 0; j < n2; ++j) t2[(size_t)j] = make_line(lines2 + 4 * j);
  const float *ovl = tab + kDenseTabOvl, *inv = tab + kDenseTabInv;
  const float seg_th = cfg->segment_percentage_th, pix_th = cfg->pixel_th;
#pragma omp parallel for schedule(static)
  for (long long i = 0; i < n1; ++i)
    for (long long j = 0; j < n2; ++j) {
      float a, oa, b, ob;
      dense_direction(F.x.data() + i, F.y.data() + i, (int)n1, F.m[(size_t)i], t2[(size_t)j], S, ovl, inv, seg_th, a, oa);
      dense_direction(B.x.data() + j, B.y.data() + j, (int)n2, B.m[(size_t)j], t1[(size_t)i], S, ovl, inv, seg_th, b, ob);
      if (d12) d12[i * n2 + j] = a;
      if (o12) o12[i * n2 + j] = oa;
      if (d21) d21[j * n1 + i] = b;
      if (o21) o21[j * n1 + i] = ob;
      if (dists) dists[i * n2 + j] = dense_combine(a, oa, b, ob, seg_th, pix_th);
    }
}

}  // namespace

extern "C" {

#ifndef LT_HOST_ONLY  // (the sanitizer program of tools/dense_host_asan.cpp compiles the host restatement alone)
int lt_match_dense_pairs(lt_ctx *ctx, int n_img, const int64_t *line_off, const float *lines, const int32_t *shapes,
                         int64_t n_pairs, const int32_t *pair_img, const float *const *warp, const float *const *cert,
                         const int32_t *dims, const lt_match_dense_config *cfg, int64_t *n_rows) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::string who = "lt_match_dense_pairs: ";
  std::string msg;
  if (check_config(cfg, msg)) return fail(ctx, LT_ERR_ARGUMENT, who + msg);
  if (n_img < 0 || !line_off) return fail(ctx, LT_ERR_ARGUMENT, who + "bad image count or null line_off");
  if (int rc = check_offsets(ctx, "lt_match_dense_pairs", "line", n_img, line_off)) return rc;
  const long long n_lines = line_off[n_img];
  if ((n_lines > 0 && !lines) || (n_img > 0 && !shapes)) return fail(ctx, LT_ERR_ARGUMENT, who + "null lines or shapes");
  if (n_pairs < 0 || n_pairs > (1 << 24)) return fail(ctx, LT_ERR_ARGUMENT, who + "n_pairs negative or above 2^24");
  if (n_pairs > 0 && (!pair_img || !warp || !cert || !dims))
    return fail(ctx, LT_ERR_ARGUMENT, who + "null pair_img, warp, cert or dims");
  for (int m = 0; m < n_img; ++m) {
    if (line_off[m + 1] - line_off[m] > kMatchMaxLines)
      return fail(ctx, LT_ERR_ARGUMENT, who + "more than 65535 lines in an image");
    if (shapes[2 * m] < 1 || shapes[2 * m + 1] < 1)
      return fail(ctx, LT_ERR_ARGUMENT, who + "shapes: image_shape must be positive");
  }
  for (long long q = 0; q < 2 * n_pairs; ++q) {
    if (pair_img[q] < 0 || pair_img[q] >= n_img) return fail(ctx, LT_ERR_ARGUMENT, who + "pair_img: not an image");
    const std::string m = dims_msg(dims + 4 * q);
    if (!m.empty()) return fail(ctx, LT_ERR_ARGUMENT, who + "dims: " + m);
    if (!warp[q] || !cert[q]) return fail(ctx, LT_ERR_ARGUMENT, who + "a null warp or cert");
  }
  const bool on_dev = cfg->on_device != 0;
  const int S = cfg->n_samples;
  double t0 = now_ms();

  // ---- terms, tables, tasks, directions, tiles ----
  std::vector<float> tab(kDenseTabLen);
  make_tables(S, tab.data());
  std::vector<DenseLine> terms((size_t)n_lines);
#pragma omp parallel for schedule(static)
  for (long long l = 0; l < n_lines; ++l) terms[(size_t)l] = make_line(lines + 4 * l);
  std::vector<DenseTask> tasks((size_t)n_pairs);
  std::vector<DenseDir> dirs((size_t)(2 * n_pairs));
  std::vector<DenseUnit> units;
  std::vector<long long> map_off((size_t)(2 * n_pairs) + 1, 0);  // floats of the directions' maps in the staging buffer
  long long smp = 0, ent = 0, R = 0;
  int max_n = 0, max_n1 = 0;
  for (long long p = 0; p < n_pairs; ++p) {
    const int ia = pair_img[2 * p], ib = pair_img[2 * p + 1];
    DenseTask &T = tasks[(size_t)p];
    T.a0 = line_off[ia];
    T.b0 = line_off[ib];
    T.n1 = (int)(line_off[ia + 1] - line_off[ia]);
    T.n2 = (int)(line_off[ib + 1] - line_off[ib]);
    T.d0 = ent;
    T.r0 = R;
    ent += (long long)T.n1 * T.n2;
    R += T.n1;
    for (int dir = 0; dir < 2; ++dir) {
      const long long q = 2 * p + dir;
      const int src = dir ? ib : ia, dst = dir ? ia : ib;
      DenseDir &D = dirs[(size_t)q];
      D.warp = warp[q];
      D.cert = cert[q];
      D.src0 = line_off[src];
      D.smp0 = smp;
      D.n = dir ? T.n2 : T.n1;
      D.hw = dims[4 * q];
      D.ww = dims[4 * q + 1];
      D.pad_ = 0;
      D.ax = (float)(2.0 / (double)shapes[2 * src + 1]);
      D.ay = (float)(2.0 / (double)shapes[2 * src]);
      D.tw = (float)shapes[2 * dst + 1];
      D.th = (float)shapes[2 * dst];
      (dir ? T.s21 : T.s12) = smp;
      smp += (long long)D.n * S;
      max_n = std::max(max_n, D.n);
      map_off[(size_t)q + 1] = map_off[(size_t)q] + 3ll * D.hw * D.ww;
    }
    max_n1 = std::max(max_n1, T.n1);
    for (int i0 = 0; i0 < T.n1; i0 += kDenseTile)
      for (int j0 = 0; j0 < T.n2; j0 += kDenseTile) units.push_back(DenseUnit{(int)p, i0, j0});
  }
  if (units.size() > 0x7fffffffull || ent >= (1ll << 36)) return fail(ctx, LT_ERR_ARGUMENT, who + "too many entries in one call");

  // ---- upload ----
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  auto &mt = ctx->mt;
  if (!on_dev) {  // every direction's warp and certainty behind each other in one buffer
    ENSURE(ctx, mt.d_desc, sizeof(float) * (size_t)std::max<long long>(map_off.back(), 1));
    for (long long q = 0; q < 2 * n_pairs; ++q) {
      const size_t hw = (size_t)dirs[(size_t)q].hw * dirs[(size_t)q].ww;
      float *dst = mt.d_desc.as<float>() + map_off[(size_t)q];
      HIPCHK(ctx, hipMemcpyAsync(dst, warp[q], sizeof(float) * 2 * hw, hipMemcpyHostToDevice, st));
      HIPCHK(ctx, hipMemcpyAsync(dst + 2 * hw, cert[q], sizeof(float) * hw, hipMemcpyHostToDevice, st));
      dirs[(size_t)q].warp = dst;
      dirs[(size_t)q].cert = dst + 2 * hw;
    }
  }
  ENSURE(ctx, mt.d_dn_lines, sizeof(float) * 4 * (size_t)std::max<long long>(n_lines, 1));
  if (n_lines)
    HIPCHK(ctx, hipMemcpyAsync(mt.d_dn_lines.p, lines, sizeof(float) * 4 * (size_t)n_lines, hipMemcpyHostToDevice, st));
  if (int rc = upload_vec(ctx, mt.d_dn_terms, terms)) return rc;
  if (int rc = upload_vec(ctx, mt.d_dn_tab, tab)) return rc;
  if (int rc = upload_vec(ctx, mt.d_tasks, tasks)) return rc;
  if (int rc = upload_vec(ctx, mt.d_dn_dirs, dirs)) return rc;
  if (int rc = upload_vec(ctx, mt.d_units, units)) return rc;
  const size_t nsmp = (size_t)std::max<long long>(smp, 1), nent = (size_t)std::max<long long>(ent, 1);
  ENSURE(ctx, mt.d_dn_wx, 4 * nsmp);
  ENSURE(ctx, mt.d_dn_wy, 4 * nsmp);
  ENSURE(ctx, mt.d_dn_wok, nsmp);
  ENSURE(ctx, mt.d_dn_dist, 4 * nent);
  const bool want_dirs = cfg->want_dirs != 0;
  if (want_dirs) ENSURE(ctx, mt.d_dn_aux, 16 * nent);
  ENSURE(ctx, mt.d_dn_cnt, 4 * (size_t)(R + 1));
  ENSURE(ctx, mt.d_dn_off, 8 * (size_t)(R + 1));
  const size_t scan_tmp = scan_temp_bytes_u32_to_i64(R + 1);
  ENSURE(ctx, mt.d_dn_scan, std::max<size_t>(scan_tmp, 16));
  HIPCHK(ctx, hipMemsetAsync(mt.d_dn_cnt.p, 0, 4 * (size_t)(R + 1), st));
  if (int rc = stream_sync(ctx)) return rc;
  double t1 = now_ms();
  mt.timers[0] = t1 - t0;

  // ---- kernels ----
  Events<4> ev;
  if (int rc = ev.create(ctx)) return rc;
  const DenseTask *d_tasks = mt.d_tasks.as<DenseTask>();
  const float seg_th = cfg->segment_percentage_th, pix_th = cfg->pixel_th;
  const int otm = cfg->one_to_many ? 1 : 0;
  if (int rc = ev.record(ctx, 0)) return rc;
  launch_dense_warp(st, mt.d_dn_dirs.as<DenseDir>(), (int)(2 * n_pairs), max_n, S, cfg->sample_thresh,
                    mt.d_dn_lines.as<float>(), mt.d_dn_tab.as<float>(), mt.d_dn_wx.as<float>(), mt.d_dn_wy.as<float>(),
                    mt.d_dn_wok.as<unsigned char>());
  if (int rc = ev.record(ctx, 1)) return rc;
  launch_dense_pairs(st, d_tasks, mt.d_units.as<DenseUnit>(), (int)units.size(), S, seg_th, pix_th,
                     mt.d_dn_terms.as<DenseLine>(), mt.d_dn_tab.as<float>(), mt.d_dn_wx.as<float>(),
                     mt.d_dn_wy.as<float>(), mt.d_dn_wok.as<unsigned char>(), mt.d_dn_dist.as<float>(),
                     want_dirs ? mt.d_dn_aux.as<float>() : nullptr, ent);
  if (int rc = ev.record(ctx, 2)) return rc;
  launch_dense_select(st, d_tasks, (int)n_pairs, max_n1, 0, otm, pix_th, mt.d_dn_dist.as<float>(),
                      mt.d_dn_cnt.as<unsigned>(), nullptr, nullptr, nullptr, nullptr);
  if (launch_scan_u32_to_i64(st, mt.d_dn_scan.p, scan_tmp, R + 1, mt.d_dn_cnt.as<unsigned>(), mt.d_dn_off.as<long long>()) != 0)
    return fail(ctx, LT_ERR_HIP, "rocprim scan failed");
  std::vector<long long> off;
  if (int rc = download(ctx, off, mt.d_dn_off.p, (size_t)(R + 1))) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  const long long rows = off.back();
  if (rows >= (1ll << 36)) return fail(ctx, LT_ERR_ARGUMENT, who + "too many result rows");
  ENSURE(ctx, mt.d_dn_line, 4 * (size_t)std::max<long long>(rows, 1));
  ENSURE(ctx, mt.d_col, 2 * (size_t)std::max<long long>(rows, 1) + 16);
  ENSURE(ctx, mt.d_score, 4 * (size_t)std::max<long long>(rows, 1));
  if (rows)
    launch_dense_select(st, d_tasks, (int)n_pairs, max_n1, 1, otm, pix_th, mt.d_dn_dist.as<float>(),
                        mt.d_dn_cnt.as<unsigned>(), mt.d_dn_off.as<long long>(), mt.d_dn_line.as<int>(),
                        mt.d_col.as<unsigned short>(), mt.d_score.as<float>());
  if (int rc = ev.record(ctx, 3)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  double t2 = now_ms();
  mt.timers[1] = t2 - t1;
  mt.dense_ms[0] = ev.ms(0, 1);
  mt.dense_ms[1] = ev.ms(1, 2);
  mt.dense_ms[2] = ev.ms(2, 3);

  // ---- download ----
  if (int rc = download(ctx, mt.dense_line, mt.d_dn_line.p, (size_t)rows)) return rc;
  if (int rc = download(ctx, mt.col, mt.d_col.p, (size_t)rows)) return rc;
  mt.score.clear();
  if (cfg->want_scores)
    if (int rc = download(ctx, mt.score, mt.d_score.p, (size_t)rows)) return rc;
  mt.dense_aux.clear();
  mt.dense_aux_n = want_dirs ? ent : -1;
  if (want_dirs) {
    mt.dense_aux.resize((size_t)(5 * ent));
    if (ent) {
      HIPCHK(ctx, hipMemcpyAsync(mt.dense_aux.data(), mt.d_dn_aux.p, 16 * (size_t)ent, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(mt.dense_aux.data() + 4 * ent, mt.d_dn_dist.p, 4 * (size_t)ent, hipMemcpyDeviceToHost, st));
    }
  }
  if (int rc = stream_sync(ctx)) return rc;
  double t3 = now_ms();
  mt.timers[2] = t3 - t2;

  // ---- rows per pair ----
  mt.row_off.assign((size_t)n_pairs + 1, 0);
  for (long long p = 0; p < n_pairs; ++p) mt.row_off[(size_t)p] = off[(size_t)tasks[(size_t)p].r0];
  mt.row_off[(size_t)n_pairs] = rows;
  mt.slot_off.assign(mt.row_off.begin(), mt.row_off.end());
  mt.kk.assign((size_t)n_pairs, 1);
  mt.mutual = false;
  mt.dense = true;
  mt.timers[3] = now_ms() - t3;
  if (n_rows) *n_rows = (int64_t)rows;
  return LT_OK;
}

int lt_match_dense_get_kernel_ms(lt_ctx *ctx, double out[3]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 3; ++k) out[k] = ctx->mt.dense_ms[k];
  return LT_OK;
}

int lt_match_dense_get_dirs(lt_ctx *ctx, float *d12, float *o12, float *d21, float *o21, float *dists) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::vector<float> &a = ctx->mt.dense_aux;
  if (!ctx->mt.dense || ctx->mt.dense_aux_n < 0)
    return fail(ctx, LT_ERR_STATE, "lt_match_dense_get_dirs: the last call was not lt_match_dense_pairs with want_dirs");
  const size_t n = (size_t)ctx->mt.dense_aux_n;
  float *dst[5] = {d12, o12, d21, o21, dists};
  for (int k = 0; k < 5; ++k)
    if (dst[k]) std::copy(a.begin() + k * n, a.begin() + (k + 1) * n, dst[k]);
  return LT_OK;
}

#endif  // LT_HOST_ONLY

int lt_fn_match_dense_dists_host(const float *lines1, int64_t n1, const int32_t *shape1, const float *lines2, int64_t n2,
                                 const int32_t *shape2, const float *warp12, const float *cert12, const int32_t *dims12,
                                 const float *warp21, const float *cert21, const int32_t *dims21,
                                 const lt_match_dense_config *cfg, float *d12, float *o12, float *d21, float *o21,
                                 float *dists) {
  if (int rc = host_check(lines1, n1, shape1, lines2, n2, shape2, warp12, cert12, dims12, warp21, cert21, dims21, cfg))
    return rc;
  host_dists(lines1, n1, shape1, lines2, n2, shape2, warp12, cert12, dims12, warp21, cert21, dims21, cfg, d12, o12, d21,
             o21, dists);
  return LT_OK;
}

int lt_fn_match_dense_pair_host(const float *lines1, int64_t n1, const int32_t *shape1, const float *lines2, int64_t n2,
                                const int32_t *shape2, const float *warp12, const float *cert12, const int32_t *dims12,
                                const float *warp21, const float *cert21, const int32_t *dims21,
                                const lt_match_dense_config *cfg, int32_t *rows2, float *scores, int64_t *n_rows) {
  if (!n_rows) return LT_ERR_ARGUMENT;
  if (int rc = host_check(lines1, n1, shape1, lines2, n2, shape2, warp12, cert12, dims12, warp21, cert21, dims21, cfg))
    return rc;
  std::vector<float> dists((size_t)(n1 * n2));
  host_dists(lines1, n1, shape1, lines2, n2, shape2, warp12, cert12, dims12, warp21, cert21, dims21, cfg, nullptr, nullptr,
             nullptr, nullptr, dists.data());
  long long n = 0;
  for (long long i = 0; i < n1; ++i) {
    const float *row = dists.data() + i * n2;
    float m = HUGE_VALF;
    for (long long j = 0; j < n2; ++j) m = row[j] < m ? row[j] : m;
    for (long long j = 0; j < n2; ++j) {
      if (!(row[j] <= cfg->pixel_th && (cfg->one_to_many || row[j] == m))) continue;
      if (rows2) { rows2[2 * n] = (int32_t)i; rows2[2 * n + 1] = (int32_t)j; }
      if (scores) scores[n] = row[j];
      ++n;
    }
  }
  *n_rows = n;
  return LT_OK;
}

}  // extern "C"
