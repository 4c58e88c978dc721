// lt_patch.cpp -- limap.features' line patch extraction (line_patch_extractor.cc, featurepatch.h): DESIGN §24 is the
// definition.  lt_patch_extract gathers all patches of one feature map in one launch of k_patch_gather per output chunk
// (lt_kernels_patch.hip); lt_fn_patch_extract_host is the host path from the same inline expressions of lt_patch.h
// under OpenMP, lt_fn_patch_geometry the patches' geometry alone and lt_fn_patch_ranges GetLine2DRange over CSR arrays
// of tracks and supports.  Every argument is checked before any work.  The sanitizer program of
// tools/patch_host_asan.cpp compiles this file with LT_HOST_ONLY: the host-only entry points, no context, no
// HIP runtime.

#ifndef LT_HOST_ONLY
#include "lt_host.h"
#else
#include "../../include/limap_amd.h"
#endif
#include "lt_patch.h"
#include "lt_twin.h"

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include <omp.h>

using namespace lt;

namespace {

thread_local lt_impl::HostError t_err;

struct PtPlan {
  std::vector<PtGeom> geom;
  std::vector<long long> off;  // n + 1: first element of every patch in the packed output
  int patch_w = 1;
};

int elem_size(int dtype) { return dtype == kPtF16 ? 2 : (dtype == kPtF32 ? 4 : 8); }
bool known_dtype(int dtype) { return dtype == kPtF16 || dtype == kPtF32 || dtype == kPtF64; }

// 0, or 1 with msg set
int check_cfg(const lt_patch_config *cfg, std::string &msg) {
  if (!cfg) { msg = "null configuration"; return 1; }
  if (!std::isfinite(cfg->k_stretch)) { msg = "non-finite k_stretch"; return 1; }
  if (cfg->t_stretch < 0) { msg = "t_stretch below 0"; return 1; }
  if (cfg->range_perp < 0) { msg = "range_perp below 0"; return 1; }
  if (cfg->range_perp > kPtMaxPerp) { msg = "range_perp above " + std::to_string(kPtMaxPerp); return 1; }
  return 0;
}

int check_map(const lt_feature_map *m, std::string &msg) {
  if (!m) { msg = "null feature map"; return 1; }
  if (m->h < 1 || m->w < 1 || m->c < 1) { msg = "feature map with H, W or C below 1"; return 1; }
  if (m->h > INT_MAX / 2 || m->w > INT_MAX / 2 || m->c > (1 << 20)) { msg = "feature map too large"; return 1; }
  if (!known_dtype(m->dtype)) { msg = "unknown feature map dtype " + std::to_string(m->dtype); return 1; }
  if (!m->ptr) { msg = "null feature map data"; return 1; }
  return 0;
}

// validates the lines and lays the patches out; c: channels of the output
int make_plan(const lt_patch_config *cfg, long long c, long long n, const double *lines4, PtPlan &plan, std::string &msg) {
  if (check_cfg(cfg, msg)) return 1;
  if (n < 0 || (n > 0 && !lines4)) { msg = "null or negative line array"; return 1; }
  if (c < 1) { msg = "channel count below 1"; return 1; }
  plan.patch_w = cfg->range_perp + 1;
  if ((long long)plan.patch_w * c > (1ll << 24)) { msg = "a patch row of more than 2^24 values"; return 1; }
  plan.geom.assign((size_t)n, PtGeom{});
  plan.off.assign((size_t)n + 1, 0);
  for (long long i = 0; i < n; ++i) {
    const double *l = lines4 + 4 * i;
    const std::string who = "line " + std::to_string(i) + ": ";
    for (int k = 0; k < 4; ++k)
      if (!std::isfinite(l[k])) { msg = who + "non-finite coordinate"; return 1; }
    PtGeom &g = plan.geom[(size_t)i];
    double hd;
    pt_geometry(l[0], l[1], l[2], l[3], cfg->k_stretch, cfg->t_stretch, cfg->range_perp, g, hd);
    bool ok = std::isfinite(hd) && hd >= 1.0 && hd <= (double)kPtMaxH;
    for (int k = 0; k < 4; ++k) ok = ok && std::isfinite(g.R[k]);
    ok = ok && std::isfinite(g.tvec[0]) && std::isfinite(g.tvec[1]);
    if (!ok) { msg = who + "the patch is not finite or has more than " + std::to_string(kPtMaxH) + " rows"; return 1; }
    g.h = (int)hd;
    plan.off[(size_t)i + 1] = plan.off[(size_t)i] + (long long)g.h * plan.patch_w * c;
  }
  return 0;
}

// the block table of the patches [a, b): entries of about kPtBlockItems lane items; out_off relative to patch a
void make_blocks(const PtPlan &plan, long long a, long long b, long long c, int vec_w, std::vector<PtPatch> &patches,
                 std::vector<PtBlock> &blocks) {
  patches.clear();
  blocks.clear();
  const long long per_row = (long long)plan.patch_w * (c / vec_w);
  const int rows_per = (int)std::max<long long>(1, kPtBlockItems / per_row);
  for (long long i = a; i < b; ++i) {
    const PtGeom &g = plan.geom[(size_t)i];
    PtPatch p;
    p.px = g.R[0]; p.py = g.R[1]; p.dx = g.R[2]; p.dy = g.R[3];
    p.cx = g.tvec[0]; p.cy = g.tvec[1];
    p.out_off = plan.off[(size_t)i] - plan.off[(size_t)a];
    p.h = g.h;
    p.pad_ = 0;
    patches.push_back(p);
    for (int y0 = 0; y0 < g.h; y0 += rows_per)
      blocks.push_back(PtBlock{(int)(i - a), y0, std::min(rows_per, g.h - y0), 0});
  }
}

inline double widen(unsigned short v) { return pt_half_bits_to_double(v); }
inline double widen(float v) { return (double)v; }
inline double widen(double v) { return v; }
inline void narrow(double v, unsigned short &o) { o = pt_double_to_half_bits(v); }
inline void narrow(double v, float &o) { o = pt_double_to_float(v); }
inline void narrow(double v, double &o) { o = v; }

template <class Tin, class Tout>
void host_block(const PtMap &map, int patch_w, const PtBlock &b, const PtPatch &p, Tout *out) {
  const Tin *base = static_cast<const Tin *>(map.ptr);
  const long long C = map.c;
  for (int y = b.y0; y < b.y0 + b.rows; ++y)
    for (int x = 0; x < patch_w; ++x) {
      double gx, gy;
      pt_global(p, x, y, gx, gy);
      const PtTaps t = pt_taps(gx, gy, map.h, map.w);
      const Tin *r0 = base + (long long)t.r0 * map.row_stride, *r1 = base + (long long)t.r1 * map.row_stride;
      const long long c0 = (long long)t.c0 * map.pix_stride, c1 = (long long)t.c1 * map.pix_stride;
      Tout *o = out + p.out_off + ((long long)y * patch_w + x) * C;
      for (long long ch = 0; ch < C; ++ch) {
        const long long k = ch * map.chan_stride;
        narrow(pt_blend(t.dx, t.dy, widen(r0[c0 + k]), widen(r0[c1 + k]), widen(r1[c0 + k]), widen(r1[c1 + k])), o[ch]);
      }
    }
}

template <class Tin>
void host_block_in(const PtMap &map, int out_dtype, int patch_w, const PtBlock &b, const PtPatch &p, void *out) {
  if (out_dtype == kPtF16) host_block<Tin, unsigned short>(map, patch_w, b, p, static_cast<unsigned short *>(out));
  else if (out_dtype == kPtF32) host_block<Tin, float>(map, patch_w, b, p, static_cast<float *>(out));
  else host_block<Tin, double>(map, patch_w, b, p, static_cast<double *>(out));
}

PtMap map_of(const lt_feature_map *m) {
  PtMap pm;
  pm.ptr = m->ptr;
  pm.row_stride = m->row_stride; pm.pix_stride = m->pix_stride; pm.chan_stride = m->chan_stride;
  pm.h = (int)m->h; pm.w = (int)m->w; pm.c = (int)m->c; pm.dtype = m->dtype;
  return pm;
}

void copy_geometry(const PtPlan &plan, double *R4, double *tvec2, int32_t *h, int64_t *off) {
  const size_t n = plan.geom.size();
  for (size_t i = 0; i < n; ++i) {
    if (R4) std::memcpy(R4 + 4 * i, plan.geom[i].R, 32);
    if (tvec2) std::memcpy(tvec2 + 2 * i, plan.geom[i].tvec, 16);
    if (h) h[i] = plan.geom[i].h;
  }
  if (off)
    for (size_t i = 0; i <= n; ++i) off[i] = plan.off[i];
}

}  // namespace

extern "C" {

void lt_patch_config_default(lt_patch_config *cfg) {
  if (!cfg) return;
  cfg->k_stretch = 1.0;  // line_patch_extractor.h:28-30
  cfg->t_stretch = 10;
  cfg->range_perp = 20;
}

const char *lt_fn_patch_host_error(void) { return t_err.c_str(); }

int lt_fn_patch_geometry(const lt_patch_config *cfg, int64_t c, int64_t n, const double *lines4, double *R4,
                         double *tvec2, int32_t *h, int64_t *off) {
  t_err.clear();
  PtPlan plan;
  if (make_plan(cfg, c, n, lines4, plan, t_err.text)) return LT_ERR_ARGUMENT;
  copy_geometry(plan, R4, tvec2, h, off);
  return LT_OK;
}

int lt_fn_patch_extract_host(const lt_patch_config *cfg, const lt_feature_map *map, int64_t n, const double *lines4,
                             int32_t out_dtype, void *out, int n_threads) {
  t_err.clear();
  PtPlan plan;
  if (check_map(map, t_err.text) || make_plan(cfg, map->c, n, lines4, plan, t_err.text)) return LT_ERR_ARGUMENT;
  if (!known_dtype(out_dtype)) { t_err.text = "unknown output dtype " + std::to_string(out_dtype); return LT_ERR_ARGUMENT; }
  if (map->on_device) { t_err.text = "lt_fn_patch_extract_host: device feature map"; return LT_ERR_ARGUMENT; }
  if (n > 0 && !out) { t_err.text = "null output"; return LT_ERR_ARGUMENT; }
  std::vector<PtPatch> patches;
  std::vector<PtBlock> blocks;
  make_blocks(plan, 0, n, map->c, 1, patches, blocks);
  const PtMap pm = map_of(map);
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
  const long long nb = (long long)blocks.size();
#pragma omp parallel for num_threads(nt) schedule(dynamic, 4)
  for (long long k = 0; k < nb; ++k) {
    const PtBlock &b = blocks[(size_t)k];
    const PtPatch &p = patches[(size_t)b.patch];
    if (pm.dtype == kPtF16) host_block_in<unsigned short>(pm, out_dtype, plan.patch_w, b, p, out);
    else if (pm.dtype == kPtF32) host_block_in<float>(pm, out_dtype, plan.patch_w, b, p, out);
    else host_block_in<double>(pm, out_dtype, plan.patch_w, b, p, out);
  }
  return LT_OK;
}

int lt_fn_patch_ranges(int64_t n_tracks, const double *line6, const int64_t *sup_off, const int32_t *sup_img,
                       const double *sup_seg4, int64_t n_pairs, const int32_t *pair_track, const int32_t *pair_img,
                       const double *pair_cam11, double *range4, int32_t *status) {
  t_err.clear();
  if (n_tracks < 0 || n_pairs < 0) { t_err.text = "negative count"; return LT_ERR_ARGUMENT; }
  if (n_tracks > 0 && (!line6 || !sup_off)) { t_err.text = "null track arrays"; return LT_ERR_ARGUMENT; }
  if (n_pairs > 0 && (!pair_track || !pair_img || !pair_cam11 || !range4 || !status)) {
    t_err.text = "null pair arrays";
    return LT_ERR_ARGUMENT;
  }
  if (n_tracks > 0) {
    if (sup_off[0] != 0) { t_err.text = "support offsets must start at 0"; return LT_ERR_ARGUMENT; }
    for (int64_t t = 0; t < n_tracks; ++t)
      if (sup_off[t + 1] < sup_off[t]) { t_err.text = "support offsets decrease"; return LT_ERR_ARGUMENT; }
    if (sup_off[n_tracks] > 0 && (!sup_img || !sup_seg4)) { t_err.text = "null support arrays"; return LT_ERR_ARGUMENT; }
    for (int64_t k = 0; k < 6 * n_tracks; ++k)
      if (!std::isfinite(line6[k])) { t_err.text = "track " + std::to_string(k / 6) + ": non-finite 3D line"; return LT_ERR_ARGUMENT; }
    for (int64_t k = 0; k < 4 * sup_off[n_tracks]; ++k)
      if (!std::isfinite(sup_seg4[k])) { t_err.text = "support " + std::to_string(k / 4) + ": non-finite 2D line"; return LT_ERR_ARGUMENT; }
  }
  for (int64_t i = 0; i < n_pairs; ++i) {
    if (pair_track[i] < 0 || pair_track[i] >= n_tracks) {
      t_err.text = "pair " + std::to_string(i) + ": track index outside the table";
      return LT_ERR_ARGUMENT;
    }
    for (int k = 0; k < 11; ++k)
      if (!std::isfinite(pair_cam11[11 * i + k])) { t_err.text = "pair " + std::to_string(i) + ": non-finite camera"; return LT_ERR_ARGUMENT; }
  }
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < n_pairs; ++i) {
    const double *cam = pair_cam11 + 11 * i;
    Cam c;
    cam_build(cam, cam + 4, cam + 8, &c);
    const int64_t t = pair_track[i], s0 = sup_off[t];
    status[i] = pt_range(c, line6 + 6 * t, sup_off[t + 1] - s0, sup_seg4 ? sup_seg4 + 4 * s0 : nullptr,
                         sup_img ? sup_img + s0 : nullptr, pair_img[i], range4 + 4 * i);
  }
  return LT_OK;
}

#ifndef LT_HOST_ONLY

using namespace lt_impl;

int lt_patch_extract(lt_ctx *ctx, const lt_patch_config *cfg, const lt_feature_map *map, int64_t n, const double *lines4,
                     int32_t out_dtype, void *out, int32_t out_on_device, int64_t max_chunk_bytes) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::string who = "lt_patch_extract: ";
  std::string msg;
  const double t0 = now_ms();
  lt_host::PtState &pt = ctx->pt;
  PtPlan plan;
  if (check_map(map, msg) || make_plan(cfg, map->c, n, lines4, plan, msg)) return fail(ctx, LT_ERR_ARGUMENT, who + msg);
  if (!known_dtype(out_dtype)) return fail(ctx, LT_ERR_ARGUMENT, who + "unknown output dtype " + std::to_string(out_dtype));
  if (out && out_on_device && (reinterpret_cast<uintptr_t>(out) & 15u) != 0)
    return fail(ctx, LT_ERR_ARGUMENT, who + "a device output must lie on a 16-byte boundary");
  void *out_host = out_on_device ? nullptr : out;
  void *out_dev = out_on_device ? out : nullptr;
  for (double &t : pt.timers) t = 0.0;
  pt.geom = plan.geom;  // kept for lt_patch_get_geometry
  pt.off = plan.off;
  pt.out_dtype = out_dtype;
  pt.resident_bytes = -1;
  const long long osz = elem_size(out_dtype), total = plan.off[(size_t)n] * osz;
  pt.timers[3] = (double)n;
  pt.timers[7] = (double)total;
  if (n == 0) {
    if (!out) pt.resident_bytes = 0;
    return LT_OK;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;

  // ---- the map as the kernel reads it: a device map in place, a host map packed (h, w, c) and uploaded ----
  PtMap pm = map_of(map);
  const long long isz = elem_size(map->dtype);
  if (!map->on_device) {
    const long long H = map->h, W = map->w, C = map->c;
    const size_t bytes = (size_t)(H * W * C * isz);
    ENSURE(ctx, pt.d_map, bytes);
    const void *src = map->ptr;
    if (!(map->chan_stride == 1 && map->pix_stride == C && map->row_stride == W * C)) {
      pt.h_map.resize(bytes);
      const unsigned char *s = static_cast<const unsigned char *>(map->ptr);
      unsigned char *d = pt.h_map.data();
#pragma omp parallel for schedule(static)
      for (long long r = 0; r < H; ++r)
        for (long long x = 0; x < W; ++x)
          for (long long ch = 0; ch < C; ++ch)
            std::memcpy(d + ((r * W + x) * C + ch) * isz,
                        s + (r * map->row_stride + x * map->pix_stride + ch * map->chan_stride) * isz, (size_t)isz);
      src = pt.h_map.data();
    }
    HIPCHK(ctx, hipMemcpyAsync(pt.d_map.p, src, bytes, hipMemcpyHostToDevice, st));
    pm.ptr = pt.d_map.p;
    pm.chan_stride = 1; pm.pix_stride = C; pm.row_stride = W * C;
  }
  const int lane_c = (int)(16 / isz);
  const bool vec = pm.chan_stride == 1 && pm.c % lane_c == 0 && (reinterpret_cast<uintptr_t>(pm.ptr) & 15u) == 0 &&
                   (pm.row_stride * isz) % 16 == 0 && (pm.pix_stride * isz) % 16 == 0;
  const int vec_w = vec ? lane_c : 1;

  // ---- chunks of whole patches under the byte budget (one chunk of everything when the output stays on the device) ----
  const long long budget = max_chunk_bytes > 0 ? max_chunk_bytes : (1ll << 30);
  std::vector<long long> cut{0};
  if (!out_host) {
    cut.push_back(n);
  } else {
    long long a = 0;
    while (a < n) {
      long long b = a + 1;
      while (b < n && (plan.off[(size_t)b + 1] - plan.off[(size_t)a]) * osz <= budget) ++b;
      cut.push_back(b);
      a = b;
    }
  }
  long long most = 0;
  for (size_t k = 0; k + 1 < cut.size(); ++k)
    most = std::max(most, (plan.off[(size_t)cut[k + 1]] - plan.off[(size_t)cut[k]]) * osz);
  if (!out_dev) ENSURE(ctx, pt.d_out, (size_t)std::max<long long>(most, 16));
  double t_kernel = 0.0, t_down = 0.0, blocks_total = 0.0;
  const double t1 = now_ms();
  std::vector<PtPatch> patches;
  std::vector<PtBlock> blocks;
  for (size_t k = 0; k + 1 < cut.size(); ++k) {
    const long long a = cut[k], b = cut[k + 1];
    make_blocks(plan, a, b, pm.c, vec_w, patches, blocks);
    if (blocks.size() > (size_t)INT_MAX) return fail(ctx, LT_ERR_ARGUMENT, who + "more blocks than one launch takes");
    if (int rc = upload_vec(ctx, pt.d_patches, patches)) return rc;
    if (int rc = upload_vec(ctx, pt.d_blocks, blocks)) return rc;
    Events<2> ev;
    if (int rc = ev.create(ctx)) return rc;
    if (int rc = ev.record(ctx, 0)) return rc;
    launch_patch_gather(st, pm, out_dtype, vec ? 1 : 0, plan.patch_w, (int)blocks.size(), pt.d_blocks.as<PtBlock>(),
                        pt.d_patches.as<PtPatch>(), out_dev ? out_dev : pt.d_out.p);
    if (int rc = ev.record(ctx, 1)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
    t_kernel += ev.ms(0, 1);
    blocks_total += (double)blocks.size();
    if (out_host) {
      const double t2 = now_ms();
      const long long bytes = (plan.off[(size_t)b] - plan.off[(size_t)a]) * osz;
      HIPCHK(ctx, hipMemcpyAsync(static_cast<unsigned char *>(out_host) + plan.off[(size_t)a] * osz, pt.d_out.p,
                                 (size_t)bytes, hipMemcpyDeviceToHost, st));
      if (int rc = stream_sync(ctx)) return rc;
      t_down += now_ms() - t2;
    }
  }
  if (!out) pt.resident_bytes = total;
  pt.timers[0] = t1 - t0;
  pt.timers[1] = t_kernel;
  pt.timers[2] = t_down;
  pt.timers[4] = (double)(cut.size() - 1);
  pt.timers[5] = vec ? 1.0 : 0.0;
  pt.timers[6] = blocks_total;
  return LT_OK;
}

int lt_patch_get_geometry(lt_ctx *ctx, double *R4, double *tvec2, int32_t *h, int64_t *off) {
  if (!ctx) return LT_ERR_ARGUMENT;
  PtPlan plan;
  plan.geom = ctx->pt.geom;
  plan.off = ctx->pt.off;
  if (plan.off.empty()) plan.off.assign(1, 0);
  copy_geometry(plan, R4, tvec2, h, off);
  return LT_OK;
}

int lt_patch_get_device_out(lt_ctx *ctx, void **ptr, int64_t *bytes) {
  if (!ctx || !ptr || !bytes) return ctx ? fail(ctx, LT_ERR_ARGUMENT, "lt_patch_get_device_out: null argument") : LT_ERR_ARGUMENT;
  if (ctx->pt.resident_bytes < 0)
    return fail(ctx, LT_ERR_STATE, "lt_patch_get_device_out: the last lt_patch_extract left no output on the device");
  *ptr = ctx->pt.d_out.p;
  *bytes = ctx->pt.resident_bytes;
  return LT_OK;
}

int lt_patch_get_out(lt_ctx *ctx, void *dst) {
  if (!ctx) return LT_ERR_ARGUMENT;
  if (ctx->pt.resident_bytes < 0)
    return fail(ctx, LT_ERR_STATE, "lt_patch_get_out: the last lt_patch_extract left no output on the device");
  if (ctx->pt.resident_bytes == 0) return LT_OK;
  if (!dst) return fail(ctx, LT_ERR_ARGUMENT, "lt_patch_get_out: null destination");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(dst, ctx->pt.d_out.p, (size_t)ctx->pt.resident_bytes, hipMemcpyDeviceToHost, ctx->stream));
  return stream_sync(ctx);
}

int lt_patch_get_timers(lt_ctx *ctx, double out[8]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 8; ++k) out[k] = ctx->pt.timers[k];
  return LT_OK;
}

int lt_patch_copy_yardstick(lt_ctx *ctx, int64_t bytes, double *ms) {
  if (!ctx || !ms || bytes < 16) return ctx ? fail(ctx, LT_ERR_ARGUMENT, "lt_patch_copy_yardstick: bad arguments") : LT_ERR_ARGUMENT;
  lt_host::PtState &pt = ctx->pt;
  const long long n16 = bytes / 16;
  if ((n16 + kPtBlock - 1) / kPtBlock > (long long)INT32_MAX)
    return fail(ctx, LT_ERR_ARGUMENT, "lt_patch_copy_yardstick: more bytes than one launch takes");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ENSURE(ctx, pt.d_ys_src, 16 * (size_t)n16);
  ENSURE(ctx, pt.d_ys_dst, 16 * (size_t)n16);
  HIPCHK(ctx, hipMemsetAsync(pt.d_ys_src.p, 1, 16 * (size_t)n16, ctx->stream));
  Events<2> ev;
  if (int rc = ev.create(ctx)) return rc;
  if (int rc = ev.record(ctx, 0)) return rc;
  launch_patch_copy16(ctx->stream, n16, pt.d_ys_src.p, pt.d_ys_dst.p);
  if (int rc = ev.record(ctx, 1)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  *ms = ev.ms(0, 1);
  return LT_OK;
}

#endif  // LT_HOST_ONLY

}  // extern "C"
