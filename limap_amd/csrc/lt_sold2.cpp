// lt_sold2.cpp -- limap_amd.line2d: SOLD2 line detection from junctions and line heatmaps (LineSegmentDetectionModule of
// line2d/SOLD2/model/line_detection.py) and the descriptor sampling of WunschLineMatcher.compute_descriptors.
// DESIGN §23 is the definition.  This unit holds the validation and the tables both paths start from, the device entry
// (lt_sold2_detect_scene, lt_sold2_descinfo_scene: one launch of every kernel of lt_kernels_sold2.hip for a whole scene),
// the host restatement from the same inline expressions of lt_sold2.h (lt_fn_sold2_detect_host,
// lt_fn_sold2_descinfo_host) and the getters.

#include "lt_host.h"
#include "lt_twin.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include <omp.h>

using namespace lt;
using namespace lt_impl;
using lt_host::S2Result;

namespace {

thread_local HostError t_err;
thread_local S2Result t_res;

struct Prep {
  S2Cfg cfg;
  std::vector<S2Img> imgs;
  std::vector<int> blk_img;
  long long n_pairs = 0, n_blocks = 0, max_pairs = 0, max_pixels = 0, heat_floats = 0, junc_floats = 0;
  bool refine_heat = false, suppress = false, refine_junc = false;
};

std::string key_msg(const char *key, const std::string &what) { return std::string("line2d: ") + key + " " + what; }

// validation and the tables of a scene; "" or the message of the ValueError (it names the key)
std::string prepare(const lt_sold2_config *c, int n_img, const lt_sold2_image *imgs, bool host, Prep &pr) {
  if (!c || n_img < 0 || (n_img > 0 && !imgs)) return "line2d: null configuration or image table";
  if (c->num_samples < 2 || c->num_samples > kS2MaxSamples)
    return key_msg("num_samples", "outside 2 .. 64: " + std::to_string(c->num_samples));
  if (!c->sampler) return key_msg("num_samples", "has no sampler");
  if (c->sampling_method != 0 && c->sampling_method != 1) return key_msg("sampling_method", "is unknown");
  if (c->max_local_patch_radius < 0 || c->max_local_patch_radius > kS2MaxRadius)
    return key_msg("max_local_patch_radius", "outside 0 .. 4: " + std::to_string(c->max_local_patch_radius));
  pr.refine_heat = c->use_heatmap_refinement != 0;
  pr.suppress = c->use_candidate_suppression != 0;
  pr.refine_junc = c->use_junction_refinement != 0;
  if (pr.refine_junc) {
    if (c->num_perturbs < 1 || c->num_perturbs > kS2MaxPerturbs || c->num_perturbs % 2 == 0)
      return key_msg("num_perturbs", "must be odd and at most 9: " + std::to_string(c->num_perturbs));
    if (!c->perturb_vec) return key_msg("num_perturbs", "has no perturbation vector");
  }
  int nb = 0;
  if (pr.refine_heat) {
    if (c->refine_mode != 0 && c->refine_mode != 1) return key_msg("mode", "of heatmap_refine_cfg is unknown");
    nb = c->refine_mode == 0 ? 1 : c->refine_num_blocks;
    if (nb < 1 || nb > kS2MaxBlocks) return key_msg("num_blocks", "outside 1 .. 32: " + std::to_string(nb));
    if (!(c->refine_ratio > 0.0) || !(c->refine_ratio <= 1.0)) return key_msg("ratio", "outside (0, 1]");
    if (!(c->refine_valid_thresh >= 0.0)) return key_msg("valid_thresh", "is negative");
    if (c->refine_mode == 1 && !(c->refine_overlap_ratio >= 0.0 && c->refine_overlap_ratio < 1.0))
      return key_msg("overlap_ratio", "outside [0, 1)");
  }
  S2Cfg &k = pr.cfg;
  std::memset(&k, 0, sizeof(k));
  k.detect_thresh = (float)c->detect_thresh;
  k.inlier_thresh = (float)c->inlier_thresh;
  k.lambda_radius = (float)c->lambda_radius;
  k.nms_tol = (float)c->nms_dist_tolerance;
  k.valid_thresh = (float)c->refine_valid_thresh;
  k.patch_c = (float)(0.5 * std::sqrt(2.0));
  k.ratio = c->refine_ratio;
  k.num_samples = c->num_samples;
  k.bilinear = c->sampling_method;
  k.radius = c->max_local_patch_radius;
  k.num_perturbs = pr.refine_junc ? c->num_perturbs : 1;
  k.win_floats = c->lds_window_floats < 0 ? kS2WinFloats : std::min<int>(c->lds_window_floats, kS2WinFloats);
  for (int s = 0; s < c->num_samples; ++s) k.sampler[s] = c->sampler[s];
  if (!all_finite(k.sampler, c->num_samples)) return key_msg("num_samples", "has a non-finite sampler");
  if (pr.refine_junc) {
    for (int s = 0; s < c->num_perturbs; ++s) k.perturb[s] = c->perturb_vec[s];
    if (!all_finite(k.perturb, c->num_perturbs)) return key_msg("perturb_interval", "is not finite");
  }
  if (n_img > 65535) return "line2d: more than 65535 images in one call";
  pr.imgs.assign((size_t)n_img, S2Img{});
  for (int i = 0; i < n_img; ++i) {
    const lt_sold2_image &in = imgs[i];
    const std::string who = "line2d: image " + std::to_string(i) + ": ";
    if (in.n_junc < 0 || in.n_junc > 46340 || (in.n_junc > 0 && !in.junctions)) return who + "junctions must be (n, 2)";
    if (in.H < 1 || in.W < 1 || in.H > kS2MaxDim || in.W > kS2MaxDim || !in.heatmap || in.heat_stride < in.W)
      return who + "the heatmap must be 2-D with H, W in 1 .. 32768";
    if (!host && (in.cand_in || in.det_in)) return who + "cand_in / det_in are taken by the host form only";
    if (host && in.on_device) return who + "the host form reads host memory";
    if (!in.on_device && !all_finite(in.junctions, 2ll * in.n_junc)) return who + "junctions must be (n, 2) and finite";
    S2Img &m = pr.imgs[(size_t)i];
    m.n = in.n_junc;
    m.H = in.H;
    m.W = in.W;
    m.heat = in.heatmap;
    m.junc = in.junctions;
    m.heat_stride = in.heat_stride;
    m.diag = (float)std::sqrt((double)((long long)in.H * in.H + (long long)in.W * in.W));
    m.pair0 = pr.n_pairs;
    m.blk0 = pr.n_blocks;
    m.nb = nb;
    const long long np = (long long)m.n * (m.n - 1) / 2;
    pr.n_pairs += np;
    pr.max_pairs = std::max(pr.max_pairs, np);
    pr.max_pixels = std::max(pr.max_pixels, (long long)m.H * m.W);
    pr.heat_floats += (long long)m.H * m.W;
    pr.junc_floats += 2ll * m.n;
    if (nb) {
      // the reference's block bounds: Python's round (half to even) is nearbyint in the default rounding mode
      const double inc = c->refine_mode == 0 ? 1.0 : 1.0 - c->refine_overlap_ratio;
      const double den = 1.0 + (double)(nb - 1) * inc;
      const long long hb = (long long)std::nearbyint((double)m.H / den), wb = (long long)std::nearbyint((double)m.W / den);
      for (int a = 0; a < nb; ++a) {
        const long long r0 = (long long)std::nearbyint((double)(a * hb) * inc), c0 = (long long)std::nearbyint((double)(a * wb) * inc);
        const long long r1 = a < nb - 1 ? r0 + hb : m.H, c1 = a < nb - 1 ? c0 + wb : m.W;
        m.r0[a] = (int)std::min<long long>(r0, m.H);
        m.r1[a] = (int)std::min<long long>(r1, m.H);
        m.c0[a] = (int)std::min<long long>(c0, m.W);
        m.c1[a] = (int)std::min<long long>(c1, m.W);
        if (m.r1[a] <= m.r0[a] || m.c1[a] <= m.c0[a])
          return who + "num_blocks leaves an empty block (" + std::to_string(nb) + " blocks of a " + std::to_string(m.H) +
                 " x " + std::to_string(m.W) + " heatmap)";
      }
      for (int b = 0; b < nb * nb; ++b) pr.blk_img.push_back(i);
      pr.n_blocks += (long long)nb * nb;
    }
  }
  if (pr.n_pairs > (long long)UINT32_MAX / 2) return "line2d: more junction pairs than one call takes";
  return std::string();
}

void fill_meta(const Prep &pr, S2Result &res) {
  res.meta.clear();
  long long heat0 = 0;
  for (const S2Img &m : pr.imgs) {
    res.meta.push_back(S2Result::Meta{m.n, m.H, m.W, m.pair0, heat0, m.heat, m.heat_stride});
    heat0 += (long long)m.H * m.W;
  }
  res.refined_on = pr.refine_heat;
}

// ---- the host restatement ----
float host_block_scale(const S2Cfg &k, const S2Img &m, int a, int b, std::vector<float> &vals) {
  vals.clear();
  float vmax = 0.f;
  for (int y = m.r0[a]; y < m.r1[a]; ++y)
    for (int x = m.c0[b]; x < m.c1[b]; ++x) {
      const float v = m.heat[(long long)y * m.heat_stride + x];
      if (v > k.valid_thresh) {
        vals.push_back(v);
        vmax = s2_max(vmax, v);
      }
    }
  if (vals.empty()) return -1.f;
  const long long n = (long long)vals.size();
  long long kk = (long long)std::ceil((double)n * k.ratio);
  kk = std::max<long long>(1, std::min(kk, n));
  std::nth_element(vals.begin(), vals.begin() + (kk - 1), vals.end(), [](float x, float y) { return x > y; });
  const float kth = vals[(size_t)(kk - 1)];
  const int sh = s2_sum_shift(k.valid_thresh, vmax, n);
  unsigned long long sum = 0ull, above = 0ull;
  for (float v : vals)
    if (v > kth) {
      sum += s2_fixed(v, sh);
      ++above;
    }
  return s2_scale(sum + ((unsigned long long)kk - above) * s2_fixed(kth, sh), sh, kk);
}

void host_detect_image(const Prep &pr, const S2Img &m, const lt_sold2_image &in, unsigned char *cand, unsigned char *det) {
  const S2Cfg &k = pr.cfg;
  const int n = m.n;
  const long long np = (long long)n * (n - 1) / 2;
  const S2HeatGlobal heat{m.stage, m.stage_stride};
#pragma omp parallel for schedule(dynamic, 64)
  for (long long p = 0; p < np; ++p) {
    int i, j;
    s2_pair_decode(n, p, i, j);
    const float sh = m.junc[2 * i], sw = m.junc[2 * i + 1], eh = m.junc[2 * j], ew = m.junc[2 * j + 1];
    unsigned char keep = 1;
    if (in.cand_in) {
      keep = in.cand_in[(long long)i * n + j] ? 1 : 0;
    } else if (pr.suppress) {
      for (int t = 0; t < n && keep; ++t)
        if (t != i && t != j && s2_suppresses(sh, sw, eh, ew, m.junc[2 * t], m.junc[2 * t + 1], k.nms_tol)) keep = 0;
    }
    cand[p] = keep;
    if (in.det_in) {
      det[p] = in.det_in[(long long)i * n + j] ? 1 : 0;
      continue;
    }
    if (!keep) {
      det[p] = 0;
      continue;
    }
    float v[kS2Wave];
    int inl = 0;
    for (int s = 0; s < kS2Wave; ++s) {
      v[s] = 0.f;
      if (s >= k.num_samples) continue;
      const float h = s2_sample_pos(sh, eh, k.sampler[s], (float)(m.H - 1));
      const float w = s2_sample_pos(sw, ew, k.sampler[s], (float)(m.W - 1));
      v[s] = k.bilinear ? s2_bilinear(heat, h, w)
                        : s2_local_max(heat, h, w, m.H, m.W, k.radius, s2_dist_thresh(k, sh, sw, eh, ew, m.diag));
      if (v[s] > k.detect_thresh) ++inl;
    }
    const float mean = s2_tree_sum_host(v) / (float)k.num_samples;
    bool ok = mean > k.detect_thresh;
    if (k.inlier_thresh > 0.f) ok = ok && ((float)inl / (float)k.num_samples >= k.inlier_thresh);
    det[p] = ok ? 1 : 0;
  }
}

S2Seg host_refine_segment(const Prep &pr, const S2Img &m, int img, long long p) {
  const S2Cfg &k = pr.cfg;
  int i, j;
  s2_pair_decode(m.n, p, i, j);
  const float sh = m.junc[2 * i], sw = m.junc[2 * i + 1], eh = m.junc[2 * j], ew = m.junc[2 * j + 1];
  if (!pr.refine_junc) return S2Seg{sh, sw, eh, ew, i, j, -1, img};
  const S2HeatGlobal heat{m.stage, m.stage_stride};
  const int P = k.num_perturbs, total = P * P * P * P;
  float best = 0.f;
  int best_idx = -1;
  for (int idx = 0; idx < total; ++idx) {
    float seg[4];
    s2_perturbed(k, idx, sh, sw, eh, ew, m.H, m.W, seg);
    const float sc = s2_perturb_score(k, heat, seg, m.H, m.W);
    if (best_idx < 0 || sc > best) {
      best = sc;
      best_idx = idx;
    }
  }
  float seg[4];
  s2_perturbed(k, best_idx, sh, sw, eh, ew, m.H, m.W, seg);
  return S2Seg{seg[0], seg[1], seg[2], seg[3], i, j, best_idx, img};
}

int host_detect(const lt_sold2_config *c, int n_img, const lt_sold2_image *imgs, int n_threads) {
  Prep pr;
  t_err.text = prepare(c, n_img, imgs, true, pr);
  if (!t_err.text.empty()) return LT_ERR_ARGUMENT;
  const int saved = omp_get_max_threads();
  if (n_threads > 0) omp_set_num_threads(n_threads);
  S2Result &res = t_res;
  fill_meta(pr, res);
  res.cand.assign((size_t)pr.n_pairs, 0);
  res.det.assign((size_t)pr.n_pairs, 0);
  res.refined.assign(pr.refine_heat ? (size_t)pr.heat_floats : 0, 0.f);
  res.seg_off.assign((size_t)n_img + 1, 0);
  res.segs.clear();
  std::vector<float> scales((size_t)pr.n_blocks, 0.f);
  for (int i = 0; i < n_img; ++i) {
    S2Img &m = pr.imgs[(size_t)i];
    m.stage = m.heat;
    m.stage_stride = m.heat_stride;
    if (pr.refine_heat) {
      const int nb = m.nb;
#pragma omp parallel
      {
        std::vector<float> vals;
#pragma omp for schedule(dynamic, 1)
        for (int b = 0; b < nb * nb; ++b) scales[(size_t)(m.blk0 + b)] = host_block_scale(pr.cfg, m, b / nb, b % nb, vals);
      }
      float *out = res.refined.data() + res.meta[(size_t)i].heat0;
#pragma omp parallel for
      for (int y = 0; y < m.H; ++y)
        for (int x = 0; x < m.W; ++x)
          out[(long long)y * m.W + x] = s2_refined_pixel(m, scales.data(), y, x, m.heat[(long long)y * m.heat_stride + x]);
      m.stage = out;
      m.stage_stride = m.W;
    }
    host_detect_image(pr, m, imgs[i], res.cand.data() + m.pair0, res.det.data() + m.pair0);
    const long long np = (long long)m.n * (m.n - 1) / 2;
    std::vector<long long> list;
    for (long long p = 0; p < np; ++p)
      if (res.det[(size_t)(m.pair0 + p)]) list.push_back(p);
    const size_t base = res.segs.size();
    res.segs.resize(base + list.size());
#pragma omp parallel for schedule(dynamic, 1)
    for (long long s = 0; s < (long long)list.size(); ++s) res.segs[base + (size_t)s] = host_refine_segment(pr, m, i, list[(size_t)s]);
    res.seg_off[(size_t)i + 1] = (long long)res.segs.size();
  }
  if (n_threads > 0) omp_set_num_threads(saved);
  return LT_OK;
}

const S2Result *result_of(lt_ctx *ctx) { return ctx ? &ctx->s2.res : &t_res; }

int bad_image(lt_ctx *ctx, const char *who) {
  const std::string msg = std::string(who) + ": no such image in the last detection";
  if (ctx) return fail(ctx, LT_ERR_ARGUMENT, msg);
  t_err.text = msg;
  return LT_ERR_ARGUMENT;
}

void desc_point_host(const lt_sold2_desc_image &d, long long p) {
  const float iy = s2_desc_coord(d.points[2 * p], (float)(d.Hd * d.grid_size), d.Hd);
  const float ix = s2_desc_coord(d.points[2 * p + 1], (float)(d.Wd * d.grid_size), d.Wd);
  float acc[kS2Wave];
  for (int l = 0; l < kS2Wave; ++l) {
    acc[l] = 0.f;
    for (int ch = l; ch < d.C; ch += kS2Wave) {
      const float v = s2_desc_sample(d.map, d.Hd, d.Wd, d.C, iy, ix, ch);
      acc[l] = acc[l] + v * v;
    }
  }
  const float norm = sqrtf(s2_tree_sum_host(acc));
  const float den = norm > 1e-12f ? norm : 1e-12f;
  for (int ch = 0; ch < d.C; ++ch) d.out[(long long)ch * d.n_points + p] = s2_desc_sample(d.map, d.Hd, d.Wd, d.C, iy, ix, ch) / den;
}

std::string check_desc(int n_img, const lt_sold2_desc_image *imgs, bool host) {
  if (n_img < 0 || (n_img > 0 && !imgs)) return "line2d: null descriptor table";
  for (int i = 0; i < n_img; ++i) {
    const lt_sold2_desc_image &d = imgs[i];
    const std::string who = "line2d: descriptor image " + std::to_string(i) + ": ";
    if (d.Hd < 1 || d.Wd < 1 || d.C < 1 || d.grid_size < 1 || d.Hd > kS2MaxDim || d.Wd > kS2MaxDim || d.C > 4096 || !d.map)
      return who + "the descriptor map must be (1, C, H, W) with C <= 4096";
    if (d.n_points < 0 || (d.n_points > 0 && (!d.points || !d.out))) return who + "null points or output";
    if (host && d.on_device) return who + "the host form reads host memory";
    if (!all_finite(d.points, 2 * d.n_points)) return who + "non-finite point";
  }
  return std::string();
}

}  // namespace

extern "C" {

int lt_fn_sold2_detect_host(const lt_sold2_config *cfg, int n_img, const lt_sold2_image *imgs, int n_threads) {
  return host_detect(cfg, n_img, imgs, n_threads);
}

const char *lt_fn_sold2_host_error(void) { return t_err.c_str(); }

int lt_fn_sold2_samples_host(const lt_sold2_config *cfg, const lt_sold2_image *img, int64_t n_pairs, const int32_t *pairs2,
                             float *pos, float *values) {
  Prep pr;
  t_err.text = prepare(cfg, 1, img, true, pr);
  if (t_err.text.empty() && (n_pairs < 0 || (n_pairs > 0 && (!pairs2 || !pos || !values)))) t_err.text = "line2d: null pairs or outputs";
  if (!t_err.text.empty()) return LT_ERR_ARGUMENT;
  const S2Cfg &k = pr.cfg;
  const S2Img &m = pr.imgs[0];
  for (int64_t p = 0; p < n_pairs; ++p)
    if (pairs2[2 * p] < 0 || pairs2[2 * p] >= m.n || pairs2[2 * p + 1] < 0 || pairs2[2 * p + 1] >= m.n) {
      t_err.text = "line2d: a pair names no junction";
      return LT_ERR_ARGUMENT;
    }
  const S2HeatGlobal heat{m.heat, m.heat_stride};
  const int S = k.num_samples;
#pragma omp parallel for
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int i = pairs2[2 * p], j = pairs2[2 * p + 1];
    const float sh = m.junc[2 * i], sw = m.junc[2 * i + 1], eh = m.junc[2 * j], ew = m.junc[2 * j + 1];
    for (int s = 0; s < S; ++s) {
      const float h = s2_sample_pos(sh, eh, k.sampler[s], (float)(m.H - 1));
      const float w = s2_sample_pos(sw, ew, k.sampler[s], (float)(m.W - 1));
      pos[2 * (p * S + s)] = h;
      pos[2 * (p * S + s) + 1] = w;
      values[p * S + s] = k.bilinear ? s2_bilinear(heat, h, w)
                                     : s2_local_max(heat, h, w, m.H, m.W, k.radius, s2_dist_thresh(k, sh, sw, eh, ew, m.diag));
    }
  }
  return LT_OK;
}

int lt_fn_sold2_block_scales_host(const lt_sold2_config *cfg, const lt_sold2_image *img, float *scales, int32_t *bounds4) {
  Prep pr;
  t_err.text = prepare(cfg, 1, img, true, pr);
  if (t_err.text.empty() && (!pr.refine_heat || !scales || !bounds4)) t_err.text = "line2d: heatmap refinement is off or an output is null";
  if (!t_err.text.empty()) return LT_ERR_ARGUMENT;
  const S2Img &m = pr.imgs[0];
  std::vector<float> vals;
  for (int b = 0; b < m.nb * m.nb; ++b) scales[b] = host_block_scale(pr.cfg, m, b / m.nb, b % m.nb, vals);
  for (int a = 0; a < m.nb; ++a) {
    bounds4[4 * a] = m.r0[a];
    bounds4[4 * a + 1] = m.r1[a];
    bounds4[4 * a + 2] = m.c0[a];
    bounds4[4 * a + 3] = m.c1[a];
  }
  return LT_OK;
}

int lt_sold2_detect_scene(lt_ctx *ctx, const lt_sold2_config *cfg, int n_img, const lt_sold2_image *imgs) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const double t0 = now_ms();
  Prep pr;
  const std::string msg = prepare(cfg, n_img, imgs, false, pr);
  if (!msg.empty()) return fail(ctx, LT_ERR_ARGUMENT, msg);
  lt_host::S2State &s2 = ctx->s2;
  S2Result &res = s2.res;
  for (double &t : s2.kernel_ms) t = 0.0;
  fill_meta(pr, res);
  res.refined.clear();
  res.seg_off.assign((size_t)n_img + 1, 0);
  res.segs.clear();
  res.cand.clear();
  res.det.clear();
  s2.dev_heat.assign((size_t)n_img, nullptr);
  s2.dev_stride.assign((size_t)n_img, 0);
  if (n_img == 0) return LT_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;

  // ---- staging: host junctions and heatmaps are packed behind one another and uploaded once; device ones are read
  // in place ----
  long long host_heat = 0, host_junc = 0;
  for (int i = 0; i < n_img; ++i)
    if (!imgs[i].on_device) {
      host_heat += (long long)imgs[i].H * imgs[i].W;
      host_junc += 2ll * imgs[i].n_junc;
    }
  s2.h_heat.resize((size_t)host_heat);
  s2.h_junc.resize((size_t)host_junc);
  ENSURE(ctx, s2.d_heat, 4 * (size_t)std::max<long long>(host_heat, 1));
  ENSURE(ctx, s2.d_junc, 4 * (size_t)std::max<long long>(host_junc, 1));
  ENSURE(ctx, s2.d_refined, 4 * (size_t)std::max<long long>(pr.refine_heat ? pr.heat_floats : 0, 1));
  long long ho = 0, jo = 0, ro = 0;
  for (int i = 0; i < n_img; ++i) {
    S2Img &m = pr.imgs[(size_t)i];
    if (!imgs[i].on_device) {
      for (int y = 0; y < m.H; ++y)
        std::memcpy(s2.h_heat.data() + ho + (long long)y * m.W, imgs[i].heatmap + (long long)y * imgs[i].heat_stride, 4 * (size_t)m.W);
      if (m.n) std::memcpy(s2.h_junc.data() + jo, imgs[i].junctions, 8 * (size_t)m.n);
      m.heat = s2.d_heat.as<float>() + ho;
      m.heat_stride = m.W;
      m.junc = s2.d_junc.as<float>() + jo;
      ho += (long long)m.H * m.W;
      jo += 2ll * m.n;
    }
    m.stage = m.heat;
    m.stage_stride = m.heat_stride;
    if (pr.refine_heat) {
      m.refined = s2.d_refined.as<float>() + ro;
      m.stage = m.refined;
      m.stage_stride = m.W;
      ro += (long long)m.H * m.W;
    }
    s2.dev_heat[(size_t)i] = m.stage;
    s2.dev_stride[(size_t)i] = m.stage_stride;
  }
  if (host_heat) HIPCHK(ctx, hipMemcpyAsync(s2.d_heat.p, s2.h_heat.data(), 4 * (size_t)host_heat, hipMemcpyHostToDevice, st));
  if (host_junc) HIPCHK(ctx, hipMemcpyAsync(s2.d_junc.p, s2.h_junc.data(), 4 * (size_t)host_junc, hipMemcpyHostToDevice, st));
  std::vector<S2Cfg> cfgv(1, pr.cfg);
  if (int rc = upload_vec(ctx, s2.d_cfg, cfgv)) return rc;
  if (int rc = upload_vec(ctx, s2.d_imgs, pr.imgs)) return rc;
  if (int rc = upload_vec(ctx, s2.d_blk_img, pr.blk_img)) return rc;
  const size_t NP = (size_t)std::max<long long>(pr.n_pairs, 1);
  ENSURE(ctx, s2.d_scales, 4 * (size_t)std::max<long long>(pr.n_blocks, 1));
  ENSURE(ctx, s2.d_cand, NP);
  ENSURE(ctx, s2.d_det, NP);
  ENSURE(ctx, s2.d_list, 4 * NP);
  ENSURE(ctx, s2.d_seg_off, 8 * ((size_t)n_img + 1));
  const S2Img *d_imgs = s2.d_imgs.as<S2Img>();
  const S2Cfg *d_cfg = s2.d_cfg.as<S2Cfg>();

  Events<7> ev;
  if (int rc = ev.create(ctx)) return rc;
  if (int rc = ev.record(ctx, 0)) return rc;
  if (pr.refine_heat) {
    launch_s2_block_scale(st, pr.n_blocks, d_imgs, s2.d_blk_img.as<int>(), d_cfg, s2.d_scales.as<float>());
    if (int rc = ev.record(ctx, 1)) return rc;
    const int gx = (int)std::min<long long>((pr.max_pixels + kS2Block - 1) / kS2Block, 4096);
    launch_s2_refine_pixels(st, n_img, gx, d_imgs, s2.d_scales.as<float>());
  } else if (int rc = ev.record(ctx, 1)) {
    return rc;
  }
  if (int rc = ev.record(ctx, 2)) return rc;
  if (pr.suppress)
    launch_s2_suppress(st, n_img, pr.max_pairs, d_imgs, d_cfg, s2.d_cand.as<unsigned char>());
  else
    HIPCHK(ctx, hipMemsetAsync(s2.d_cand.p, 1, NP, st));
  if (int rc = ev.record(ctx, 3)) return rc;
  launch_s2_score(st, n_img, pr.max_pairs, d_imgs, d_cfg, s2.d_cand.as<unsigned char>(), s2.d_det.as<unsigned char>());
  if (int rc = ev.record(ctx, 4)) return rc;
  launch_s2_compact(st, n_img, d_imgs, s2.d_det.as<unsigned char>(), s2.d_list.as<unsigned>(), s2.d_seg_off.as<long long>());
  if (int rc = ev.record(ctx, 5)) return rc;
  // the segment count stays on the device: a fixed grid strides over the segments
  ENSURE(ctx, s2.d_segs, sizeof(S2Seg) * NP);
  const int grid = (int)std::min<long long>(pr.n_pairs, 2048);
  launch_s2_refine_junc(st, n_img, grid, d_imgs, d_cfg, s2.d_list.as<unsigned>(), s2.d_seg_off.as<long long>(),
                        s2.d_segs.as<S2Seg>(), pr.refine_junc ? 1 : 0);
  if (int rc = ev.record(ctx, 6)) return rc;
  if (int rc = download(ctx, res.seg_off, s2.d_seg_off.p, (size_t)n_img + 1)) return rc;
  if (int rc = download(ctx, res.cand, s2.d_cand.p, (size_t)pr.n_pairs)) return rc;
  if (int rc = download(ctx, res.det, s2.d_det.p, (size_t)pr.n_pairs)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  if (int rc = download(ctx, res.segs, s2.d_segs.p, (size_t)res.seg_off[(size_t)n_img])) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  for (int k = 0; k < 6; ++k) s2.kernel_ms[k] = ev.ms(k, k + 1);
  s2.kernel_ms[6] = ev.ms(0, 6);
  s2.kernel_ms[7] = now_ms() - t0;
  return LT_OK;
}

int lt_sold2_get_counts(lt_ctx *ctx, int64_t *counts) {
  const S2Result *r = result_of(ctx);
  if (!counts) return LT_ERR_ARGUMENT;
  for (size_t i = 0; i + 1 < r->seg_off.size(); ++i) counts[i] = r->seg_off[i + 1] - r->seg_off[i];
  return LT_OK;
}

int lt_sold2_get_segments(lt_ctx *ctx, int img, float *segs4, int32_t *pairs2, int32_t *perturb) {
  const S2Result *r = result_of(ctx);
  if (img < 0 || (size_t)img + 1 >= r->seg_off.size()) return bad_image(ctx, "lt_sold2_get_segments");
  for (long long s = r->seg_off[(size_t)img], o = 0; s < r->seg_off[(size_t)img + 1]; ++s, ++o) {
    const S2Seg &g = r->segs[(size_t)s];
    if (segs4) {
      segs4[4 * o] = g.h1;
      segs4[4 * o + 1] = g.w1;
      segs4[4 * o + 2] = g.h2;
      segs4[4 * o + 3] = g.w2;
    }
    if (pairs2) {
      pairs2[2 * o] = g.i;
      pairs2[2 * o + 1] = g.j;
    }
    if (perturb) perturb[o] = g.perturb;
  }
  return LT_OK;
}

int lt_sold2_get_stages(lt_ctx *ctx, int img, float *heat, uint8_t *cand, uint8_t *det) {
  const S2Result *r = result_of(ctx);
  if (img < 0 || (size_t)img >= r->meta.size()) return bad_image(ctx, "lt_sold2_get_stages");
  const S2Result::Meta &m = r->meta[(size_t)img];
  if (heat) {
    if (ctx) {
      HIPCHK(ctx, hipSetDevice(ctx->device));
      HIPCHK(ctx, hipMemcpy2DAsync(heat, 4 * (size_t)m.W, ctx->s2.dev_heat[(size_t)img], 4 * (size_t)ctx->s2.dev_stride[(size_t)img],
                                   4 * (size_t)m.W, (size_t)m.H, hipMemcpyDeviceToHost, ctx->stream));
      if (int rc = stream_sync(ctx)) return rc;
    } else if (r->refined_on) {
      std::memcpy(heat, r->refined.data() + m.heat0, 4 * (size_t)m.H * m.W);
    } else {
      for (int y = 0; y < m.H; ++y) std::memcpy(heat + (long long)y * m.W, m.heat_in + (long long)y * m.heat_stride, 4 * (size_t)m.W);
    }
  }
  for (int pass = 0; pass < 2; ++pass) {
    uint8_t *out = pass ? det : cand;
    if (!out) continue;
    const std::vector<unsigned char> &src = pass ? r->det : r->cand;
    std::memset(out, 0, (size_t)m.n * m.n);
    long long p = m.pair0;
    for (int i = 0; i < m.n; ++i)
      for (int j = i + 1; j < m.n; ++j) out[(long long)i * m.n + j] = src[(size_t)p++];
  }
  return LT_OK;
}

int lt_sold2_get_kernel_ms(lt_ctx *ctx, double out[8]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 8; ++k) out[k] = ctx->s2.kernel_ms[k];
  return LT_OK;
}

int lt_fn_sold2_descinfo_host(int n_img, const lt_sold2_desc_image *imgs, int n_threads) {
  t_err.text = check_desc(n_img, imgs, true);
  if (!t_err.text.empty()) return LT_ERR_ARGUMENT;
  const int saved = omp_get_max_threads();
  if (n_threads > 0) omp_set_num_threads(n_threads);
  for (int i = 0; i < n_img; ++i) {
    const lt_sold2_desc_image &d = imgs[i];
#pragma omp parallel for
    for (long long p = 0; p < d.n_points; ++p) desc_point_host(d, p);
  }
  if (n_threads > 0) omp_set_num_threads(saved);
  return LT_OK;
}

int lt_sold2_descinfo_scene(lt_ctx *ctx, int n_img, const lt_sold2_desc_image *imgs, double *out_ms) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::string msg = check_desc(n_img, imgs, false);
  if (!msg.empty()) return fail(ctx, LT_ERR_ARGUMENT, msg);
  if (out_ms) *out_ms = 0.0;
  if (n_img == 0) return LT_OK;
  lt_host::S2State &s2 = ctx->s2;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  std::vector<long long> pt_off((size_t)n_img + 1, 0), maps((size_t)n_img, 0), out_off((size_t)n_img, 0);
  std::vector<int> dims(4 * (size_t)n_img, 0);
  std::vector<float> pts;
  long long map_floats = 0, out_floats = 0;
  for (int i = 0; i < n_img; ++i) {
    const lt_sold2_desc_image &d = imgs[i];
    pt_off[(size_t)i + 1] = pt_off[(size_t)i] + d.n_points;
    pts.insert(pts.end(), d.points, d.points + 2 * d.n_points);
    dims[4 * (size_t)i] = d.Hd;
    dims[4 * (size_t)i + 1] = d.Wd;
    dims[4 * (size_t)i + 2] = d.C;
    dims[4 * (size_t)i + 3] = d.grid_size;
    if (!d.on_device) {
      map_floats += (long long)d.Hd * d.Wd * d.C;
      out_floats += (long long)d.C * d.n_points;
    }
  }
  ENSURE(ctx, s2.d_map_data, 4 * (size_t)std::max<long long>(map_floats, 1));
  ENSURE(ctx, s2.d_out, 4 * (size_t)std::max<long long>(out_floats, 1));
  long long mo = 0, oo = 0;
  for (int i = 0; i < n_img; ++i) {
    const lt_sold2_desc_image &d = imgs[i];
    if (d.on_device) {
      maps[(size_t)i] = (long long)reinterpret_cast<uintptr_t>(d.map);
      out_off[(size_t)i] = (long long)reinterpret_cast<uintptr_t>(d.out);
    } else {
      const long long nf = (long long)d.Hd * d.Wd * d.C;
      HIPCHK(ctx, hipMemcpyAsync(s2.d_map_data.as<float>() + mo, d.map, 4 * (size_t)nf, hipMemcpyHostToDevice, st));
      maps[(size_t)i] = (long long)reinterpret_cast<uintptr_t>(s2.d_map_data.as<float>() + mo);
      out_off[(size_t)i] = (long long)reinterpret_cast<uintptr_t>(s2.d_out.as<float>() + oo);
      mo += nf;
      oo += (long long)d.C * d.n_points;
    }
  }
  if (int rc = upload_vec(ctx, s2.d_pts, pts)) return rc;
  if (int rc = upload_vec(ctx, s2.d_pt_off, pt_off)) return rc;
  if (int rc = upload_vec(ctx, s2.d_maps, maps)) return rc;
  if (int rc = upload_vec(ctx, s2.d_dims, dims)) return rc;
  if (int rc = upload_vec(ctx, s2.d_out_off, out_off)) return rc;
  Events<2> ev;
  if (int rc = ev.create(ctx)) return rc;
  if (int rc = ev.record(ctx, 0)) return rc;
  launch_s2_descinfo(st, pt_off[(size_t)n_img], n_img, s2.d_pts.as<float>(), s2.d_pt_off.as<long long>(),
                     s2.d_maps.as<long long>(), s2.d_dims.as<int>(), s2.d_out_off.as<long long>());
  if (int rc = ev.record(ctx, 1)) return rc;
  oo = 0;
  for (int i = 0; i < n_img; ++i) {
    const lt_sold2_desc_image &d = imgs[i];
    if (d.on_device) continue;
    const long long nf = (long long)d.C * d.n_points;
    if (nf) HIPCHK(ctx, hipMemcpyAsync(d.out, s2.d_out.as<float>() + oo, 4 * (size_t)nf, hipMemcpyDeviceToHost, st));
    oo += nf;
  }
  if (int rc = stream_sync(ctx)) return rc;
  if (out_ms) *out_ms = ev.ms(0, 1);
  return LT_OK;
}

}  // extern "C"
