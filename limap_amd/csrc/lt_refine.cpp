// lt_refine.cpp -- the geometric refinement of line tracks with constant cameras: step [E] of
// limap.runners.line_triangulation (runners/line_triangulation.py:208-219; HybridBAEngine with set_constant_camera,
// optimize/hybrid_bundle_adjustment/hybrid_bundle_adjustment.cc:39-59,106-123,156-197,298-310) and the geometric terms
// of limap.optimize.line_refinement.  Validation, the residual order (AddLineGeometricResiduals: sorted image ids, then
// the id map's order within an image -- a stable sort of the supports by image id), upload, the three launches of
// lt_kernels_refine.hip and the download; lt_fn_refine_host is the whole step in plain C++ from the same inline functions
// (lt_refine.h) with the reductions in the device's order, so both agree bit for bit.

#include "lt_host.h"
#include "lt_refine.h"
#include "lt_ingest.h"
#include "lt_twin.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include <omp.h>

using namespace lt;
using namespace lt_impl;

namespace {

struct Plan {
  std::vector<RfTrack> tracks;
  std::vector<int> sup_cam;    // residual order
  std::vector<double> l2d;     // 4 per support, residual order
  std::vector<double> l3d;     // 6 per support, list order
  std::vector<double> line6;
  std::vector<long long> src;  // residual order -> the caller's support
  long long n_sup = 0;
};

// the heatmaps a call can read: the caller's (host path) or the context's (device path)
struct HmSet {
  int type = LT_TEXEL_F16;
  std::vector<int> h, w;
  std::vector<long long> off;          // first texel in the packed buffer, n + 1
  std::vector<const void *> data;      // host path: the caller's images
  std::unordered_map<int, int> slot;   // image id -> row
};

// what the terms add to a plan, residual order
struct TermsPlan {
  std::vector<int> vp_flag, sup_hm;
  std::vector<double> vp3;
  RfTermCfg cfg;
};

int check_terms(const lt_refine_terms *t, std::string &msg) {
  if (!t) { msg = "null terms"; return 1; }
  if (!t->use_geometric && !t->use_vp && !t->use_heatmap) { msg = "no term is enabled"; return 1; }
  if (t->use_vp && !std::isfinite(t->vp_multiplier)) { msg = "vp_multiplier is not finite"; return 1; }
  if (t->use_heatmap) {
    if (t->n_samples_heatmap < 2 || t->n_samples_heatmap > 1024) {  // interval = range / (n - 1)
      msg = "n_samples_heatmap outside [2, 1024]";
      return 1;
    }
    if (!std::isfinite(t->heatmap_multiplier)) { msg = "heatmap_multiplier is not finite"; return 1; }
    if (!std::isfinite(t->sample_range_min) || !std::isfinite(t->sample_range_max)) {
      msg = "sample_range is not finite";
      return 1;
    }
    if (t->texel_type != LT_TEXEL_F16 && t->texel_type != LT_TEXEL_F32) { msg = "unknown texel type"; return 1; }
  }
  return 0;
}

int check_heatmaps(int n, const int32_t *ids, const int32_t *h, const int32_t *w, const void *const *data, int type,
                   HmSet &hs, std::string &msg) {
  if (n < 0 || (n > 0 && (!ids || !h || !w || !data))) { msg = "bad heatmap arrays"; return 1; }
  if (type != LT_TEXEL_F16 && type != LT_TEXEL_F32) { msg = "unknown texel type"; return 1; }
  hs.type = type;
  hs.off.assign(1, 0);
  for (int i = 0; i < n; ++i) {
    if (h[i] < 1 || w[i] < 1 || !data[i]) { msg = "heatmap of image " + std::to_string(ids[i]) + " is empty"; return 1; }
    if (!hs.slot.emplace(ids[i], i).second) { msg = "heatmap of image " + std::to_string(ids[i]) + " given twice"; return 1; }
    hs.h.push_back(h[i]);
    hs.w.push_back(w[i]);
    hs.data.push_back(data[i]);
    hs.off.push_back(hs.off.back() + (long long)h[i] * w[i]);
  }
  return 0;
}

// the checks of the terms' per-support input and its tables in residual order; view_hw: (h, w) per camera row, or null,
// an entry <= 0 meaning the view carries no size
int make_terms_plan(const Plan &pl, const int32_t *img, const lt_refine_terms &t, const int32_t *vp_flag, const double *vp3,
                    const int32_t *view_hw, const HmSet *hs, TermsPlan &tp, std::string &msg) {
  const size_t S = (size_t)pl.n_sup;
  tp.vp_flag.assign(S, 0);
  tp.vp3.assign(3 * S, 0.0);
  tp.sup_hm.assign(S, 0);
  if (t.use_vp && S > 0 && (!vp_flag || !vp3)) { msg = "use_vp without VP arrays"; return 1; }
  if (t.use_heatmap && !hs) { msg = "use_heatmap without heatmaps"; return 1; }
  if (t.use_heatmap && hs->type != t.texel_type) { msg = "the heatmaps' texel type is not the terms'"; return 1; }
  for (size_t i = 0; i < S; ++i) {
    const long long src = pl.src[i];
    if (t.use_vp && vp_flag[src]) {
      if (!all_finite(vp3 + 3 * src, 3)) { msg = "non-finite vanishing point"; return 1; }
      tp.vp_flag[i] = 1;
      for (int c = 0; c < 3; ++c) tp.vp3[3 * i + c] = vp3[3 * src + c];
    }
    if (t.use_heatmap) {
      auto it = hs->slot.find(img[src]);
      if (it == hs->slot.end()) { msg = "image " + std::to_string(img[src]) + " supports a track and has no heatmap"; return 1; }
      const int cam = pl.sup_cam[i], sl = it->second;
      // THROW_CHECK_EQ of the heatmap's size against the view's (refine.cc:283-284)
      if (view_hw && view_hw[2 * cam] > 0 && view_hw[2 * cam + 1] > 0 &&
          (view_hw[2 * cam] != hs->h[(size_t)sl] || view_hw[2 * cam + 1] != hs->w[(size_t)sl])) {
        msg = "the heatmap of image " + std::to_string(img[src]) + " has not the size of its view";
        return 1;
      }
      const double *l = pl.l2d.data() + 4 * i;
      const double dx = l[2] - l[0], dy = l[3] - l[1];
      if (!(std::sqrt(dx * dx + dy * dy) > 0.0)) {  // THROW_CHECK_LT(|direc.norm() - 1|, EPS) (infinite_line.cc:10)
        msg = "a 2D support of zero length has no sample lines";
        return 1;
      }
      tp.sup_hm[i] = sl;
    }
  }
  tp.cfg.vp_multiplier = t.vp_multiplier;
  tp.cfg.heatmap_multiplier = t.heatmap_multiplier;
  tp.cfg.n_samples = t.use_heatmap ? t.n_samples_heatmap : 0;
  tp.cfg.heatmap_den = t.n_samples_heatmap / 10.0;
  tp.cfg.t0 = t.sample_range_min;
  tp.cfg.interval = t.use_heatmap ? (t.sample_range_max - t.sample_range_min) / (t.n_samples_heatmap - 1) : 0.0;
  tp.cfg.use_geometric = t.use_geometric != 0;
  tp.cfg.use_vp = t.use_vp != 0;
  tp.cfg.use_heatmap = t.use_heatmap != 0;
  return 0;
}

// ---- the feature-consistency term ----
// the tables of lt::RfDevFeat for a call's tracks; kept[n]: the samples ComputeFConsistencySamples keeps for track n,
// with or without targets (the n_samples of the weight)
struct FeatPlan {
  std::vector<RfFTrack> ftracks;
  std::vector<RfFImg> imgs;
  std::vector<RfFView> views;
  std::vector<RfFSample> smps;
  std::vector<int> tgts;
  std::vector<double> pairs;
  std::vector<int> kept;
  int type = LT_TEXEL_F16;
};

// a kept sample as upstream's tuple: reference image, sample line, targets (images of the track, ascending)
struct FSample {
  int ref;
  double k[3];
  std::vector<int> tgts;
};

int check_feature(const lt_refine_terms *t, const lt_refine_feature *f, std::string &msg) {
  if (!t) { msg = "null terms"; return 1; }
  if (!f) { msg = "null feature configuration"; return 1; }
  if (!f->use_feature) { msg = "use_feature is off"; return 1; }
  if (f->channels != kRfChannels) { msg = "channels must be 128"; return 1; }
  if (f->n_samples_feature < 2 || f->n_samples_feature > 4096) { msg = "n_samples_feature outside [2, 4096]"; return 1; }
  if (!std::isfinite(f->fconsis_multiplier)) { msg = "fconsis_multiplier is not finite"; return 1; }
  if (f->texel_type != LT_TEXEL_F16 && f->texel_type != LT_TEXEL_F32) { msg = "unknown texel type"; return 1; }
  if (!std::isfinite(t->sample_range_min) || !std::isfinite(t->sample_range_max)) { msg = "sample_range is not finite"; return 1; }
  if (t->use_heatmap && t->texel_type != f->texel_type) {
    msg = "the heatmaps' texel type is not the features'";
    return 1;
  }
  if (t->use_geometric || t->use_vp || t->use_heatmap) return check_terms(t, msg);
  return 0;
}

// ComputeFConsistencySamples (linetrack.cc:353-454) for one track: the supports in the caller's list order, ids the
// track's sorted image ids, cams their cameras
int feat_samples(const double *line6, int K, const int32_t *img, const double *l2d4, const std::vector<int> &ids,
                 const std::vector<Cam> &cams, double rmin, double rmax, int n, std::vector<FSample> &out, std::string &msg) {
  out.clear();
  const size_t I = ids.size();
  auto idx_of = [&](int id) { return (size_t)(std::lower_bound(ids.begin(), ids.end(), id) - ids.begin()); };
  const d3 start = mk3(line6[0], line6[1], line6[2]), end = mk3(line6[3], line6[4], line6[5]);
  const double nm1 = (double)(n - 1);
  const d3 interval = mk3((end.x - start.x) / nm1, (end.y - start.y) / nm1, (end.z - start.z) / nm1);
  std::vector<d2> ps(I), pe(I), proj(I);  // track.line.projection(view)
  for (size_t i = 0; i < I; ++i) {
    ps[i] = cam_project(cams[i], start);
    pe[i] = cam_project(cams[i], end);
  }
  std::vector<int> supports, good, timg;
  for (int pi = 0; pi < n; ++pi) {
    const double fi = (double)pi;
    const d3 point = mk3(start.x + fi * interval.x, start.y + fi * interval.y, start.z + fi * interval.z);
    for (size_t i = 0; i < I; ++i) proj[i] = cam_project(cams[i], point);
    supports.clear();
    for (int k = 0; k < K; ++k) {
      const d2 s = mk2(l2d4[4 * k], l2d4[4 * k + 1]), e = mk2(l2d4[4 * k + 2], l2d4[4 * k + 3]);
      const double length = sqrt(sqn(sub(s, e)));
      const d2 dir = unit(sub(e, s));
      const double pr = dot(sub(proj[idx_of(img[k])], s), dir) / length;
      if (pr >= rmin && pr <= rmax) supports.push_back(k);
    }
    if (supports.size() < 2) continue;
    good.clear();
    for (int k : supports) {  // PERPENDICULAR_ONEWAY of the support against the track's projection (line_dists.h:98-119)
      const size_t i = idx_of(img[k]);
      const d2 v2 = unit(sub(pe[i], ps[i]));
      const d2 ds = sub(mk2(l2d4[4 * k], l2d4[4 * k + 1]), ps[i]), de = sub(mk2(l2d4[4 * k + 2], l2d4[4 * k + 3]), ps[i]);
      const double a = dot(ds, v2), b = dot(de, v2);
      const double d12s = sqrt(dmax(sqn(ds) - a * a, 0.0)), d12e = sqrt(dmax(sqn(de) - b * b, 0.0));
      if (dmax(d12s, d12e) < 0.3) good.push_back(k);
    }
    if (good.empty()) continue;
    double max_length = -1.0;
    int max_id = -1;
    for (int k : good) {
      const double length = sqrt(sqn(sub(mk2(l2d4[4 * k], l2d4[4 * k + 1]), mk2(l2d4[4 * k + 2], l2d4[4 * k + 3]))));
      if (length > max_length) { max_length = length; max_id = k; }
    }
    if (max_id < 0) { msg = "a support has no length"; return 1; }  // (a NaN length: upstream indexes image_id_list[-1])
    FSample smp;
    smp.ref = (int)idx_of(img[max_id]);
    const d2 rs = mk2(l2d4[4 * max_id], l2d4[4 * max_id + 1]), re = mk2(l2d4[4 * max_id + 2], l2d4[4 * max_id + 3]);
    const d2 rdir = unit(sub(re, rs));
    const d2 perp = mk2(rdir.y, -rdir.x);
    if (!(std::fabs(sqrt(sqn(perp)) - 1.0) < kEps)) {  // THROW_CHECK_LT(|direc.norm() - 1|, EPS) (infinite_line.cc:10)
      msg = "a 2D support of zero length has no sample line";
      return 1;
    }
    const d2 p = proj[(size_t)smp.ref];
    const d3 coor = unit(mk3(perp.y, (-1.0) * perp.x, ((-1.0) * perp.y) * p.x + perp.x * p.y));  // InfiniteLine2d(p, direc)
    smp.k[0] = coor.x; smp.k[1] = coor.y; smp.k[2] = coor.z;
    timg.clear();
    for (int k : supports) timg.push_back((int)idx_of(img[k]));
    std::sort(timg.begin(), timg.end());
    timg.erase(std::unique(timg.begin(), timg.end()), timg.end());
    for (int i : timg)
      if (i != smp.ref) smp.tgts.push_back(i);
    out.push_back(std::move(smp));
  }
  return 0;
}

// the term's tables for the plan's tracks.  grids: one per (track, sorted image) in track order; all: where given, the
// kept samples of every track (lt_fn_refine_eval_feature)
int make_feat_plan(const Plan &pl, const std::unordered_map<int, int> &id2idx, int n_cams, const double *k4, const double *q4,
                   const double *t3, const int64_t *off, const int32_t *img, const double *l2d4, const lt_refine_terms &t,
                   const lt_refine_feature &f, int64_t n_grids, const lt_refine_grid *grids, bool device, FeatPlan &fp,
                   std::string &msg, std::vector<std::vector<FSample>> *all = nullptr) {
  const size_t T = pl.tracks.size();
  if (n_grids < 0 || (n_grids > 0 && !grids)) { msg = "bad grid arrays"; return 1; }
  fp.type = f.texel_type;
  fp.views.resize((size_t)std::max(n_cams, 1));
  for (int c = 0; c < n_cams; ++c) rf_fview_prep(k4 + 4 * (size_t)c, q4 + 4 * (size_t)c, t3 + 3 * (size_t)c, &fp.views[(size_t)c]);
  fp.ftracks.resize(T);
  fp.kept.assign(T, 0);
  if (all) all->assign(T, {});
  const size_t align = f.texel_type == LT_TEXEL_F32 ? 8 : 4;
  std::vector<int> ids;
  std::vector<Cam> cams;
  std::vector<FSample> smps;
  int64_t g = 0;
  for (size_t n = 0; n < T; ++n) {
    const long long a = off[n];
    const int K = (int)(off[n + 1] - a);
    ids.assign(img + a, img + a + K);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const int I = (int)ids.size();
    if (I > kRfFeatMaxImages) {
      msg = "track " + std::to_string(n) + " has more than " + std::to_string(kRfFeatMaxImages) + " images (not built)";
      return 1;
    }
    if (g + I > n_grids) { msg = "fewer grids than images of the tracks"; return 1; }
    RfFTrack ft{(long long)fp.imgs.size(), (long long)fp.smps.size(), (long long)(fp.pairs.size() / 9), I, 0};
    cams.resize((size_t)I);
    for (int i = 0; i < I; ++i, ++g) {
      const lt_refine_grid &gr = grids[g];
      const std::string who = "the grid of track " + std::to_string(n) + ", image " + std::to_string(ids[(size_t)i]);
      if (!gr.data || gr.h < 1 || gr.w < 1) { msg = who + " is empty"; return 1; }
      if (gr.on_device && !device) { msg = who + " is on the device (host path)"; return 1; }
      if (reinterpret_cast<uintptr_t>(gr.data) % align) { msg = who + " is not aligned to two texels"; return 1; }
      if (!all_finite(gr.R, 4) || !all_finite(gr.tvec, 2)) { msg = who + " has a non-finite transform"; return 1; }
      const int cam = id2idx.at(ids[(size_t)i]);  // make_plan has checked the ids
      fp.imgs.push_back(RfFImg{gr.data, gr.h, gr.w, {gr.R[0], gr.R[1], gr.R[2], gr.R[3]}, {gr.tvec[0], gr.tvec[1]}, cam, 0});
      cam_build(k4 + 4 * (size_t)cam, q4 + 4 * (size_t)cam, t3 + 3 * (size_t)cam, &cams[(size_t)i]);
    }
    if (feat_samples(pl.line6.data() + 6 * n, K, img + a, l2d4 + 4 * a, ids, cams, t.sample_range_min, t.sample_range_max,
                     f.n_samples_feature, smps, msg)) {
      msg = "track " + std::to_string(n) + ": " + msg;
      return 1;
    }
    fp.kept[n] = (int)smps.size();
    for (const FSample &s : smps) {
      if (s.tgts.empty()) continue;  // contributes nothing
      RfFSample r;
      r.k[0] = s.k[0]; r.k[1] = s.k[1]; r.k[2] = s.k[2];
      r.weight = f.fconsis_multiplier / ((double)((double)smps.size() / 100.0) * (double)((double)s.tgts.size() / 5.0));  // refine.cc:394-396
      r.tgt0 = (long long)fp.tgts.size();
      r.ref = s.ref;
      r.n_tgt = (int)s.tgts.size();
      fp.tgts.insert(fp.tgts.end(), s.tgts.begin(), s.tgts.end());
      fp.smps.push_back(r);
      ++ft.n_smp;
    }
    fp.pairs.resize(fp.pairs.size() + 9 * (size_t)I * (size_t)I, 0.0);
    for (int r = 0; r < I; ++r)
      for (int c = 0; c < I; ++c)
        if (r != c)
          rf_fundamental(fp.views[(size_t)fp.imgs[(size_t)ft.img0 + (size_t)r].cam], fp.views[(size_t)fp.imgs[(size_t)ft.img0 + (size_t)c].cam],
                         fp.pairs.data() + 9 * ((size_t)ft.pair0 + (size_t)r * (size_t)I + (size_t)c));
    fp.ftracks[n] = ft;
    if (all) (*all)[n] = smps;
  }
  if (g != n_grids) { msg = "more grids than images of the tracks"; return 1; }
  return 0;
}

int check_config(const lt_refine_config *cfg, std::string &msg) {
  if (!cfg) { msg = "null configuration"; return 1; }
  if (!(cfg->geometric_alpha >= 0.0) || !(cfg->geometric_alpha <= 700.0)) { msg = "geometric_alpha outside [0, 700]"; return 1; }
  if (cfg->max_num_iterations < 0) { msg = "max_num_iterations is negative"; return 1; }
  return 0;
}

// the checks upstream makes (or fails without) and the tables of the kernels
int make_plan(const std::unordered_map<int, int> &id2idx, int64_t T, const double *line6, const int64_t *off,
              const int32_t *img, const double *l2d4, const double *l3d6, const lt_refine_config &cfg, Plan &pl,
              std::string &msg) {
  if (T < 0 || !off || (T > 0 && !line6)) { msg = "bad track arrays"; return 1; }
  msg = offsets_msg("track", T, off);
  if (!msg.empty()) return 1;
  for (int64_t n = 0; n < T; ++n) {
    if (off[n + 1] <= off[n]) { msg = "track " + std::to_string(n) + " has no supports"; return 1; }  // THROW_CHECK_GT(line3ds.size(), 0)
    if (off[n + 1] - off[n] > (1 << 28)) { msg = "too many supports in a track"; return 1; }
  }
  const long long S = T > 0 ? off[T] : 0;
  if (S > 0 && (!img || !l2d4 || !l3d6)) { msg = "null support arrays"; return 1; }
  if (!all_finite(line6, 6 * (size_t)T) || !all_finite(l2d4, 4 * (size_t)S) || !all_finite(l3d6, 6 * (size_t)S)) {
    msg = "non-finite coordinate";
    return 1;
  }
  pl.n_sup = S;
  pl.tracks.resize((size_t)T);
  pl.sup_cam.resize((size_t)S);
  pl.l2d.resize(4 * (size_t)S);
  pl.src.resize((size_t)S);
  pl.l3d.assign(l3d6, l3d6 + 6 * (size_t)S);
  pl.line6.assign(line6, line6 + 6 * (size_t)T);
  SupportOrder so;
  for (int64_t n = 0; n < T; ++n) {
    const long long a = off[n];
    const int K = (int)(off[n + 1] - a);
    int n_images;
    if (ingest_line_length("track", n, line6 + 6 * n, msg) || ingest_outliers("track", n, cfg.num_outliers_aggregator, K, msg) ||
        ingest_supports("track", n, img + a, K, id2idx, so, &n_images, msg, [&](int k, int x, int row) {
          pl.sup_cam[(size_t)(a + k)] = row;
          pl.src[(size_t)(a + k)] = a + x;
          for (int c = 0; c < 4; ++c) pl.l2d[4 * (size_t)(a + k) + c] = l2d4[4 * (a + x) + c];
        }))
      return 1;
    pl.tracks[(size_t)n] = RfTrack{a, K, (cfg.constant_line != 0 || n_images < cfg.min_num_images) ? 1 : 0};
  }
  return 0;
}

// ---- the host twins of the groups of k_refine_lm and k_refine_lm_terms (W lanes): the lanes are a loop ----
typedef RfGroup<LmHostLanes<kRfWidth>> HostGroup;

// where a support's heatmap comes from on the host: the caller's images
struct HostGrids {
  const TermsPlan &tp;
  const HmSet *hs;
  template <class Tx>
  RfGrid<Tx> grid(long long s) const {
    const size_t sl = (size_t)tp.sup_hm[(size_t)s];
    return RfGrid<Tx>{static_cast<const Tx *>(hs->data[sl]), hs->h[sl], hs->w[sl]};
  }
};
template <int W, bool HM, class Tx>
using HostGroupTerms = RfGroupTerms<LmHostLanes<W>, HM, Tx, HostGrids>;

// f(HostGroupTerms) for the instantiation the terms select, like launch_refine_lm_terms
template <class F>
void with_host_group(const double *tab, const double *ext, long long stride, const RfTrack &t, double alpha,
                     const TermsPlan &tp, const HmSet *hs, F &&f) {
  const HostGrids gr{tp, hs};
  if (!tp.cfg.use_heatmap) {
    HostGroupTerms<kRfTermWidth, false, float> g{{}, tab, ext, stride, t, alpha, tp.cfg, gr};
    f(g);
  } else if (hs->type == LT_TEXEL_F32) {
    HostGroupTerms<kRfTermWidth, true, float> g{{}, tab, ext, stride, t, alpha, tp.cfg, gr};
    f(g);
  } else {
    HostGroupTerms<kRfTermWidth, true, unsigned short> g{{}, tab, ext, stride, t, alpha, tp.cfg, gr};
    f(g);
  }
}

// the host twin of a wave of k_refine_lm_feat: the supports' half is RfGroupTerms over the wave's lanes; in the feature
// blocks' half the lanes are a loop, the tree is lm_tree_host
template <bool HM, class Tx>
struct HostGroupFeat {
  HostGroupTerms<kRfFeatLanes, HM, Tx> sup;  // the supports' blocks: lanes 0 .. kRfTermWidth - 1 of the wave
  const FeatPlan &fp;
  const RfFTrack &f;
  const RfFImg *imgs() const { return fp.imgs.data() + f.img0; }
  const double *pair(int ref, int tg) const { return fp.pairs.data() + 9 * ((size_t)f.pair0 + (size_t)ref * (size_t)f.n_img + (size_t)tg); }
  double cost(const double p[6]) const {
    double total = sup.cost_sum(p);
    if (f.n_smp == 0) return 0.5 * total;
    double d[3], m[3];
    rf_plucker_c<double>(p, p + 4, d, m);
    double c[kRfFeatMaxImages][3];
    for (int i = 0; i < f.n_img; ++i) rf_w2p<double>(fp.views[(size_t)imgs()[i].cam], d, m, c[i]);
    bool ok = true;
    for (int si = 0; si < f.n_smp; ++si) {
      const RfFSample &s = fp.smps[(size_t)f.smp0 + (size_t)si];
      const RfFImg &gr = imgs()[s.ref];
      double x, y, lx, ly, fref[kRfFeatLanes][2];
      const bool ok_ref = rf_feat_ref_xy<double>(c[s.ref], s, gr, &x, &y, &lx, &ly);
      for (int l = 0; l < kRfFeatLanes; ++l) rf_feat_value<Tx>(gr, ly, lx, l, fref[l]);
      for (int ti = 0; ti < s.n_tgt; ++ti) {
        const int tg = fp.tgts[(size_t)s.tgt0 + (size_t)ti];
        const RfFImg &gt = imgs()[tg];
        double tx, ty, part[kRfFeatLanes][1], sq;
        const bool ok_tgt = rf_feat_tgt_xy<double>(c[tg], pair(s.ref, tg), x, y, gt, &tx, &ty);
        for (int l = 0; l < kRfFeatLanes; ++l) part[l][0] = rf_feat_sq_lane<Tx>(gt, tx, ty, fref[l], l);
        lm_tree_host(part, 1, &sq);
        if (ok_ref && ok_tgt) total = total + rf_rho(s.weight, sq);
        else ok = false;
      }
    }
    return ok ? 0.5 * total : __builtin_inf();
  }
  // res: 128 residuals per block, failed: one flag per block, in block order (tests)
  bool linearise_res(const double p[6], double acc[kRfSums], double *res, int32_t *failed) const {
    Rf4 u[4], w[2], dm[6];
    rf_seed(p, u, w);
    rf_plucker<Rf4>(u, w, dm);
    sup.lin_sums(dm, acc, nullptr);
    if (f.n_smp == 0) return true;
    Rf4 d[3], m[3];
    rf_plucker_c<Rf4>(u, w, d, m);
    Rf4 c[kRfFeatMaxImages][3];
    for (int i = 0; i < f.n_img; ++i) rf_w2p<Rf4>(fp.views[(size_t)imgs()[i].cam], d, m, c[i]);
    bool ok = true;
    size_t b = 0;
    for (int si = 0; si < f.n_smp; ++si) {
      const RfFSample &s = fp.smps[(size_t)f.smp0 + (size_t)si];
      const RfFImg &gr = imgs()[s.ref];
      Rf4 x, y, lx, ly;
      const bool ok_ref = rf_feat_ref_xy<Rf4>(c[s.ref], s, gr, &x, &y, &lx, &ly);
      RfFRef ref[kRfFeatLanes];
      for (int l = 0; l < kRfFeatLanes; ++l) rf_feat_ref_lane<Tx>(gr, lx, ly, l, &ref[l]);
      for (int ti = 0; ti < s.n_tgt; ++ti, ++b) {
        const int tg = fp.tgts[(size_t)s.tgt0 + (size_t)ti];
        const RfFImg &gt = imgs()[tg];
        Rf4 tx, ty;
        const bool ok_tgt = rf_feat_tgt_xy<Rf4>(c[tg], pair(s.ref, tg), x, y, gt, &tx, &ty);
        double part[kRfFeatLanes][kRfFeatSums], blk[kRfFeatSums];
        for (int l = 0; l < kRfFeatLanes; ++l) {
          for (int o = 0; o < kRfFeatSums; ++o) part[l][o] = 0.0;
          rf_feat_block_lane<Tx>(gt, tx, ty, ref[l], l, part[l], res ? res + kRfChannels * b + 2 * (size_t)l : nullptr);
        }
        lm_tree_host(part, kRfFeatSums, blk);
        if (failed) failed[b] = (ok_ref && ok_tgt) ? 0 : 1;
        if (ok_ref && ok_tgt) {
          const double rho1 = rf_rho1(s.weight, blk[kRfSums]);
          for (int o = 0; o < kRfSums; ++o) acc[o] = acc[o] + rho1 * blk[o];
        } else {
          ok = false;
        }
      }
    }
    return ok;
  }
  void linearise(const double p[6], double acc[kRfSums]) const { linearise_res(p, acc, nullptr, nullptr); }
};

// f(HostGroupFeat) for the instantiation the call selects, like launch_refine_lm_feat
template <class F>
void with_host_group_feat(const double *tab, const double *ext, long long stride, const RfTrack &t, double alpha,
                          const TermsPlan &tp, const HmSet *hs, const FeatPlan &fp, const RfFTrack &ft, F &&f) {
  const bool f32 = fp.type == LT_TEXEL_F32;
  const HostGrids gr{tp, hs};
  if (!tp.cfg.use_heatmap) {
    if (f32) { HostGroupFeat<false, float> g{{{}, tab, ext, stride, t, alpha, tp.cfg, gr}, fp, ft}; f(g); }
    else { HostGroupFeat<false, unsigned short> g{{{}, tab, ext, stride, t, alpha, tp.cfg, gr}, fp, ft}; f(g); }
  } else {
    if (f32) { HostGroupFeat<true, float> g{{{}, tab, ext, stride, t, alpha, tp.cfg, gr}, fp, ft}; f(g); }
    else { HostGroupFeat<true, unsigned short> g{{{}, tab, ext, stride, t, alpha, tp.cfg, gr}, fp, ft}; f(g); }
  }
}

// k_refine_cut on the host: the same rank rule
void cut_host(const RfTrack &t, const double *l3d, int num_outliers, RfOut &o) {
  d3 dir, m;
  rf_infinite(o.p, &dir, &m);
  const double *l3 = l3d + 6 * t.s0;
  const d3 pref = rf_pref(dir, m, mk3(l3[0], l3[1], l3[2]));
  const long long n = 2 * (long long)t.n, lo = num_outliers, hi = n - 1 - num_outliers;
  const double nan = std::nan("");
  for (int c = 0; c < 6; ++c) o.seg[c] = nan;
  for (long long i = 0; i < n; ++i) {
    double v;
    bool is_lo, is_hi;
    rf_rank_test(l3, n, i, pref, dir, lo, hi, &v, &is_lo, &is_hi);
    if (is_lo) { o.seg[0] = pref.x + dir.x * v; o.seg[1] = pref.y + dir.y * v; o.seg[2] = pref.z + dir.z * v; }
    if (is_hi) { o.seg[3] = pref.x + dir.x * v; o.seg[4] = pref.y + dir.y * v; o.seg[5] = pref.z + dir.z * v; }
  }
}

// k_refine_prep's support table
void fill_support(const double *k4, const double *q4, const double *t3, const double *l, double *tab, long long stride) {
  rf_view_matrix(k4, q4, t3, tab, stride);
  tab[18 * stride] = l[0]; tab[19 * stride] = l[1];
  tab[20 * stride] = l[2]; tab[21 * stride] = l[3];
  const double dx = l[2] - l[0], dy = l[3] - l[1];
  tab[22 * stride] = std::sqrt(dx * dx + dy * dy) / 30.0;
}

// tp: the terms of the call, or null (then hs is not read)
void run_host(const Plan &pl, const double *k, const double *q, const double *t, const lt_refine_config &cfg, int n_threads,
              std::vector<RfOut> &out, const TermsPlan *tp = nullptr, const HmSet *hs = nullptr, const FeatPlan *fp = nullptr) {
  const long long S = pl.n_sup, T = (long long)pl.tracks.size();
  const long long stride = std::max<long long>(S, 1);
  std::vector<double> tab((size_t)kRfFields * (size_t)stride), ext(tp ? (size_t)kRfExtFields * (size_t)stride : 0);
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
#pragma omp parallel for num_threads(nt) schedule(static)
  for (long long i = 0; i < S; ++i) {
    const int cam = pl.sup_cam[(size_t)i];
    fill_support(k + 4 * (size_t)cam, q + 4 * (size_t)cam, t + 3 * (size_t)cam, pl.l2d.data() + 4 * i, tab.data() + i, stride);
    if (tp)
      rf_ext_prep(k + 4 * (size_t)cam, q + 4 * (size_t)cam, tp->vp_flag[(size_t)i] != 0, tp->vp3.data() + 3 * i,
                  ext.data() + i, stride);
  }
  out.resize((size_t)T);
#pragma omp parallel for num_threads(nt) schedule(dynamic, fp ? 1 : 16)
  for (long long n = 0; n < T; ++n) {
    RfOut &o = out[(size_t)n];
    const RfTrack &tr = pl.tracks[(size_t)n];
    rf_minimal(pl.line6.data() + 6 * n, o.p);
    if (fp) {
      with_host_group_feat(tab.data(), ext.data(), stride, tr, cfg.geometric_alpha, *tp, hs, *fp, fp->ftracks[(size_t)n], [&](auto &grp) {
        rf_lm_terms(grp, tr.constant != 0, cfg.max_num_iterations, o.p, &o.cost0, &o.cost1, &o.iters, &o.code);
      });
    } else if (tp) {
      with_host_group(tab.data(), ext.data(), stride, tr, cfg.geometric_alpha, *tp, hs, [&](auto &grp) {
        rf_lm_terms(grp, tr.constant != 0, cfg.max_num_iterations, o.p, &o.cost0, &o.cost1, &o.iters, &o.code);
      });
    } else {
      HostGroup grp{{}, tab.data(), stride, tr, cfg.geometric_alpha};
      rf_lm(grp, tr.constant != 0, cfg.max_num_iterations, o.p, &o.cost0, &o.cost1, &o.iters, &o.code);
    }
    cut_host(tr, pl.l3d.data(), cfg.num_outliers_aggregator, o);
  }
}

void copy_out(const RfOut *o, long long T, double *params6, double *seg6, double *cost2, int32_t *iters, int32_t *codes) {
  for (long long n = 0; n < T; ++n) {
    if (params6) std::copy(o[n].p, o[n].p + 6, params6 + 6 * n);
    if (seg6) std::copy(o[n].seg, o[n].seg + 6, seg6 + 6 * n);
    if (cost2) { cost2[2 * n] = o[n].cost0; cost2[2 * n + 1] = o[n].cost1; }
    if (iters) iters[n] = o[n].iters;
    if (codes) codes[n] = o[n].code;
  }
}

#ifndef LT_HOST_ONLY  // (tools/refine_feature_host_asan.cpp compiles the host twins alone: no context, no HIP runtime)
// upload of the plan, the three kernels, download into ctx->rf.out; d_k / d_q / d_t: the cameras on the device
// tp: the terms of the call, or null; with them k_refine_prep_terms runs too and k_refine_lm_terms replaces k_refine_lm
int run_device(lt_ctx *ctx, const Plan &pl, const double *d_k, const double *d_q, const double *d_t,
               const lt_refine_config &cfg, double t0, const TermsPlan *tp = nullptr, const FeatPlan *fp = nullptr) {
  const long long S = pl.n_sup, T = (long long)pl.tracks.size();
  static_assert(sizeof(RfOut) == 15 * sizeof(double), "RfOut is 15 doubles");
  ctx->rf.out.assign(15 * (size_t)T, 0.0);
  for (int k = 0; k < 4; ++k) ctx->rf.timers[k] = 0.0;
  if (T == 0) return LT_OK;
  if (T * kRfWidth / kRfBlock + 1 > (long long)INT_MAX / kRfBlock || S > ((long long)1 << 31))
    return fail(ctx, LT_ERR_ARGUMENT, "lt_refine: too many tracks for one call (split them)");
  hipStream_t st = ctx->stream;
  const long long stride = S;
  if (int rc = upload_vec(ctx, ctx->rf.d_cam, pl.sup_cam)) return rc;
  if (int rc = upload_vec(ctx, ctx->rf.d_l2d, pl.l2d)) return rc;
  if (int rc = upload_vec(ctx, ctx->rf.d_l3d, pl.l3d)) return rc;
  if (int rc = upload_vec(ctx, ctx->rf.d_line, pl.line6)) return rc;
  if (int rc = upload_vec(ctx, ctx->rf.d_tracks, pl.tracks)) return rc;
  ENSURE(ctx, ctx->rf.d_tab, 8 * (size_t)kRfFields * (size_t)stride);
  ENSURE(ctx, ctx->rf.d_out, sizeof(RfOut) * (size_t)T);
  if (tp) {
    if (int rc = upload_vec(ctx, ctx->rf.d_vp_flag, tp->vp_flag)) return rc;
    if (int rc = upload_vec(ctx, ctx->rf.d_vp3, tp->vp3)) return rc;
    if (int rc = upload_vec(ctx, ctx->rf.d_sup_hm, tp->sup_hm)) return rc;
    ENSURE(ctx, ctx->rf.d_ext, 8 * (size_t)kRfExtFields * (size_t)stride);
  }
  if (fp) {  // (the grids already hold device addresses: upload_grids)
    if (int rc = upload_vec(ctx, ctx->rf.d_f_tracks, fp->ftracks)) return rc;
    if (int rc = upload_vec(ctx, ctx->rf.d_f_imgs, fp->imgs)) return rc;
    if (int rc = upload_vec(ctx, ctx->rf.d_f_views, fp->views)) return rc;
    if (int rc = upload_vec(ctx, ctx->rf.d_f_smps, fp->smps)) return rc;
    if (int rc = upload_vec(ctx, ctx->rf.d_f_tgts, fp->tgts)) return rc;
    if (int rc = upload_vec(ctx, ctx->rf.d_f_pairs, fp->pairs)) return rc;
  }
  if (int rc = stream_sync(ctx)) return rc;
  const double t1 = now_ms();
  ctx->rf.timers[0] = t1 - t0;

  RfDev dev;
  dev.tracks = ctx->rf.d_tracks.as<RfTrack>();
  dev.n_tracks = T;
  dev.sup = ctx->rf.d_tab.as<double>();
  dev.stride = stride;
  dev.l3d = ctx->rf.d_l3d.as<double>();
  dev.alpha = cfg.geometric_alpha;
  dev.max_iter = cfg.max_num_iterations;
  dev.num_outliers = cfg.num_outliers_aggregator;
  RfOut *d_out = ctx->rf.d_out.as<RfOut>();
  Events<2> ev;  // around k_refine_lm
  if (int rc = ev.create(ctx)) return rc;
  launch_refine_prep(st, d_k, d_q, d_t, ctx->rf.d_cam.as<int>(), ctx->rf.d_l2d.as<double>(), S, ctx->rf.d_tab.as<double>(),
                     stride, ctx->rf.d_line.as<double>(), T, d_out);
  if (tp)
    launch_refine_prep_terms(st, d_k, d_q, ctx->rf.d_cam.as<int>(), ctx->rf.d_vp_flag.as<int>(), ctx->rf.d_vp3.as<double>(), S,
                             ctx->rf.d_ext.as<double>(), stride);
  if (int rc = ev.record(ctx, 0)) return rc;
  if (fp) {
    const RfDevTerms terms{ctx->rf.d_ext.as<double>(), ctx->rf.d_sup_hm.as<int>(), ctx->rf.d_hm_tab.as<RfHm>(),
                           ctx->rf.d_hm_tex.p, tp->cfg};
    const RfDevFeat feat{ctx->rf.d_f_tracks.as<RfFTrack>(), ctx->rf.d_f_imgs.as<RfFImg>(), ctx->rf.d_f_views.as<RfFView>(),
                         ctx->rf.d_f_smps.as<RfFSample>(), ctx->rf.d_f_tgts.as<int>(), ctx->rf.d_f_pairs.as<double>()};
    launch_refine_lm_feat(st, dev, terms, feat, fp->type == LT_TEXEL_F32, d_out);
  } else if (tp) {
    const RfDevTerms terms{ctx->rf.d_ext.as<double>(), ctx->rf.d_sup_hm.as<int>(), ctx->rf.d_hm_tab.as<RfHm>(),
                           ctx->rf.d_hm_tex.p, tp->cfg};
    launch_refine_lm_terms(st, dev, terms, ctx->rf.hm_type == LT_TEXEL_F32, d_out);
  } else {
    launch_refine_lm(st, dev, d_out);
  }
  if (int rc = ev.record(ctx, 1)) return rc;
  launch_refine_cut(st, dev, d_out);
  if (int rc = stream_sync(ctx)) return rc;
  const double t2 = now_ms();
  ctx->rf.timers[1] = t2 - t1;
  ctx->rf.timers[3] = ev.ms(0, 1);
  HIPCHK(ctx, hipMemcpyAsync(ctx->rf.out.data(), d_out, sizeof(RfOut) * (size_t)T, hipMemcpyDeviceToHost, st));
  if (int rc = stream_sync(ctx)) return rc;
  ctx->rf.timers[2] = now_ms() - t2;
  return LT_OK;
}

// the caller's cameras into the context's buffers (lt_refine_arrays and lt_refine_arrays_terms)
int upload_cameras(lt_ctx *ctx, int n_img, const double *kvec4, const double *qvec4, const double *tvec3) {
  const size_t nI = (size_t)std::max(n_img, 1);
  ENSURE(ctx, ctx->rf.d_k, 32 * nI);
  ENSURE(ctx, ctx->rf.d_q, 32 * nI);
  ENSURE(ctx, ctx->rf.d_t, 24 * nI);
  if (n_img > 0) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->rf.d_k.p, kvec4, 32 * (size_t)n_img, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->rf.d_q.p, qvec4, 32 * (size_t)n_img, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->rf.d_t.p, tvec3, 24 * (size_t)n_img, hipMemcpyHostToDevice, ctx->stream));
  }
  return LT_OK;
}
#endif  // LT_HOST_ONLY

}  // namespace

#ifndef LT_HOST_ONLY
namespace lt_impl {

// lt_refine_tracks (lt_tracks.cpp): the cameras of the context, resident since lt_init
int refine_with_ctx_cams(lt_ctx *ctx, int64_t T, const double *line6, const int64_t *off, const int32_t *img,
                         const double *l2d4, const double *l3d6, const lt_refine_config *cfg) {
  const std::string who = "lt_refine_tracks";
  const double t0 = now_ms();
  if (!ctx->inited || !ctx->d_kvec.p || !ctx->d_qvec.p || !ctx->d_tvec.p)
    return fail(ctx, LT_ERR_STATE, who + ": the context holds no cameras (lt_init first)");
  std::string msg;
  Plan pl;
  if (check_config(cfg, msg) || make_plan(ctx->id2idx, T, line6, off, img, l2d4, l3d6, *cfg, pl, msg))
    return fail(ctx, LT_ERR_ARGUMENT, who + ": " + msg);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return run_device(ctx, pl, ctx->d_kvec.as<double>(), ctx->d_qvec.as<double>(), ctx->d_tvec.as<double>(), *cfg, t0);
}

}  // namespace lt_impl
#endif  // LT_HOST_ONLY

extern "C" {

void lt_refine_config_default(lt_refine_config *cfg) {
  if (!cfg) return;
  cfg->geometric_alpha = 10.0;       // refinement_config.h:58-69
  cfg->min_num_images = 4;
  cfg->num_outliers_aggregator = 2;  // cfgs/triangulation/default.yaml:143
  cfg->num_outliers_aggregate = 2;
  cfg->max_num_iterations = 100;
  cfg->constant_line = 0;            // hybrid_bundle_adjustment_config.h:33
  cfg->pad_ = 0;
}

#ifndef LT_HOST_ONLY
int lt_refine_arrays(lt_ctx *ctx, int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4,
                     const double *tvec3, int64_t n_tracks, const double *line6, const int64_t *off, const int32_t *img,
                     const double *line2d4, const double *line3d6, const lt_refine_config *cfg) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::string who = "lt_refine_arrays";
  const double t0 = now_ms();
  std::string msg;
  std::unordered_map<int, int> id2idx;
  Plan pl;
  if (check_config(cfg, msg) || ingest_cams(n_img, img_ids, kvec4, qvec4, tvec3, id2idx, msg) ||
      make_plan(id2idx, n_tracks, line6, off, img, line2d4, line3d6, *cfg, pl, msg))
    return fail(ctx, LT_ERR_ARGUMENT, who + ": " + msg);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = upload_cameras(ctx, n_img, kvec4, qvec4, tvec3)) return rc;
  return run_device(ctx, pl, ctx->rf.d_k.as<double>(), ctx->rf.d_q.as<double>(), ctx->rf.d_t.as<double>(), *cfg, t0);
}
#endif  // LT_HOST_ONLY

void lt_refine_terms_default(lt_refine_terms *t) {
  if (!t) return;
  t->use_geometric = 1;          // refinement_config.h:54-79
  t->use_vp = 0;
  t->use_heatmap = 0;
  t->n_samples_heatmap = 10;
  t->vp_multiplier = 1.0;
  t->sample_range_min = 0.05;
  t->sample_range_max = 0.95;
  t->heatmap_multiplier = 1.0;
  t->texel_type = LT_TEXEL_F16;  // interpolation's dtype "float16" (cfgs/refinement/default.yaml)
  t->pad_ = 0;
}

#ifndef LT_HOST_ONLY
int lt_refine_set_heatmaps(lt_ctx *ctx, int n, const int32_t *img_ids, const int32_t *h, const int32_t *w,
                           const void *const *data, int texel_type) {
  if (!ctx) return LT_ERR_ARGUMENT;
  HmSet hs;
  std::string msg;
  if (check_heatmaps(n, img_ids, h, w, data, texel_type, hs, msg))
    return fail(ctx, LT_ERR_ARGUMENT, "lt_refine_set_heatmaps: " + msg);
  lt_refine_clear_heatmaps(ctx);  // a failure below leaves the context without heatmaps
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t px = texel_type == LT_TEXEL_F32 ? 4 : 2;
  std::vector<RfHm> tab((size_t)n);
  ENSURE(ctx, ctx->rf.d_hm_tex, std::max<size_t>(px * (size_t)hs.off.back(), 1));
  for (int i = 0; i < n; ++i) {
    tab[(size_t)i] = RfHm{hs.off[(size_t)i], h[i], w[i]};
    HIPCHK(ctx, hipMemcpyAsync(static_cast<char *>(ctx->rf.d_hm_tex.p) + px * (size_t)hs.off[(size_t)i], data[i],
                               px * (size_t)h[i] * (size_t)w[i], hipMemcpyHostToDevice, ctx->stream));
  }
  if (int rc = upload_vec(ctx, ctx->rf.d_hm_tab, tab)) return rc;
  if (int rc = stream_sync(ctx)) return rc;  // the caller's images may go after the call
  ctx->rf.hm_type = texel_type;
  ctx->rf.hm_ids.assign(img_ids, img_ids + n);
  ctx->rf.hm_h = hs.h;
  ctx->rf.hm_w = hs.w;
  return LT_OK;
}

int lt_refine_clear_heatmaps(lt_ctx *ctx) {
  if (!ctx) return LT_ERR_ARGUMENT;
  ++ctx->rf.hm_generation;
  ctx->rf.hm_ids.clear();
  ctx->rf.hm_h.clear();
  ctx->rf.hm_w.clear();
  return LT_OK;
}

int64_t lt_refine_heatmaps_generation(lt_ctx *ctx) { return ctx ? (int64_t)ctx->rf.hm_generation : 0; }

int lt_refine_arrays_terms(lt_ctx *ctx, int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4,
                           const double *tvec3, int64_t n_tracks, const double *line6, const int64_t *off,
                           const int32_t *img, const double *line2d4, const double *line3d6, const lt_refine_config *cfg,
                           const lt_refine_terms *terms, const int32_t *vp_flag, const double *vp3,
                           const int32_t *view_hw) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::string who = "lt_refine_arrays_terms";
  const double t0 = now_ms();
  std::string msg;
  if (check_terms(terms, msg)) return fail(ctx, LT_ERR_ARGUMENT, who + ": " + msg);
  if (!terms->use_vp && !terms->use_heatmap)
    return lt_refine_arrays(ctx, n_img, img_ids, kvec4, qvec4, tvec3, n_tracks, line6, off, img, line2d4, line3d6, cfg);
  std::unordered_map<int, int> id2idx;
  Plan pl;
  TermsPlan tp;
  HmSet hs;  // the context's heatmaps as the checks read them
  hs.type = ctx->rf.hm_type;
  hs.h = ctx->rf.hm_h;
  hs.w = ctx->rf.hm_w;
  for (size_t i = 0; i < ctx->rf.hm_ids.size(); ++i) hs.slot.emplace(ctx->rf.hm_ids[i], (int)i);
  if (check_config(cfg, msg) || ingest_cams(n_img, img_ids, kvec4, qvec4, tvec3, id2idx, msg) ||
      make_plan(id2idx, n_tracks, line6, off, img, line2d4, line3d6, *cfg, pl, msg) ||
      make_terms_plan(pl, img, *terms, vp_flag, vp3, view_hw, &hs, tp, msg))
    return fail(ctx, LT_ERR_ARGUMENT, who + ": " + msg);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = upload_cameras(ctx, n_img, kvec4, qvec4, tvec3)) return rc;
  return run_device(ctx, pl, ctx->rf.d_k.as<double>(), ctx->rf.d_q.as<double>(), ctx->rf.d_t.as<double>(), *cfg, t0, &tp);
}

int lt_refine_set_feature_maps(lt_ctx *ctx, int n, const int32_t *img_ids, const int32_t *h, const int32_t *w,
                               const void *const *data, int texel_type, int on_device) {
  if (!ctx) return LT_ERR_ARGUMENT;
  HmSet hs;  // the same checks as a heatmap's: distinct ids, positive sizes, a known texel type
  std::string msg;
  if (check_heatmaps(n, img_ids, h, w, data, texel_type, hs, msg))
    return fail(ctx, LT_ERR_ARGUMENT, "lt_refine_set_feature_maps: " + msg);
  const size_t px = texel_type == LT_TEXEL_F32 ? 4 : 2;
  for (int i = 0; i < n; ++i)
    if (reinterpret_cast<uintptr_t>(data[i]) % (2 * px))
      return fail(ctx, LT_ERR_ARGUMENT, "lt_refine_set_feature_maps: a map is not aligned to two texels");
  lt_refine_clear_feature_maps(ctx);  // a failure below leaves the context without feature maps
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<const void *> ptr((size_t)n);
  if (on_device) {
    for (int i = 0; i < n; ++i) ptr[(size_t)i] = data[i];
  } else {
    ENSURE(ctx, ctx->rf.d_ft_tex, std::max<size_t>(px * kRfChannels * (size_t)hs.off.back(), 1));
    for (int i = 0; i < n; ++i) {
      char *dst = static_cast<char *>(ctx->rf.d_ft_tex.p) + px * kRfChannels * (size_t)hs.off[(size_t)i];
      HIPCHK(ctx, hipMemcpyAsync(dst, data[i], px * kRfChannels * (size_t)h[i] * (size_t)w[i], hipMemcpyHostToDevice, ctx->stream));
      ptr[(size_t)i] = dst;
    }
    if (int rc = stream_sync(ctx)) return rc;  // the caller's maps may go after the call
  }
  ctx->rf.ft_type = texel_type;
  ctx->rf.ft_ids.assign(img_ids, img_ids + n);
  ctx->rf.ft_h = hs.h;
  ctx->rf.ft_w = hs.w;
  ctx->rf.ft_ptr = ptr;
  return LT_OK;
}

int lt_refine_clear_feature_maps(lt_ctx *ctx) {
  if (!ctx) return LT_ERR_ARGUMENT;
  ++ctx->rf.ft_generation;
  ctx->rf.ft_ids.clear();
  ctx->rf.ft_h.clear();
  ctx->rf.ft_w.clear();
  ctx->rf.ft_ptr.clear();
  return LT_OK;
}

int64_t lt_refine_feature_maps_generation(lt_ctx *ctx) { return ctx ? (int64_t)ctx->rf.ft_generation : 0; }

int lt_refine_arrays_feature(lt_ctx *ctx, int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4,
                             const double *tvec3, int64_t n_tracks, const double *line6, const int64_t *off,
                             const int32_t *img, const double *line2d4, const double *line3d6, const lt_refine_config *cfg,
                             const lt_refine_terms *terms, const int32_t *vp_flag, const double *vp3,
                             const int32_t *view_hw, const lt_refine_feature *feat, int64_t n_grids,
                             const lt_refine_grid *grids) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::string who = "lt_refine_arrays_feature";
  const double t0 = now_ms();
  std::string msg;
  if (check_feature(terms, feat, msg)) return fail(ctx, LT_ERR_ARGUMENT, who + ": " + msg);
  std::unordered_map<int, int> id2idx;
  Plan pl;
  TermsPlan tp;
  FeatPlan fp;
  HmSet hs;  // the context's heatmaps as the checks read them
  hs.type = ctx->rf.hm_type;
  hs.h = ctx->rf.hm_h;
  hs.w = ctx->rf.hm_w;
  for (size_t i = 0; i < ctx->rf.hm_ids.size(); ++i) hs.slot.emplace(ctx->rf.hm_ids[i], (int)i);
  if (check_config(cfg, msg) || ingest_cams(n_img, img_ids, kvec4, qvec4, tvec3, id2idx, msg) ||
      make_plan(id2idx, n_tracks, line6, off, img, line2d4, line3d6, *cfg, pl, msg) ||
      make_terms_plan(pl, img, *terms, vp_flag, vp3, view_hw, &hs, tp, msg))
    return fail(ctx, LT_ERR_ARGUMENT, who + ": " + msg);
  std::vector<lt_refine_grid> maps;  // the map form: the context's maps with the identity transform
  if (!grids) {
    if (n_grids != 0) return fail(ctx, LT_ERR_ARGUMENT, who + ": n_grids without grids");
    if (ctx->rf.ft_type != feat->texel_type && !ctx->rf.ft_ids.empty())
      return fail(ctx, LT_ERR_ARGUMENT, who + ": the feature maps' texel type is not the configuration's");
    std::unordered_map<int, size_t> slot;
    for (size_t i = 0; i < ctx->rf.ft_ids.size(); ++i) slot.emplace(ctx->rf.ft_ids[i], i);
    std::vector<int> ids;
    for (int64_t n = 0; n < n_tracks; ++n) {
      ids.assign(img + off[n], img + off[n + 1]);
      std::sort(ids.begin(), ids.end());
      ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
      for (int id : ids) {
        auto it = slot.find(id);
        if (it == slot.end())
          return fail(ctx, LT_ERR_ARGUMENT, who + ": image " + std::to_string(id) + " supports a track and has no feature map");
        const size_t sl = it->second;
        const int cam = id2idx.at(id);
        if (view_hw && view_hw[2 * cam] > 0 && view_hw[2 * cam + 1] > 0 &&
            (view_hw[2 * cam] != ctx->rf.ft_h[sl] || view_hw[2 * cam + 1] != ctx->rf.ft_w[sl]))
          return fail(ctx, LT_ERR_ARGUMENT, who + ": the feature map of image " + std::to_string(id) + " has not the size of its view");
        maps.push_back(lt_refine_grid{ctx->rf.ft_ptr[sl], ctx->rf.ft_h[sl], ctx->rf.ft_w[sl], {1.0, 0.0, 0.0, 1.0}, {0.0, 0.0}, 1, 0});
      }
    }
    grids = maps.data();
    n_grids = (int64_t)maps.size();
  }
  if (make_feat_plan(pl, id2idx, n_img, kvec4, qvec4, tvec3, off, img, line2d4, *terms, *feat, n_grids, grids, true, fp, msg))
    return fail(ctx, LT_ERR_ARGUMENT, who + ": " + msg);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // the call's host patches into one packed buffer, every patch at a multiple of 256 bytes; device patches stay in place
  const size_t px = feat->texel_type == LT_TEXEL_F32 ? 4 : 2;
  size_t total = 0;
  std::vector<size_t> at((size_t)n_grids, 0);
  for (int64_t g = 0; g < n_grids; ++g)
    if (!grids[g].on_device) {
      at[(size_t)g] = total;
      total += (px * kRfChannels * (size_t)grids[g].h * (size_t)grids[g].w + 255) / 256 * 256;
    }
  ENSURE(ctx, ctx->rf.d_f_tex, std::max<size_t>(total, 1));
  for (int64_t g = 0; g < n_grids; ++g)
    if (!grids[g].on_device) {
      char *dst = static_cast<char *>(ctx->rf.d_f_tex.p) + at[(size_t)g];
      HIPCHK(ctx, hipMemcpyAsync(dst, grids[g].data, px * kRfChannels * (size_t)grids[g].h * (size_t)grids[g].w,
                                 hipMemcpyHostToDevice, ctx->stream));
      fp.imgs[(size_t)g].tex = dst;
    }
  if (int rc = upload_cameras(ctx, n_img, kvec4, qvec4, tvec3)) return rc;
  return run_device(ctx, pl, ctx->rf.d_k.as<double>(), ctx->rf.d_q.as<double>(), ctx->rf.d_t.as<double>(), *cfg, t0, &tp, &fp);
}

int64_t lt_refine_num(lt_ctx *ctx) { return ctx ? (int64_t)(ctx->rf.out.size() / 15) : 0; }

int lt_refine_get(lt_ctx *ctx, double *params6, double *seg6, double *cost2, int32_t *iters, int32_t *codes) {
  if (!ctx) return LT_ERR_ARGUMENT;
  copy_out(reinterpret_cast<const RfOut *>(ctx->rf.out.data()), (long long)(ctx->rf.out.size() / 15), params6, seg6, cost2,
           iters, codes);
  return LT_OK;
}

int lt_refine_get_timers(lt_ctx *ctx, double out[4]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 4; ++k) out[k] = ctx->rf.timers[k];
  return LT_OK;
}
#endif  // LT_HOST_ONLY

static thread_local HostError g_host_error;
const char *lt_fn_refine_host_error(void) { return g_host_error.c_str(); }

int lt_fn_refine_host(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                      int64_t n_tracks, const double *line6, const int64_t *off, const int32_t *img,
                      const double *line2d4, const double *line3d6, const lt_refine_config *cfg, int n_threads,
                      double *params6, double *seg6, double *cost2, int32_t *iters, int32_t *codes) {
  std::string msg;
  std::unordered_map<int, int> id2idx;
  Plan pl;
  const bool bad = check_config(cfg, msg) || ingest_cams(n_img, img_ids, kvec4, qvec4, tvec3, id2idx, msg) ||
                   make_plan(id2idx, n_tracks, line6, off, img, line2d4, line3d6, *cfg, pl, msg);
  if (int rc = g_host_error.check("lt_fn_refine_host", bad, msg)) return rc;
  std::vector<RfOut> out;
  run_host(pl, kvec4, qvec4, tvec3, *cfg, n_threads, out);
  copy_out(out.data(), (long long)out.size(), params6, seg6, cost2, iters, codes);
  return LT_OK;
}

int lt_fn_refine_host_terms(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                            int64_t n_tracks, const double *line6, const int64_t *off, const int32_t *img,
                            const double *line2d4, const double *line3d6, const lt_refine_config *cfg,
                            const lt_refine_terms *terms, const int32_t *vp_flag, const double *vp3, const int32_t *view_hw,
                            int n_hm, const int32_t *hm_ids, const int32_t *hm_h, const int32_t *hm_w,
                            const void *const *hm_data, int n_threads, double *params6, double *seg6, double *cost2,
                            int32_t *iters, int32_t *codes) {
  std::string msg;
  if (check_terms(terms, msg)) return g_host_error.refuse("lt_fn_refine_host_terms", msg);
  if (!terms->use_vp && !terms->use_heatmap)
    return lt_fn_refine_host(n_img, img_ids, kvec4, qvec4, tvec3, n_tracks, line6, off, img, line2d4, line3d6, cfg,
                             n_threads, params6, seg6, cost2, iters, codes);
  std::unordered_map<int, int> id2idx;
  Plan pl;
  TermsPlan tp;
  HmSet hs;
  const bool bad = (terms->use_heatmap && check_heatmaps(n_hm, hm_ids, hm_h, hm_w, hm_data, terms->texel_type, hs, msg)) ||
                   check_config(cfg, msg) || ingest_cams(n_img, img_ids, kvec4, qvec4, tvec3, id2idx, msg) ||
                   make_plan(id2idx, n_tracks, line6, off, img, line2d4, line3d6, *cfg, pl, msg) ||
                   make_terms_plan(pl, img, *terms, vp_flag, vp3, view_hw, &hs, tp, msg);
  if (int rc = g_host_error.check("lt_fn_refine_host_terms", bad, msg)) return rc;
  std::vector<RfOut> out;
  run_host(pl, kvec4, qvec4, tvec3, *cfg, n_threads, out, &tp, &hs);
  copy_out(out.data(), (long long)out.size(), params6, seg6, cost2, iters, codes);
  return LT_OK;
}

void lt_refine_feature_default(lt_refine_feature *f) {
  if (!f) return;
  f->use_feature = 1;
  f->n_samples_feature = 100;    // refinement_config.h:82-88
  f->fconsis_multiplier = 1.0;
  f->channels = kRfChannels;
  f->texel_type = LT_TEXEL_F16;
}

int lt_fn_refine_host_feature(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                              int64_t n_tracks, const double *line6, const int64_t *off, const int32_t *img,
                              const double *line2d4, const double *line3d6, const lt_refine_config *cfg,
                              const lt_refine_terms *terms, const int32_t *vp_flag, const double *vp3, const int32_t *view_hw,
                              int n_hm, const int32_t *hm_ids, const int32_t *hm_h, const int32_t *hm_w,
                              const void *const *hm_data, const lt_refine_feature *feat, int64_t n_grids,
                              const lt_refine_grid *grids, int n_threads, double *params6, double *seg6, double *cost2,
                              int32_t *iters, int32_t *codes) {
  std::string msg;
  std::unordered_map<int, int> id2idx;
  Plan pl;
  TermsPlan tp;
  FeatPlan fp;
  HmSet hs;
  const bool bad =
      check_feature(terms, feat, msg) ||
      (terms->use_heatmap && check_heatmaps(n_hm, hm_ids, hm_h, hm_w, hm_data, terms->texel_type, hs, msg)) ||
      check_config(cfg, msg) || ingest_cams(n_img, img_ids, kvec4, qvec4, tvec3, id2idx, msg) ||
      make_plan(id2idx, n_tracks, line6, off, img, line2d4, line3d6, *cfg, pl, msg) ||
      make_terms_plan(pl, img, *terms, vp_flag, vp3, view_hw, &hs, tp, msg) ||
      make_feat_plan(pl, id2idx, n_img, kvec4, qvec4, tvec3, off, img, line2d4, *terms, *feat, n_grids, grids, false, fp, msg);
  if (int rc = g_host_error.check("lt_fn_refine_host_feature", bad, msg)) return rc;
  std::vector<RfOut> out;
  run_host(pl, kvec4, qvec4, tvec3, *cfg, n_threads, out, &tp, &hs, &fp);
  copy_out(out.data(), (long long)out.size(), params6, seg6, cost2, iters, codes);
  return LT_OK;
}

int lt_fn_refine_eval_feature(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                              const double line6[6], int64_t K, const int32_t *img, const double *line2d4, double alpha,
                              const lt_refine_terms *terms, const lt_refine_feature *feat, int64_t n_grids,
                              const lt_refine_grid *grids, const double *params6, int64_t cap_samples, int64_t cap_blocks,
                              int32_t *n_kept, int32_t *sample_ref, double *sample_line, int32_t *sample_ntgt,
                              int32_t *targets, int32_t *n_blocks, double *residuals, int32_t *failed, double *cost,
                              double g[4], double H[16]) {
  std::string msg;
  auto bad = [&](const std::string &m) { return g_host_error.refuse("lt_fn_refine_eval_feature", m); };
  if (K < 1 || K > (1 << 28) || !line6 || !(alpha >= 0.0) || !(alpha <= 700.0)) return bad("bad track arrays");
  if (check_feature(terms, feat, msg)) return bad(msg);
  if (terms->use_vp || terms->use_heatmap) return bad("the VP and heatmap terms are lt_fn_refine_eval_terms'");
  lt_refine_config cfg;
  lt_refine_config_default(&cfg);
  cfg.geometric_alpha = alpha;
  cfg.min_num_images = 0;
  cfg.num_outliers_aggregator = 0;
  const int64_t off[2] = {0, K};
  const std::vector<double> l3d(6 * (size_t)K, 0.0);
  std::unordered_map<int, int> id2idx;
  Plan pl;
  TermsPlan tp;
  FeatPlan fp;
  HmSet hs;
  std::vector<std::vector<FSample>> all;
  if (ingest_cams(n_img, img_ids, kvec4, qvec4, tvec3, id2idx, msg) ||
      make_plan(id2idx, 1, line6, off, img, line2d4, l3d.data(), cfg, pl, msg) ||
      make_terms_plan(pl, img, *terms, nullptr, nullptr, nullptr, &hs, tp, msg) ||
      make_feat_plan(pl, id2idx, n_img, kvec4, qvec4, tvec3, off, img, line2d4, *terms, *feat, n_grids, grids, false, fp, msg, &all))
    return bad(msg);
  g_host_error.clear();
  std::vector<int> ids(img, img + K);
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  const std::vector<FSample> &smps = all[0];
  size_t nb = 0;
  for (const FSample &s : smps) nb += s.tgts.size();
  if ((int64_t)smps.size() > cap_samples || (int64_t)nb > cap_blocks) return bad("more samples or blocks than the outputs hold");
  if (n_kept) *n_kept = (int32_t)smps.size();
  if (n_blocks) *n_blocks = (int32_t)nb;
  size_t ti = 0;
  for (size_t i = 0; i < smps.size(); ++i) {
    if (sample_ref) sample_ref[i] = ids[(size_t)smps[i].ref];
    if (sample_line) std::copy(smps[i].k, smps[i].k + 3, sample_line + 3 * i);
    if (sample_ntgt) sample_ntgt[i] = (int32_t)smps[i].tgts.size();
    for (int tg : smps[i].tgts) {
      if (targets) targets[ti] = ids[(size_t)tg];
      ++ti;
    }
  }
  double p[6];
  if (params6) std::copy(params6, params6 + 6, p);
  else rf_minimal(line6, p);
  std::vector<double> tab((size_t)kRfFields * (size_t)K), ext((size_t)kRfExtFields * (size_t)K);
  for (int64_t i = 0; i < K; ++i) {
    const size_t cam = (size_t)pl.sup_cam[(size_t)i];
    fill_support(kvec4 + 4 * cam, qvec4 + 4 * cam, tvec3 + 3 * cam, pl.l2d.data() + 4 * i, tab.data() + i, (long long)K);
    rf_ext_prep(kvec4 + 4 * cam, qvec4 + 4 * cam, false, tp.vp3.data() + 3 * i, ext.data() + i, (long long)K);
  }
  with_host_group_feat(tab.data(), ext.data(), (long long)K, pl.tracks[0], alpha, tp, &hs, fp, fp.ftracks[0], [&](auto &grp) {
    if (cost) *cost = grp.cost(p);
    double acc[kRfSums];
    grp.linearise_res(p, acc, residuals, failed);
    sums_to_gH<4>(acc, g, H);
  });
  return LT_OK;
}

int lt_fn_refine_eval_terms(int64_t K, const double *cam11, const double *line2d4, const double params6[6], double alpha,
                            const lt_refine_terms *terms, const int32_t *vp_flag, const double *vp3, const int32_t *hm_h,
                            const int32_t *hm_w, const void *const *hm_data, double *residuals, int32_t *failed,
                            double *cost, double g[4], double H[16]) {
  std::string msg;
  if (K < 1 || K > (1 << 28) || !cam11 || !line2d4 || !params6 || !(alpha >= 0.0) || !(alpha <= 700.0) ||
      check_terms(terms, msg))
    return LT_ERR_ARGUMENT;
  Plan pl;  // one track, the supports already in residual order, every support its own camera row
  pl.n_sup = K;
  pl.sup_cam.resize((size_t)K);
  pl.src.resize((size_t)K);
  std::iota(pl.sup_cam.begin(), pl.sup_cam.end(), 0);
  std::iota(pl.src.begin(), pl.src.end(), 0ll);
  pl.l2d.assign(line2d4, line2d4 + 4 * (size_t)K);
  std::vector<int32_t> ids((size_t)K);
  std::iota(ids.begin(), ids.end(), 0);
  TermsPlan tp;
  HmSet hs;
  if ((terms->use_heatmap && check_heatmaps((int)K, ids.data(), hm_h, hm_w, hm_data, terms->texel_type, hs, msg)) ||
      make_terms_plan(pl, ids.data(), *terms, vp_flag, vp3, nullptr, &hs, tp, msg))
    return LT_ERR_ARGUMENT;
  std::vector<double> tab((size_t)kRfFields * (size_t)K), ext((size_t)kRfExtFields * (size_t)K);
  for (int64_t i = 0; i < K; ++i) {
    const double *c = cam11 + 11 * i;
    fill_support(c, c + 4, c + 8, line2d4 + 4 * i, tab.data() + i, (long long)K);
    rf_ext_prep(c, c + 4, tp.vp_flag[(size_t)i] != 0, tp.vp3.data() + 3 * i, ext.data() + i, (long long)K);
  }
  const RfTrack tr{0, (int)K, 0};
  const size_t per = 3 + (size_t)tp.cfg.n_samples;
  if (residuals) std::fill(residuals, residuals + per * (size_t)K, std::nan(""));
  with_host_group(tab.data(), ext.data(), (long long)K, tr, alpha, tp, &hs, [&](auto &grp) {
    if (cost) *cost = grp.cost(params6);
    double acc[kRfSums];
    const bool ok = grp.linearise_res(params6, acc, residuals);
    if (failed) *failed = ok ? 0 : 1;
    sums_to_gH<4>(acc, g, H);
  });
  return LT_OK;
}

int lt_fn_refine_eval(int64_t K, const double *cam11, const double *line2d4, const double params6[6], double alpha,
                      double *residuals, double *cost, double g[4], double H[16]) {
  if (K < 1 || !cam11 || !line2d4 || !params6 || !(alpha >= 0.0) || !(alpha <= 700.0)) return LT_ERR_ARGUMENT;
  std::vector<double> tab((size_t)kRfFields * (size_t)K);
  for (int64_t i = 0; i < K; ++i) {
    const double *c = cam11 + 11 * i, *l = line2d4 + 4 * i;
    rf_view_matrix(c, c + 4, c + 8, tab.data() + i, (long long)K);
    tab[18 * K + i] = l[0]; tab[19 * K + i] = l[1]; tab[20 * K + i] = l[2]; tab[21 * K + i] = l[3];
    const double dx = l[2] - l[0], dy = l[3] - l[1];
    tab[22 * K + i] = std::sqrt(dx * dx + dy * dy) / 30.0;
  }
  const RfTrack tr{0, (int)K, 0};
  HostGroup grp{{}, tab.data(), (long long)K, tr, alpha};
  if (cost) *cost = grp.cost(params6);
  double acc[kRfSums];
  grp.linearise(params6, acc);
  sums_to_gH<4>(acc, g, H);
  if (residuals) {
    Rf4 u[4], w[2], dm[6];
    rf_seed(params6, u, w);
    rf_plucker<Rf4>(u, w, dm);
    double scratch[kRfSums] = {0};
    for (int64_t i = 0; i < K; ++i) rf_accumulate(rf_load(tab.data(), K, i), dm, alpha, scratch, residuals + 2 * i);
  }
  return LT_OK;
}

int lt_fn_lm_step(int n, const double *acc, double mu, double *dl, double *md) {
  if ((n != 4 && n != 6) || !acc || !dl || !md) return -1;
  for (int i = 0; i < n; ++i) dl[i] = std::nan("");
  *md = std::nan("");
  return n == 4 ? lm_step<4>(acc, mu, dl, md) : lm_step<6>(acc, mu, dl, md);
}

int lt_fn_refine_cut(int64_t K, const double *line3d6, const double params6[6], int num_outliers, double seg6[6]) {
  if (K < 1 || K > (1 << 28) || !line3d6 || !params6 || !seg6 || num_outliers < 0 || num_outliers > 2 * K - 1 ||
      !all_finite(line3d6, 6 * (size_t)K))
    return LT_ERR_ARGUMENT;
  RfOut o;
  std::copy(params6, params6 + 6, o.p);
  cut_host(RfTrack{0, (int)K, 0}, line3d6, num_outliers, o);
  std::copy(o.seg, o.seg + 6, seg6);
  return LT_OK;
}

int lt_fn_refine_explog(int which, int64_t n, const double *x, double *out) {
  if (n < 0 || (n > 0 && (!x || !out)) || (which != 0 && which != 1)) return LT_ERR_ARGUMENT;
  for (int64_t k = 0; k < n; ++k) {
    if (which == 0 ? !(x[k] >= 0.0 && x[k] <= 700.0) : !(x[k] >= 1.0 && x[k] < kMaxDist)) return LT_ERR_ARGUMENT;
    out[k] = which == 0 ? lt_exp(x[k]) : lt_log(x[k]);
  }
  return LT_OK;
}

int lt_fn_refine_minimal(const double line6[6], double params6[6]) {
  if (!line6 || !params6 || !all_finite(line6, 6)) return LT_ERR_ARGUMENT;
  const double dx = line6[0] - line6[3], dy = line6[1] - line6[4], dz = line6[2] - line6[5];
  if (!(std::sqrt((dx * dx + dy * dy) + dz * dz) > 0.0)) return LT_ERR_ARGUMENT;
  rf_minimal(line6, params6);
  return LT_OK;
}

int lt_fn_refine_infinite(const double params6[6], double dm6[6]) {
  if (!params6 || !dm6) return LT_ERR_ARGUMENT;
  d3 d, m;
  rf_infinite(params6, &d, &m);
  dm6[0] = d.x; dm6[1] = d.y; dm6[2] = d.z;
  dm6[3] = m.x; dm6[4] = m.y; dm6[5] = m.z;
  return LT_OK;
}

}  // extern "C"
