// lt_sfm_host.cpp -- the host-only half of limap_amd.pointsfm: validation and the tables both paths start
// from (sfm_prepare), the host path of the visual neighbours (lt_fn_sfm_neighbors_host: the inline expressions of
// lt_sfm.h, OpenMP, one sort) and the robust ranges (lt_fn_sfm_ranges).  Nothing here touches the device or the
// context, so this unit links on its own.

#include "lt_hostutil.h"
#include "lt_sfm_host.h"
#include "lt_twin.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <parallel/algorithm>

#include <omp.h>

using namespace lt;
using namespace lt_impl;

namespace lt_impl {

int sfm_prepare(int n_img, const float *R9, const float *T3, int64_t n_pts, const float *xyz, const int64_t *track_off,
            const int32_t *track_img, int kind, int64_t num_images, double min_angle_deg, SfmPrep &m, std::string &msg) {
  if (n_img < 0 || n_img > kSfmMaxImages) { msg = "image count outside [0, 65535]"; return 1; }
  if (n_pts < 0) { msg = "bad point count"; return 1; }
  if (kind < 0 || kind > 2) { msg = "neighbour type outside 0 (overlap), 1 (iou), 2 (dice)"; return 1; }
  if (num_images < 0) { msg = "negative number of neighbours"; return 1; }
  if (!std::isfinite(min_angle_deg)) { msg = "non-finite min_triangulation_angle"; return 1; }
  if ((n_img > 0 && (!R9 || !T3)) || (n_pts > 0 && !xyz)) { msg = "null poses or points"; return 1; }
  msg = offsets_msg("track", n_pts, track_off);
  if (!msg.empty()) return 1;
  const long long n_el = track_off[n_pts];
  if (n_el > INT_MAX) { msg = "more than 2^31 - 1 track elements"; return 1; }
  if (n_el > 0 && !track_img) { msg = "null track elements"; return 1; }
  if (!all_finite(R9, 9ll * n_img) || !all_finite(T3, 3ll * n_img)) { msg = "non-finite pose"; return 1; }
  if (!all_finite(xyz, 3 * n_pts)) { msg = "non-finite point coordinate"; return 1; }
  m.n_img = n_img;
  m.n_pts = n_pts;
  m.n_points.assign((size_t)n_img, 0);
  for (long long k = 0; k < n_el; ++k) {
    const int i = track_img[k];
    if (i < 0 || i >= n_img) { msg = "unknown image index " + std::to_string(i) + " in a point track"; return 1; }
    m.n_points[(size_t)i] += 1;
  }
  // ComputeProjectionCenter: C = -R^T T in float32 (the model stores R and T as float32), widened
  m.centres.resize(3 * (size_t)n_img);
  for (int i = 0; i < n_img; ++i) {
    const float *R = R9 + 9 * (size_t)i, *T = T3 + 3 * (size_t)i;
    for (int c = 0; c < 3; ++c) {
      const float s = (-R[c]) * T[0] + (-R[3 + c]) * T[1] + (-R[6 + c]) * T[2];
      if (!std::isfinite(s)) { msg = "non-finite pose (the projection centre overflows float32)"; return 1; }
      m.centres[3 * (size_t)i + c] = (double)s;
    }
  }
  m.pair_off.assign((size_t)n_pts + 1, 0);
  for (long long p = 0; p < n_pts; ++p) {
    const long long L = track_off[p + 1] - track_off[p];
    m.pair_off[(size_t)p + 1] = m.pair_off[(size_t)p] + L * (L - 1) / 2;  // L < 2^31: below 2^61, and the sum is
    if (m.pair_off[(size_t)p + 1] > (1ll << 50)) { msg = "more than 2^50 instance slots"; return 1; }  // checked as it grows
  }
  m.n_slots = m.pair_off[(size_t)n_pts];
  return 0;
}

void sfm_copy_pairs(const std::vector<SfmPair> &pairs, int32_t *ij, int32_t *shared, float *angle) {
  for (size_t k = 0; k < pairs.size(); ++k) {
    if (ij) { ij[2 * k] = (int32_t)(pairs[k].ij >> 16); ij[2 * k + 1] = (int32_t)(pairs[k].ij & 0xffffu); }
    if (shared) shared[k] = (int32_t)pairs[k].shared;
    if (angle) angle[k] = sfm_from_bits32(pairs[k].angle_bits);
  }
}

}  // namespace lt_impl

namespace {

// ---- the host path: the same keys, a sort, the same records, the same total order ----
struct HostResult {
  std::vector<long long> nb_off{0};
  std::vector<int> nb;
  std::vector<SfmPair> pairs;
  HostError err;
};
thread_local HostResult t_host;

void host_neighbors(const SfmPrep &m, const float *xyz, const int64_t *track_off, const int32_t *track_img, int kind,
                    long long num_images, float gate, int nt, HostResult &out) {
  const long long E = m.n_slots;
  std::vector<unsigned long long> keys((size_t)E);
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets are passed through as long long");
  const long long *toff = reinterpret_cast<const long long *>(track_off);
#pragma omp parallel for num_threads(nt) schedule(static)
  for (long long e = 0; e < E; ++e)
    keys[(size_t)e] = sfm_slot_key(e, m.n_pts, m.pair_off.data(), toff, track_img, m.centres.data(), xyz);
  __gnu_parallel::sort(keys.begin(), keys.end(), std::less<unsigned long long>(),
                       __gnu_parallel::default_parallel_tag((unsigned)nt));
  out.pairs.clear();
  for (long long s = 0; s < E;) {
    const unsigned top = (unsigned)(keys[(size_t)s] >> 32);
    if (top == 0xffffffffu) break;  // the skipped slots sort last
    long long e = s + 1;
    while (e < E && (unsigned)(keys[(size_t)e] >> 32) == top) ++e;
    const long long n = e - s;
    out.pairs.push_back(SfmPair{top, (unsigned)n, (unsigned)keys[(size_t)(s + sfm_percentile_index(n))], 0u});
    s = e;
  }
  struct Partner {
    double score;
    unsigned idx;
  };
  std::vector<std::vector<Partner>> kept((size_t)m.n_img);
  for (const SfmPair &p : out.pairs) {
    if (!(sfm_from_bits32(p.angle_bits) >= gate)) continue;
    const unsigned i = p.ij >> 16, j = p.ij & 0xffffu;
    kept[i].push_back(Partner{sfm_score(kind, p.shared, m.n_points[i], m.n_points[j]), j});
    kept[j].push_back(Partner{sfm_score(kind, p.shared, m.n_points[j], m.n_points[i]), i});
  }
  const auto before = [](const Partner &a, const Partner &b) { return sfm_better(a.score, a.idx, b.score, b.idx); };
#pragma omp parallel for num_threads(nt) schedule(dynamic, 16)
  for (int i = 0; i < m.n_img; ++i) {
    std::vector<Partner> &v = kept[(size_t)i];
    const size_t take = (size_t)std::min<long long>((long long)v.size(), num_images);
    std::partial_sort(v.begin(), v.begin() + take, v.end(), before);
    v.resize(take);
  }
  out.nb_off.assign((size_t)m.n_img + 1, 0);
  out.nb.clear();
  for (int i = 0; i < m.n_img; ++i) {
    for (const Partner &p : kept[(size_t)i]) out.nb.push_back((int)p.idx);
    out.nb_off[(size_t)i + 1] = (long long)out.nb.size();
  }
}

}  // namespace

extern "C" {

int lt_fn_sfm_neighbors_host(int n_img, const float *R9, const float *T3, int64_t n_pts, const float *xyz,
                             const int64_t *track_off, const int32_t *track_img, int kind, int64_t num_images,
                             double min_triangulation_angle, int n_threads, int64_t *n_neighbors, int64_t *n_pairs) {
  HostResult &out = t_host;
  out.err.clear();
  out.nb_off.assign(1, 0);
  out.nb.clear();
  out.pairs.clear();
  SfmPrep m;
  if (sfm_prepare(n_img, R9, T3, n_pts, xyz, track_off, track_img, kind, num_images, min_triangulation_angle, m, out.err.text))
    return LT_ERR_ARGUMENT;
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
  host_neighbors(m, xyz, track_off, track_img, kind, (long long)num_images, sfm_gate_of(min_triangulation_angle), nt, out);
  if (n_neighbors) *n_neighbors = (int64_t)out.nb.size();
  if (n_pairs) *n_pairs = (int64_t)out.pairs.size();
  return LT_OK;
}

int lt_fn_sfm_host_get(int64_t *nb_off, int32_t *nb, int32_t *ij, int32_t *shared, float *angle) {
  const HostResult &r = t_host;
  if (nb_off) std::copy(r.nb_off.begin(), r.nb_off.end(), nb_off);
  if (nb) std::copy(r.nb.begin(), r.nb.end(), nb);
  sfm_copy_pairs(r.pairs, ij, shared, angle);
  return LT_OK;
}

const char *lt_fn_sfm_host_error(void) { return t_host.err.c_str(); }

int lt_fn_sfm_ranges(int64_t n_pts, const float *xyz, double range_lo, double range_hi, double k_stretch, double lo[3],
                     double hi[3]) {
  std::string &err = t_host.err.text;
  err.clear();
  if (!lo || !hi) { err = "lt_fn_sfm_ranges: null output"; return LT_ERR_ARGUMENT; }
  if (n_pts <= 0 || !xyz) { err = "lt_fn_sfm_ranges: the model has no points"; return LT_ERR_ARGUMENT; }
  if (!all_finite(xyz, 3 * n_pts)) { err = "lt_fn_sfm_ranges: non-finite point coordinate"; return LT_ERR_ARGUMENT; }
  // get_robust_range: data[data.size() * kMinPercentile] with a float percentile: a float product, truncated
  const float size_f = (float)(size_t)n_pts;
  const float at_lo = size_f * (float)range_lo, at_hi = size_f * (float)range_hi;
  if (!(at_lo >= 0.0f) || !(at_hi >= 0.0f) || !(at_lo < size_f) || !(at_hi < size_f) || (size_t)at_lo >= (size_t)n_pts ||
      (size_t)at_hi >= (size_t)n_pts) {
    err = "lt_fn_sfm_ranges: range_robust indexes outside the " + std::to_string((long long)n_pts) + " sorted values";
    return LT_ERR_ARGUMENT;
  }
  const size_t i_lo = (size_t)at_lo, i_hi = (size_t)at_hi;
  const float k = (float)k_stretch;
  std::vector<float> data((size_t)n_pts);
  for (int c = 0; c < 3; ++c) {
    for (int64_t p = 0; p < n_pts; ++p) data[(size_t)p] = xyz[3 * p + c];
    std::nth_element(data.begin(), data.begin() + i_lo, data.end());
    float first = data[i_lo];
    std::nth_element(data.begin(), data.begin() + i_hi, data.end());
    float second = data[i_hi];
    const float diff = second - first;
    first -= k * diff;
    second += k * diff;
    lo[c] = (double)first;
    hi[c] = (double)second;
  }
  return LT_OK;
}

}  // extern "C"
