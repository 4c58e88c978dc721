// lt_sfm.cpp -- limap.pointsfm's SfmModel (pointsfm/sfm_model.{h,cc} over colmap::mvs::Model): the visual neighbours
// of every image -- step [A] of limap.runners.line_triangulation, `compute_metainfos` -- and the robust ranges.
// DESIGN §21 is the definition.  This unit is the device path (lt_sfm_neighbors: lt_kernels_sfm.hip, one key sort);
// the host path from the same inline expressions of lt_sfm.h (lt_fn_sfm_neighbors_host) and the ranges
// (lt_fn_sfm_ranges: host work) are in lt_sfm_host.cpp.

#include "lt_host.h"
#include "lt_bpt.h"
#include "lt_sfm_host.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include <omp.h>

using namespace lt;
using namespace lt_impl;

namespace {

// bytes of device memory the keys of one call may take (two key buffers and the sort's scratch); a model with more
// instance slots than fit is refused.  LT_TEST_SFM_KEY_BUDGET lowers it for the tests.
constexpr unsigned long long kSfmKeyBudget = 32ull << 30;
// pair records the first launch of k_sfm_segments has room for; a model with more runs it a second time
constexpr unsigned long long kSfmPairCap = 1ull << 22;

}  // namespace

extern "C" {

int lt_sfm_neighbors(lt_ctx *ctx, int n_img, const float *R9, const float *T3, int64_t n_pts, const float *xyz,
                     const int64_t *track_off, const int32_t *track_img, int kind, int64_t num_images,
                     double min_triangulation_angle, int64_t *n_neighbors, int64_t *n_pairs) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::string who = "lt_sfm_neighbors: ";
  SfmPrep m;
  std::string msg;
  double t0 = now_ms();
  if (sfm_prepare(n_img, R9, T3, n_pts, xyz, track_off, track_img, kind, num_images, min_triangulation_angle, m, msg))
    return fail(ctx, LT_ERR_ARGUMENT, msg.rfind("unknown", 0) == 0 ? msg : who + msg);
  lt_host::SfmState &sf = ctx->sf;
  for (double &t : sf.timers) t = 0.0;
  sf.nb_off.assign((size_t)n_img + 1, 0);
  sf.nb.clear();
  sf.n_pairs = 0;
  if (n_neighbors) *n_neighbors = 0;
  if (n_pairs) *n_pairs = 0;
  const long long E = m.n_slots;
  if (n_img == 0 || E == 0) return LT_OK;  // no image pair shares a point: every list is empty

  unsigned long long budget = kSfmKeyBudget;
  if (const char *e = test_switch("LT_TEST_SFM_KEY_BUDGET")) budget = std::strtoull(e, nullptr, 10);
  const size_t tmp_bytes = bpt_sort_keys_temp_bytes(E);
  if (16ull * (unsigned long long)E + tmp_bytes > budget ||
      (E + kSfmBlock - 1) / kSfmBlock > (long long)INT_MAX)
    return fail(ctx, LT_ERR_ARGUMENT,
                who + "the model has E = " + std::to_string(E) + " pair instances; their keys need " +
                    std::to_string(16ull * (unsigned long long)E + tmp_bytes) + " bytes on the device, the budget is " +
                    std::to_string(budget) + " (split the model's points, or use the host path)");

  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const float gate = sfm_gate_of(min_triangulation_angle);
  const long long n_el = track_off[n_pts];
  // ---- upload ----
  if (int rc = upload_vec(ctx, sf.d_pair_off, m.pair_off)) return rc;
  if (int rc = upload_vec(ctx, sf.d_centres, m.centres)) return rc;
  if (int rc = upload_vec(ctx, sf.d_npts, m.n_points)) return rc;
  ENSURE(ctx, sf.d_track_off, 8 * ((size_t)n_pts + 1));
  ENSURE(ctx, sf.d_track_img, 4 * (size_t)n_el);
  ENSURE(ctx, sf.d_xyz, 12 * (size_t)n_pts);
  HIPCHK(ctx, hipMemcpyAsync(sf.d_track_off.p, track_off, 8 * ((size_t)n_pts + 1), hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(sf.d_track_img.p, track_img, 4 * (size_t)n_el, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(sf.d_xyz.p, xyz, 12 * (size_t)n_pts, hipMemcpyHostToDevice, st));
  ENSURE(ctx, sf.d_keys, 8 * (size_t)E);
  ENSURE(ctx, sf.d_keys2, 8 * (size_t)E);
  ENSURE(ctx, sf.d_tmp, std::max<size_t>(tmp_bytes, 8));
  ENSURE(ctx, sf.d_cnt, 4 * (size_t)n_img);
  ENSURE(ctx, sf.d_nb_cnt, 4 * (size_t)n_img);
  ENSURE(ctx, sf.d_off, 8 * ((size_t)n_img + 1));
  ENSURE(ctx, sf.d_nb_off, 8 * ((size_t)n_img + 1));
  if (int rc = stream_sync(ctx)) return rc;  // the caller's arrays are free again
  double t1 = now_ms();
  sf.timers[0] = t1 - t0;

  // ---- keys, sort, pair records ----
  Events<6> ev;  // start, keys done, sort done, around the segment launch that fitted, end
  if (int rc = ev.create(ctx)) return rc;
  if (int rc = ev.record(ctx, 0)) return rc;
  launch_sfm_pairs(st, E, n_pts, sf.d_pair_off.as<long long>(), sf.d_track_off.as<long long>(),
                   sf.d_track_img.as<int>(), sf.d_centres.as<double>(), sf.d_xyz.as<float>(),
                   sf.d_keys.as<unsigned long long>());
  if (int rc = ev.record(ctx, 1)) return rc;
  if (launch_bpt_sort_keys(st, sf.d_tmp.p, tmp_bytes, E, sf.d_keys.as<unsigned long long>(),
                           sf.d_keys2.as<unsigned long long>()) != 0)
    return fail(ctx, LT_ERR_HIP, who + "the key sort failed");
  if (int rc = ev.record(ctx, 2)) return rc;
  const unsigned long long max_pairs = (unsigned long long)n_img * (unsigned long long)(n_img - 1) / 2;
  unsigned long long capacity = std::max(1ull, std::min({(unsigned long long)E, max_pairs, kSfmPairCap}));
  if (const char *e = test_switch("LT_TEST_SFM_PAIR_CAP")) capacity = std::max(1ull, std::strtoull(e, nullptr, 10));
  unsigned long long U = 0;
  int attempts = 0;
  // [counter (8 B, padded to 16) | capacity records of 16 B]
  if (int rc = run_counted(ctx, sf.d_pairs, 16, sizeof(SfmPair), capacity,
                           [&](void *items, unsigned long long cap, unsigned long long *d_cnt) {
        if (int rc = ev.record(ctx, 3)) return rc;
        launch_sfm_segments(st, E, sf.d_keys2.as<unsigned long long>(), static_cast<SfmPair *>(items), cap, d_cnt);
        return ev.record(ctx, 4);
      }, &U, &attempts))
    return rc;
  sf.timers[7] = (double)attempts;
  sf.n_pairs = (long long)U;
  if (n_pairs) *n_pairs = (int64_t)U;
  long long total = 0;
  double t2 = now_ms(), t3 = t2;
  if (U > 0) {
    // ---- partner lists, selection ----
    const SfmPair *d_pairs = reinterpret_cast<const SfmPair *>(sf.d_pairs.as<char>() + 16);
    ENSURE(ctx, sf.d_part, 4 * 2 * (size_t)U);
    ENSURE(ctx, sf.d_nb, 4 * 2 * (size_t)U);
    ENSURE(ctx, sf.d_score, 8 * 2 * (size_t)U);
    HIPCHK(ctx, hipMemsetAsync(sf.d_cnt.p, 0, 4 * (size_t)n_img, st));
    launch_sfm_partners(st, 0, (long long)U, d_pairs, sf.d_cnt.as<unsigned>(), nullptr, nullptr);
    launch_sfm_scan(st, n_img, sf.d_cnt.as<unsigned>(), sf.d_off.as<long long>());
    HIPCHK(ctx, hipMemsetAsync(sf.d_cnt.p, 0, 4 * (size_t)n_img, st));
    launch_sfm_partners(st, 1, (long long)U, d_pairs, sf.d_cnt.as<unsigned>(), sf.d_off.as<long long>(),
                        sf.d_part.as<unsigned>());
    launch_sfm_select(st, n_img, sf.d_off.as<long long>(), sf.d_part.as<unsigned>(), sf.d_score.as<double>(), d_pairs,
                      sf.d_npts.as<int>(), kind, gate, (long long)num_images, sf.d_nb.as<unsigned>(),
                      sf.d_nb_cnt.as<unsigned>());
    launch_sfm_scan(st, n_img, sf.d_nb_cnt.as<unsigned>(), sf.d_nb_off.as<long long>());
    if (int rc = download(ctx, sf.nb_off, sf.d_nb_off.p, (size_t)n_img + 1)) return rc;
    if (int rc = stream_sync(ctx)) return rc;  // the second count the host needs: the neighbours of all images
    total = sf.nb_off.back();
    if (total < 0 || total > 2 * (long long)U)
      return fail(ctx, LT_ERR_RUNTIME, who + "the selection kernel returned a count out of range");
    ENSURE(ctx, sf.d_dense, 4 * (size_t)std::max<long long>(total, 1));
    launch_sfm_compact(st, n_img, sf.d_off.as<long long>(), sf.d_nb.as<unsigned>(), sf.d_nb_cnt.as<unsigned>(),
                       sf.d_nb_off.as<long long>(), sf.d_dense.as<int>());
    if (int rc = ev.record(ctx, 5)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
    t3 = now_ms();
    if (int rc = download(ctx, sf.nb, sf.d_dense.p, (size_t)total)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
    for (int v : sf.nb)
      if (v < 0 || v >= n_img) return fail(ctx, LT_ERR_RUNTIME, who + "the selection kernel returned an image out of range");
  }
  sf.timers[1] = t3 - t1;
  sf.timers[2] = now_ms() - t3;
  sf.timers[3] = ev.ms(0, 1);
  sf.timers[4] = ev.ms(1, 2);
  sf.timers[5] = ev.ms(3, 4);
  sf.timers[6] = ev.ms(4, 5);
  if (n_neighbors) *n_neighbors = (int64_t)total;
  return LT_OK;
}

int lt_sfm_get(lt_ctx *ctx, int64_t *nb_off, int32_t *nb) {
  if (!ctx) return LT_ERR_ARGUMENT;
  if (nb_off) std::copy(ctx->sf.nb_off.begin(), ctx->sf.nb_off.end(), nb_off);
  if (nb) std::copy(ctx->sf.nb.begin(), ctx->sf.nb.end(), nb);
  return LT_OK;
}

int lt_sfm_get_pairs(lt_ctx *ctx, int32_t *ij, int32_t *shared, float *angle) {
  if (!ctx) return LT_ERR_ARGUMENT;
  std::vector<SfmPair> pairs;
  if (ctx->sf.n_pairs > 0) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = download(ctx, pairs, ctx->sf.d_pairs.as<char>() + 16, (size_t)ctx->sf.n_pairs)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
  }
  // the records arrive in the order their waves drew slots; (i, j) is unique, so this order is not
  std::sort(pairs.begin(), pairs.end(), [](const SfmPair &a, const SfmPair &b) { return a.ij < b.ij; });
  sfm_copy_pairs(pairs, ij, shared, angle);
  return LT_OK;
}

int lt_sfm_get_timers(lt_ctx *ctx, double out[8]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 8; ++k) out[k] = ctx->sf.timers[k];
  return LT_OK;
}

}  // extern "C"
