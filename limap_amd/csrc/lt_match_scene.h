// lt_match_scene.h -- the host path the descriptor matcher (lt_match.cpp) and the SOLD2 matcher (lt_match_wunsch.cpp)
// share: the check of a scene's CSR arrays and neighbour list, the descriptors' way to the device, the collection of
// the result into the state lt_match_get / lt_match_get_scores / lt_match_get_timers read, and the pieces of the two
// host restatements that are one definition (the value bound, the fmaf chain, the top-k selection).  DESIGN §17, §20.
#pragma once

#include "lt_host.h"
#include "lt_match.h"

#include <algorithm>
#include <cmath>
#include <functional>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

namespace lt_impl {

inline bool values_ok(const float *v, long long n) {
  int bad = 0;
#pragma omp parallel for reduction(| : bad) schedule(static)
  for (long long k = 0; k < n; ++k) bad |= !(std::fabs(v[k]) <= lt::kMatchMaxAbs);
  return !bad;
}

// score(i, j): the fmaf chain in ascending k from +0.0f
inline float dot_chain(const float *a, const float *b, int dim) {
  float acc = 0.0f;
  for (int k = 0; k < dim; ++k) acc = std::fmaf(a[k], b[k], acc);
  return acc;
}

// per row i < n1 the kk best columns j < n2 under match_key(score(i, j), j), best first, at best[i * kk ...]
template <class Score>
void best_columns(long long n1, long long n2, int kk, Score score, std::vector<unsigned long long> &best) {
  best.assign((size_t)n1 * kk, 0ull);
#pragma omp parallel
  {
    std::vector<unsigned long long> keys((size_t)n2);
#pragma omp for schedule(static)
    for (long long i = 0; i < n1; ++i) {
      for (long long j = 0; j < n2; ++j) keys[(size_t)j] = lt::match_key(score(i, j), (unsigned)j);
      std::partial_sort(keys.begin(), keys.begin() + kk, keys.end(), std::greater<unsigned long long>());
      std::copy(keys.begin(), keys.begin() + kk, best.begin() + i * kk);
    }
  }
}

// The arrays of a scene call: `offs` are its CSR arrays over the images by name, the descriptors' last; image_msg(m)
// is what is wrong with image m, or nullptr; data_null: an input array that the descriptors need is missing.
template <class ImageMsg>
int check_scene(lt_ctx *ctx, const char *fn, int n_img, std::initializer_list<std::pair<const char *, const int64_t *>> offs,
                const int64_t *pair_off, const int32_t *pair_nb, bool data_null, ImageMsg image_msg) {
  const std::string who = std::string(fn) + ": ";
  bool null_off = n_img < 0 || !pair_off;
  for (const auto &o : offs) null_off = null_off || !o.second;
  if (null_off) return fail(ctx, LT_ERR_ARGUMENT, who + "bad image count or null offsets");
  for (const auto &o : offs)
    if (int rc = check_offsets(ctx, fn, o.first, n_img, o.second)) return rc;
  if (int rc = check_offsets(ctx, fn, "pair", n_img, pair_off)) return rc;
  for (int m = 0; m < n_img; ++m)
    if (const char *msg = image_msg(m)) return fail(ctx, LT_ERR_ARGUMENT, who + msg);
  const long long n_desc = (offs.end() - 1)->second[n_img], n_pairs = pair_off[n_img];
  if (n_pairs > (1 << 30)) return fail(ctx, LT_ERR_ARGUMENT, who + "too many pairs");
  if ((n_desc > 0 && data_null) || (n_pairs > 0 && !pair_nb)) return fail(ctx, LT_ERR_ARGUMENT, who + "null input");
  for (long long p = 0; p < n_pairs; ++p)
    if (pair_nb[p] < 0 || pair_nb[p] >= n_img) return fail(ctx, LT_ERR_ARGUMENT, who + "a neighbour is not an image");
  return LT_OK;
}

// The descriptors on the context's device (which this selects for the rest of the call): a host array is checked here
// and goes up into mt.d_desc; a device array is used in place after the same rejection by a kernel of its own, before
// any matching launch.
inline int stage_desc(lt_ctx *ctx, const char *fn, const float *desc, long long n_values, bool on_dev,
                      const float **d_desc) {
  const std::string bad = std::string(fn) + ": a descriptor value is not finite or above 2^57 in magnitude";
  if (!on_dev && !values_ok(desc, n_values)) return fail(ctx, LT_ERR_ARGUMENT, bad);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  *d_desc = desc;
  if (!on_dev) {
    ENSURE(ctx, ctx->mt.d_desc, sizeof(float) * (size_t)std::max<long long>(n_values, 1));
    if (n_values)
      HIPCHK(ctx, hipMemcpyAsync(ctx->mt.d_desc.p, desc, sizeof(float) * (size_t)n_values, hipMemcpyHostToDevice, ctx->stream));
    *d_desc = ctx->mt.d_desc.as<float>();
  } else if (n_values) {
    ENSURE(ctx, ctx->mt.d_flag, 16);
    HIPCHK(ctx, hipMemsetAsync(ctx->mt.d_flag.p, 0, 4, ctx->stream));
    lt::launch_match_check(ctx->stream, desc, n_values, ctx->mt.d_flag.as<int>());
    int flag = 0;
    HIPCHK(ctx, hipMemcpyAsync(&flag, ctx->mt.d_flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = stream_sync(ctx)) return rc;
    if (flag) return fail(ctx, LT_ERR_ARGUMENT, bad);
  }
  return LT_OK;
}

// The result of a scene call into ctx->mt, after the kernels (t2: the host time behind them).  On entry mt.row_off
// holds the pairs' offsets into the output slots; d_col / d_score are the buffers that hold the slots' columns and
// scores: 2 bytes per row come down, the scores only when asked for.  kk: columns kept per line and pair.  Mutual: a
// pair's rows are the slots that survived the cross check.
inline int collect_rows(lt_ctx *ctx, const DevBuf &d_col, const DevBuf &d_score, std::vector<int> &&kk, bool want_scores,
                        bool mutual, double t2, int64_t *n_rows) {
  lt_host::MatchState &mt = ctx->mt;
  const size_t slots = (size_t)mt.row_off.back();
  if (int rc = download(ctx, mt.col, d_col.p, slots)) return rc;
  mt.score.clear();
  if (want_scores)
    if (int rc = download(ctx, mt.score, d_score.p, slots)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  const double t3 = now_ms();
  mt.timers[2] = t3 - t2;

  mt.kk = std::move(kk);
  mt.slot_off = mt.row_off;
  if (mutual)
    for (size_t p = 0; p + 1 < mt.row_off.size(); ++p) {
      long long n = 0;
      for (long long s = mt.slot_off[p]; s < mt.slot_off[p + 1]; ++s) n += mt.col[(size_t)s] != 0xffff;
      mt.row_off[p + 1] = mt.row_off[p] + n;
    }
  mt.mutual = mutual;
  mt.dense = false;
  mt.timers[3] = now_ms() - t3;
  if (n_rows) *n_rows = (int64_t)mt.row_off.back();
  return LT_OK;
}

}  // namespace lt_impl
