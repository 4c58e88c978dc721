// lt_match.cpp -- line-descriptor matching (limap.line2d: L2D2Matcher, NNEndpointsMatcher top-k) for a whole scene in
// one call: validation, one upload of the descriptors, the launches of lt_kernels_match.hip on the context's stream,
// context-owned rows with getters, timers; and the host restatement lt_fn_match_pair_host of the same semantics
// (std::fmaf in a plain loop).  The entry point is four steps: its configuration check, its tasks and units, the stage
// of lt_match_scene.h, its launches and that header's collection of the result.  DESIGN §17.

#include "lt_match_scene.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace lt;
using namespace lt_impl;

namespace {

int check_config(const lt_match_config *cfg, int dim, std::string &msg) {
  if (!cfg) { msg = "null configuration"; return 1; }
  if (cfg->kind != LT_MATCH_L2D2 && cfg->kind != LT_MATCH_ENDPOINTS) { msg = "unknown matcher kind"; return 1; }
  if (cfg->topk < 0) { msg = "topk is negative"; return 1; }
  if (cfg->topk > LT_MATCH_MAX_TOPK) { msg = "topk above LT_MATCH_MAX_TOPK (64)"; return 1; }
  if (cfg->kind == LT_MATCH_ENDPOINTS && cfg->topk == 0) {
    msg = "the endpoints matcher has no mutual nearest-neighbour form here (topk == 0 is Sinkhorn in limap)";
    return 1;
  }
  if (dim < 8 || dim > LT_MATCH_MAX_DIM || (dim & 7)) {
    msg = "descriptor width must be a multiple of 8 in [8, 256]";
    return 1;
  }
  return 0;
}

}  // namespace

extern "C" {

int lt_match_scene(lt_ctx *ctx, int n_img, const int64_t *desc_off, const float *desc, int dim, const int64_t *pair_off,
                   const int32_t *pair_nb, const lt_match_config *cfg, int64_t *n_rows) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const char *fn = "lt_match_scene";
  const std::string who = std::string(fn) + ": ";
  std::string msg;
  if (check_config(cfg, dim, msg)) return fail(ctx, LT_ERR_ARGUMENT, who + msg);
  const int rpl = cfg->kind == LT_MATCH_ENDPOINTS ? 2 : 1;  // descriptor rows per line
  if (int rc = check_scene(ctx, fn, n_img, {{"descriptor", desc_off}}, pair_off, pair_nb, !desc, [&](int m) -> const char * {
        const int64_t n = desc_off[m + 1] - desc_off[m];
        if (n % rpl) return "an image has an odd number of endpoints";
        return n / rpl > kMatchMaxLines ? "more than 65535 lines in an image" : nullptr;
      }))
    return rc;
  const long long n_desc = desc_off[n_img], n_pairs = pair_off[n_img];
  double t0 = now_ms();

  // ---- tasks (a pair each; mutual: the swapped pairs behind them), units, output slots ----
  const bool mutual = cfg->topk == 0;
  const int topk = mutual ? 1 : cfg->topk;
  std::vector<MatchTask> tasks((size_t)n_pairs * (mutual ? 2 : 1));
  std::vector<int> kk((size_t)n_pairs);
  std::vector<long long> &row_off = ctx->mt.row_off;
  row_off.assign((size_t)n_pairs + 1, 0);
  long long slots = 0;
  int kcap = 0;
  {
    long long p = 0;
    for (int m = 0; m < n_img; ++m)
      for (; p < pair_off[m + 1]; ++p) {
        const int nb = pair_nb[p];
        MatchTask &T = tasks[(size_t)p];
        T.a0 = desc_off[m];
        T.na = (int)(desc_off[m + 1] - desc_off[m]);
        T.b0 = desc_off[nb];
        T.nb = (int)(desc_off[nb + 1] - desc_off[nb]);
        T.kk = kk[(size_t)p] = T.na > 0 ? std::min(topk, T.nb / rpl) : 0;
        T.out0 = slots;
        T.pad_ = 0;
        slots += (long long)(T.na / rpl) * T.kk;
        row_off[(size_t)p + 1] = slots;  // (mutual: an upper bound, replaced by collect_rows)
        kcap = std::max(kcap, T.kk);
      }
  }
  if (mutual)
    for (long long p = 0; p < n_pairs; ++p) {
      const MatchTask &F = tasks[(size_t)p];
      MatchTask &B = tasks[(size_t)(n_pairs + p)];
      B = MatchTask{F.b0, F.a0, slots, F.nb, F.na, F.kk, 0};
      slots += (long long)(B.na / rpl) * B.kk;
    }
  if (slots >= (1ll << 40)) return fail(ctx, LT_ERR_ARGUMENT, who + "too many result rows");
  const int waves = kcap ? match_waves(dim, kcap) : 1;
  std::vector<MatchUnit> units;
  for (size_t t = 0; t < tasks.size(); ++t)
    if (tasks[t].kk > 0)
      for (int r0 = 0; r0 < tasks[t].na; r0 += kMatchTile * waves) units.push_back(MatchUnit{(int)t, r0});
  if (units.size() > 0x7fffffffull) return fail(ctx, LT_ERR_ARGUMENT, who + "too many row tiles");

  // ---- upload ----
  const float *d_desc = nullptr;
  if (int rc = stage_desc(ctx, fn, desc, n_desc * dim, cfg->desc_on_device != 0, &d_desc)) return rc;
  if (int rc = upload_vec(ctx, ctx->mt.d_tasks, tasks)) return rc;
  if (int rc = upload_vec(ctx, ctx->mt.d_units, units)) return rc;
  ENSURE(ctx, ctx->mt.d_col, 2 * (size_t)std::max<long long>(slots, 1) + 16);
  ENSURE(ctx, ctx->mt.d_score, 4 * (size_t)std::max<long long>(slots, 1));
  if (int rc = stream_sync(ctx)) return rc;
  double t1 = now_ms();
  ctx->mt.timers[0] = t1 - t0;

  // ---- kernels ----
  hipStream_t st = ctx->stream;
  launch_match_topk(st, cfg->kind, dim, kcap, waves, ctx->mt.d_tasks.as<MatchTask>(), ctx->mt.d_units.as<MatchUnit>(),
                    (int)units.size(), d_desc, ctx->mt.d_col.as<unsigned short>(), ctx->mt.d_score.as<float>());
  if (mutual)
    launch_match_mutual(st, ctx->mt.d_tasks.as<MatchTask>(), (int)n_pairs, rpl, ctx->mt.d_col.as<unsigned short>());
  if (int rc = stream_sync(ctx)) return rc;
  double t2 = now_ms();
  ctx->mt.timers[1] = t2 - t1;

  return collect_rows(ctx, ctx->mt.d_col, ctx->mt.d_score, std::move(kk), cfg->want_scores != 0, mutual, t2, n_rows);
}

int lt_match_get(lt_ctx *ctx, int64_t *row_off, int32_t *rows2) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::vector<long long> &off = ctx->mt.row_off, &soff = ctx->mt.slot_off;
  if (row_off) std::copy(off.begin(), off.end(), row_off);
  if (!rows2 || off.empty()) return LT_OK;
  const long long n_pairs = (long long)off.size() - 1;
  if (ctx->mt.dense) {  // lt_match_dense_pairs: a row per slot, its line kept beside its column
    for (long long s = 0; s < off.back(); ++s) {
      rows2[2 * s] = ctx->mt.dense_line[(size_t)s];
      rows2[2 * s + 1] = (int32_t)ctx->mt.col[(size_t)s];
    }
    return LT_OK;
  }
#pragma omp parallel for schedule(dynamic, 8)
  for (long long p = 0; p < n_pairs; ++p) {
    const int kk = ctx->mt.kk[(size_t)p];
    int32_t *out = rows2 + 2 * off[(size_t)p];
    for (long long s = soff[(size_t)p]; s < soff[(size_t)p + 1]; ++s) {
      const unsigned short c = ctx->mt.col[(size_t)s];
      if (ctx->mt.mutual && c == 0xffff) continue;
      *out++ = (int32_t)((s - soff[(size_t)p]) / kk);
      *out++ = (int32_t)c;
    }
  }
  return LT_OK;
}

int lt_match_get_scores(lt_ctx *ctx, float *scores) {
  if (!ctx) return LT_ERR_ARGUMENT;
  if (!scores) return LT_OK;
  const long long slots = ctx->mt.slot_off.empty() ? 0 : ctx->mt.slot_off.back();
  if ((long long)ctx->mt.score.size() != slots)
    return fail(ctx, LT_ERR_STATE, "lt_match_get_scores: the last lt_match_scene did not ask for scores (want_scores)");
  for (long long s = 0; s < slots; ++s)
    if (!(ctx->mt.mutual && ctx->mt.col[(size_t)s] == 0xffff)) *scores++ = ctx->mt.score[(size_t)s];
  return LT_OK;
}

int lt_match_get_timers(lt_ctx *ctx, double out[4]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 4; ++k) out[k] = ctx->mt.timers[k];
  return LT_OK;
}

int lt_fn_match_pair_host(const float *desc1, int64_t n1, const float *desc2, int64_t n2, int dim,
                          const lt_match_config *cfg, int32_t *rows2, float *scores, int64_t *n_rows) {
  std::string msg;
  if (check_config(cfg, dim, msg) || n1 < 0 || n2 < 0 || !n_rows) return LT_ERR_ARGUMENT;
  const int rpl = cfg->kind == LT_MATCH_ENDPOINTS ? 2 : 1;
  if (n1 % rpl || n2 % rpl || n1 / rpl > kMatchMaxLines || n2 / rpl > kMatchMaxLines) return LT_ERR_ARGUMENT;
  if ((n1 && !desc1) || (n2 && !desc2)) return LT_ERR_ARGUMENT;
  if (!values_ok(desc1, n1 * dim) || !values_ok(desc2, n2 * dim)) return LT_ERR_ARGUMENT;
  const long long m1 = n1 / rpl, m2 = n2 / rpl;
  const bool mutual = cfg->topk == 0;
  const int kk = (int)std::min<long long>(mutual ? 1 : cfg->topk, m2);
  *n_rows = 0;
  if (m1 == 0 || m2 == 0) return LT_OK;
  auto line_score = [&](long long i, long long j) {
    if (rpl == 1) return dot_chain(desc1 + i * dim, desc2 + j * dim, dim);
    const float *a0 = desc1 + 2 * i * dim, *a1 = a0 + dim, *b0 = desc2 + 2 * j * dim, *b1 = b0 + dim;
    return match_endpoint_score(dot_chain(a0, b0, dim), dot_chain(a1, b1, dim), dot_chain(a0, b1, dim),
                                dot_chain(a1, b0, dim));
  };
  std::vector<unsigned long long> best, col_best;  // per line its kk best columns; mutual: per column its best line
  best_columns(m1, m2, kk, line_score, best);
  if (mutual) best_columns(m2, m1, 1, [&](long long j, long long i) { return line_score(i, j); }, col_best);
  long long n = 0;
  for (long long i = 0; i < m1; ++i)
    for (int t = 0; t < kk; ++t) {
      const unsigned long long key = best[(size_t)(i * kk + t)];
      const unsigned j = match_key_col(key);
      if (mutual && match_key_col(col_best[j]) != (unsigned)i) continue;
      if (rows2) { rows2[2 * n] = (int32_t)i; rows2[2 * n + 1] = (int32_t)j; }
      if (scores) scores[n] = match_key_score(key);
      ++n;
    }
  *n_rows = n;
  return LT_OK;
}

}  // extern "C"
